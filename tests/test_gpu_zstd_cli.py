"""GPU: the sigtk-amd CLI and the job API on a BLOW5 file with zstd records (tests/golden/sp1_dna.zstd_svb.blow5: the
records of sp1_dna.blow5, each one ZSTD_compress level 1 frame) -- the reference's goldens byte for byte, with the
records decoded on the GPU (the default) and on the host threads (--host-inflate), in file order and by read id."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import zstd_craft
from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
IDS = ["00011a60-dd92-4aad-be1d-59a33545ab1d", "0448591b-036c-4cc7-a702-6c542ccc07de", "03880e3d-b79d-4bd8-aab4-15724f1331af"]


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


@pytest.fixture(scope="module")
def zst(tmp_path_factory):
    """a copy of the fixture (read-id mode writes an index beside the file) and of sp1_dna.blow5"""
    d = tmp_path_factory.mktemp("zstd")
    paths = {}
    for name in ("sp1_dna.zstd_svb.blow5", "sp1_dna.blow5"):
        paths[name] = str(d / name)
        open(paths[name], "wb").write(open(os.path.join(GOLDEN, name), "rb").read())
    return paths["sp1_dna.zstd_svb.blow5"], paths["sp1_dna.blow5"]


def out(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("fname,tool", [
    ("sp1_dna.stat.tsv", ["stat"]), ("sp1_dna.event_c.tsv", ["event", "-c"]), ("sp1_dna.jnn.tsv", ["jnn"]),
    ("sp1_dna.jnn_c.tsv", ["jnn", "-c"]), ("sp1_dna.prefix.tsv", ["prefix"]), ("sp1_dna.prefix_stat.tsv", ["prefix", "--print-stat"]),
    ("sp1_dna.ent.tsv", ["ent"]), ("sp1_dna.pa3.tsv", ["pa"]),
])
def test_goldens_from_the_zstd_file(cli, zst, fname, tool):
    z, plain = zst
    ids = IDS if tool == ["pa"] else []
    assert out(cli, *tool, z, *ids) == gold(fname)
    assert out(cli, *tool, "--host-inflate", z, *ids) == gold(fname)
    if not ids and tool != ["ent"]:               # three reads by id: what the zlib file gives for them (`ent` takes no ids)
        want = out(cli, *tool, plain, *IDS)
        assert out(cli, *tool, z, *IDS) == want and out(cli, *tool, "--host-inflate", z, *IDS) == want
        assert want.count(b"\n") >= 3


def test_small_batches_keep_file_order(cli, zst):
    assert out(cli, "stat", "--batch-samples", "5000", zst[0]) == gold("sp1_dna.stat.tsv")


def _records(path):
    """the on-disk records of a BLOW5 file"""
    buf = open(path, "rb").read()
    (hsize,) = struct.unpack_from("<I", buf, 64)
    pos, recs = 68 + hsize, []
    while buf[pos:pos + 5] != b"5WOLB" or pos + 5 != len(buf):
        (size,) = struct.unpack_from("<Q", buf, pos)
        recs.append(buf[pos + 8:pos + 8 + size])
        pos += 8 + size
    return recs


def test_zstd_job_equals_the_int16_job(gpu, sp1):
    """Job.stage_zrec(record_format=RECORD_ZSTD): the fixture's frames as they sit in the file; what a record holds is
    known from sp1_dna.blow5, whose inflated records are the same bytes"""
    frames = _records(os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5"))
    plain = [zlib.decompress(r) for r in _records(SP1)]
    pick = list(range(0, 100, 4))
    reads = [sp1.reads[i] for i in pick]
    sig_off, sig_len = [], []
    for i in pick:
        (idl,) = struct.unpack_from("<H", plain[i], 0)
        (ln,) = struct.unpack_from("<Q", plain[i], 2 + idl + 36)
        sig_off.append(2 + idl + 44); sig_len.append(ln)
    dig, off, rng = [r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads]
    job = gpu.Job(0)
    job.stage([r.raw for r in reads], dig, off, rng)
    job.launch(gpu.TOOL_STAT)
    want_stat = job.wait()["stat"].copy()
    job.launch(gpu.TOOL_PA)
    want_pa = [p.copy() for p in job.wait()["pa"]]
    job.stage_zrec([frames[i] for i in pick], [r.raw.size for r in reads], sig_off, sig_len, [len(plain[i]) for i in pick],
                   dig, off, rng, record_format=gpu.RECORD_ZSTD)
    job.launch(gpu.TOOL_STAT)
    assert job.wait()["stat"].tobytes() == want_stat.tobytes()
    job.launch(gpu.TOOL_PA)
    got_pa = job.wait()["pa"]
    assert all(np.array_equal(a, b) for a, b in zip(got_pa, want_pa))
    # a zlib record under the zstd format is refused with the zstd status, not decoded as something else
    job.stage_zrec([_records(SP1)[0]], [sp1.reads[0].raw.size], sig_off[:1], sig_len[:1], [len(plain[0])],
                   dig[:1], off[:1], rng[:1], record_format=gpu.RECORD_ZSTD)
    job.launch(gpu.TOOL_STAT)
    rc, ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT and ds[0] == 0x200 | zstd_craft.ST_HEADER


def test_qts_writes_zlib_records(cli, zst, tmp_path):
    """qts on zstd input decodes on the host and writes zlib records (header byte 9 = 1): the records a reader sees are
    those of qts on the zlib file"""
    a, b = str(tmp_path / "qa.blow5"), str(tmp_path / "qb.blow5")
    for src, dst in ((zst[0], a), (zst[1], b)):
        p = subprocess.run([cli, "qts", src, "-o", dst, "-b", "3"], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    ha, hb = open(a, "rb").read(16), open(b, "rb").read(16)
    assert ha[9] == 1 and ha[14] == 1 and ha == hb
    da = subprocess.run([cli, "_dump", a], capture_output=True)
    db = subprocess.run([cli, "_dump", b], capture_output=True)
    assert da.returncode == 0 and da.stdout == db.stdout and da.stdout.count(b"\n") == 101
    assert blow5.digest(a) == blow5.digest(b)


def test_a_corrupted_record_ends_the_run_like_a_read_error(cli, tmp_path):
    """A level 1 frame carries no checksum, so a flipped bit in the middle of one may leave a frame that every decoder
    (libzstd too) takes, with other bytes.  These two defects no decoder may take: the declared content size off by one
    (Frame_Content_Size is the two-byte form here, at byte 5 of the single-segment frame; the record's head still
    decodes, so on the default path it is the kernel that meets the defect), and a sequences bitstream without its end
    mark (the frame's last byte zero)."""
    src = open(os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5"), "rb").read()
    (hsize,) = struct.unpack_from("<I", src, 64)
    pos = 68 + hsize
    for _ in range(3):                           # the fourth record
        pos += 8 + struct.unpack_from("<Q", src, pos)[0]
    (size,) = struct.unpack_from("<Q", src, pos)
    frame = pos + 8
    assert src[frame:frame + 4] == zstd_craft.MAGIC and src[frame + 4] == 0x60 and src[frame + size - 1] != 0
    for name, at, value in (("size", frame + 5, src[frame + 5] ^ 1), ("endmark", frame + size - 1, 0)):
        data = bytearray(src)
        data[at] = value
        path = str(tmp_path / (name + ".blow5"))
        open(path, "wb").write(bytes(data))
        for extra in ([], ["--host-inflate"]):
            p = subprocess.run([cli, "stat", *extra, path], capture_output=True)
            assert p.returncode == 1 and b"Error in slow5_get_next" in p.stderr, (name, extra, p.returncode, p.stderr[-300:])
