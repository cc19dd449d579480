"""GPU: BLOW5 records compressed around an UNCOMPRESSED signal (signal_press 0) on the record path -- jobs staged with
sgk_job_begin_zrec_signal(SGK_SIGNAL_INT16) from zlib records (deflated here) and from the zstd fixture
(tests/golden/sp1_24.zstd_raw.blow5), and the CLI on such files: all records decompressed on the GPU, the output
byte-identical to --host-inflate and to the reference's goldens."""
import hashlib
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
FIXTURE = os.path.join(GOLDEN, "sp1_24.zstd_raw.blow5")
META = json.load(open(os.path.join(GOLDEN, "zrec_raw.json")))
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
ATTRS = {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"}
TABLE = [(8, 0), (4, 0), (1, 0), (8, 0), (1, 0), (1, 1)]      # sp1_dna.blow5's auxiliary columns (test_gpu_zrec_aux.py)
SLACK = 256
N = 24


# ---------------------------------------------------------------------------------------------- jobs

def file_records(path):
    """the on-disk records of a BLOW5 file"""
    buf = open(path, "rb").read()
    (hsize,) = struct.unpack_from("<I", buf, 64)
    pos, recs = 68 + hsize, []
    while buf[pos:pos + 5] != b"5WOLB" or pos + 5 != len(buf):
        (size,) = struct.unpack_from("<Q", buf, pos)
        recs.append(buf[pos + 8:pos + 8 + size])
        pos += 8 + size
    return recs


def plain_signal_record(rec):
    """an inflated record with an svb-zd signal -> the same record with plain samples, and where they lie"""
    (idl,) = struct.unpack_from("<H", rec, 0)
    p = 2 + idl + 36
    (ln,) = struct.unpack_from("<Q", rec, p)
    raw = blow5.svb_zd_decode(rec[p + 8:p + 8 + ln])
    return rec[:p] + struct.pack("<Q", raw.size) + raw.astype("<i2").tobytes() + rec[p + 8 + ln:], p + 8, raw.size


def zlib_room(sig_end, table, slack=SLACK):
    return sig_end + sum(eb for eb, a in table if not a) + sum(8 + slack for eb, a in table if a)


def zstd_content_size(frame):
    """Frame_Content_Size of a zstd frame header (RFC 8878 3.1.1.1)"""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    d = frame[4]
    single, fcs_flag, dict_flag = (d >> 5) & 1, d >> 6, d & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag]
    n = (1 if single else 0, 2, 4, 8)[fcs_flag]
    assert n
    return int.from_bytes(frame[pos:pos + n], "little") + (256 if n == 2 else 0)


@pytest.fixture(scope="module")
def raw_job(gpu, sp1):
    """the first 24 records of sp1_dna.blow5 with plain samples, and what an int16 job gives for them, computed once"""
    reads = sp1.reads[:N]
    made = [plain_signal_record(r) for r in blow5.raw_records(SP1)[:N]]
    plain = [m[0] for m in made]
    assert [(len(p), zlib.crc32(p)) for p in plain] == [(m["length"], m["crc32"]) for m in META["records"]]
    assert [m[2] for m in made] == [r.raw.size for r in reads]
    scal = ([r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads])
    job = gpu.Job(0)
    job.stage([r.raw for r in reads], *scal)
    want = {}
    job.launch(gpu.TOOL_STAT)
    want["stat"] = job.wait()["stat"].tobytes()
    job.launch(gpu.TOOL_PA)
    want["pa"] = [p.copy() for p in job.wait()["pa"]]
    job.launch(gpu.TOOL_EVENT)
    want["events"] = [(e.start.copy(), e.length.copy(), e.mean.copy(), e.stdv.copy()) for e in job.wait()["events"]]
    job.launch_qts(3, 1, True)
    want["qts"] = [bytes(b) for b in job.wait()["blobs"]]
    job.close()
    sig_off = [m[1] for m in made]
    lengths = [m[2] for m in made]
    return {"reads": reads, "plain": plain, "scal": scal, "want": want, "lengths": lengths, "sig_off": sig_off,
            "sig_bytes": [2 * n for n in lengths], "room": [zlib_room(o + 2 * n, TABLE) for o, n in zip(sig_off, lengths)]}


def check_results(gpu, job, want):
    job.launch(gpu.TOOL_STAT)
    assert job.wait()["stat"].tobytes() == want["stat"]
    job.launch(gpu.TOOL_PA)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(job.wait()["pa"], want["pa"]))
    job.launch(gpu.TOOL_EVENT)
    got = job.wait()["events"]
    assert len(got) == len(want["events"])
    for e, (s, l, m, d) in zip(got, want["events"]):
        assert np.array_equal(e.start, s) and np.array_equal(e.length, l)
        assert np.array_equal(e.mean.view(np.uint32), m.view(np.uint32)) and np.array_equal(e.stdv.view(np.uint32), d.view(np.uint32))


def stage(gpu, job, j, recs, room=None, aux=TABLE, **kw):
    job.stage_zrec(recs, j["lengths"], j["sig_off"], kw.pop("sig_bytes", j["sig_bytes"]), j["room"] if room is None else room,
                   *j["scal"], aux=aux, signal_format=gpu.SIGNAL_INT16, **kw)


def statuses(gpu, job):
    job.launch(gpu.TOOL_STAT)
    rc, ds = job.wait_rc()
    return rc, [int(x) for x in ds]


def test_zlib_records_with_plain_samples(gpu, raw_job):
    j = raw_job
    assert {(o % 16) for o in j["sig_off"]} != {0} and all(len(p) < r for p, r in zip(j["plain"], j["room"]))
    job = gpu.Job(0)
    stage(gpu, job, j, [zlib.compress(p) for p in j["plain"]])
    check_results(gpu, job, j["want"])
    # qts on such a batch works as on any staged one; the frames of the records inflated on the GPU are not for it
    job.launch_qts(3, 1, True)
    assert [bytes(b) for b in job.wait()["blobs"]] == j["want"]["qts"]
    with pytest.raises(gpu.SigtkGpuError):
        job.launch_qts(3, 1, True, records=True, zrec_frames=True)
    check_results(gpu, job, j["want"])
    job.close()


def test_zstd_records_with_plain_samples(gpu, raw_job):
    j = raw_job
    frames = file_records(FIXTURE)
    room = [zstd_content_size(f) for f in frames]
    assert len(frames) == N and room == [len(p) for p in j["plain"]]
    job = gpu.Job(0)
    stage(gpu, job, j, frames, room=room, record_format=gpu.RECORD_ZSTD)
    check_results(gpu, job, j["want"])
    job.close()


def test_begin_checks_the_signal_format_and_the_signal_bytes(gpu, raw_job):
    import ctypes as C
    j = raw_job
    recs = [zlib.compress(p) for p in j["plain"]]
    job = gpu.Job(0)
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
    lengths, rbytes, so, room = u32(j["lengths"]), u32([len(r) for r in recs]), u32(j["sig_off"]), u32(j["room"])
    jin = gpu.JobInput()

    def begin(signal_format, sig_bytes):
        sb = u32(sig_bytes)
        return job.L.sgk_job_begin_zrec_signal(job.h, N, gpu.RECORD_ZLIB, signal_format, lengths.ctypes.data, rbytes.ctypes.data,
                                               so.ctypes.data, sb.ctypes.data, room.ctypes.data, gpu.aux_table(TABLE), len(TABLE),
                                               C.byref(jin))
    for r, delta in ((0, 1), (7, -1), (23, 2), (11, -2)):
        sb = list(j["sig_bytes"])
        sb[r] += delta
        assert begin(gpu.SIGNAL_INT16, sb) == gpu.SGK_ERR_ARG
    for fmt in (2, 3, 9):
        assert begin(fmt, j["sig_bytes"]) == gpu.SGK_ERR_ARG
    assert begin(gpu.SIGNAL_INT16, j["sig_bytes"]) == gpu.SGK_OK
    # the job is as usable as before
    stage(gpu, job, j, recs)
    check_results(gpu, job, j["want"])
    job.close()


def test_short_cut_and_corrupt_records_get_their_own_status(gpu, raw_job):
    j = raw_job
    good = [zlib.compress(p) for p in j["plain"]]
    job = gpu.Job(0)
    # record 5 re-deflated one tail byte short: it inflates, its fields do not fill it
    recs = list(good)
    recs[5] = zlib.compress(j["plain"][5][:-1])
    stage(gpu, job, j, recs)
    assert statuses(gpu, job) == (gpu.SGK_ERR_FORMAT, [0x400 | 2 if r == 5 else 0 for r in range(N)])
    # record 9 cut inside its signal (at an odd byte), record 14 in front of it
    recs = list(good)
    recs[9] = zlib.compress(j["plain"][9][:j["sig_off"][9] + 1001])
    recs[14] = zlib.compress(j["plain"][14][:j["sig_off"][14] - 3])
    stage(gpu, job, j, recs)
    assert statuses(gpu, job) == (gpu.SGK_ERR_FORMAT, [0x400 | 1 if r in (9, 14) else 0 for r in range(N)])
    # a stream whose check value is wrong, and one cut short: the inflate status comes first
    recs = list(good)
    recs[3] = good[3][:-1] + bytes([good[3][-1] ^ 0x40])
    recs[20] = good[20][:len(good[20]) // 2]
    stage(gpu, job, j, recs)
    rc, ds = statuses(gpu, job)
    assert rc == gpu.SGK_ERR_FORMAT and ds[3] == 0x107 and ds[20] >> 8 == 1 and 1 <= (ds[20] & 0xff) <= 8
    assert [d for r, d in enumerate(ds) if r not in (3, 20)] == [0] * (N - 2)
    # the same job, the sound records again: nothing of the batches before is left in anybody's samples
    stage(gpu, job, j, good)
    check_results(gpu, job, j["want"])
    job.close()


def test_records_without_columns_end_exactly_at_their_signal(gpu, raw_job):
    j = raw_job
    bare = [p[:o + 2 * n] for p, o, n in zip(j["plain"], j["sig_off"], j["lengths"])]
    room = [len(b) for b in bare]
    job = gpu.Job(0)
    stage(gpu, job, j, [zlib.compress(b) for b in bare], room=room, aux=[])
    check_results(gpu, job, j["want"])
    stage(gpu, job, j, [zlib.compress(b) for b in bare], room=room, aux=None)       # (no table given counts as none)
    check_results(gpu, job, j["want"])
    recs = [zlib.compress(b + (b"\x00" if r == 2 else b"")) for r, b in enumerate(bare)]
    stage(gpu, job, j, recs, room=[x + 8 for x in room], aux=[])
    assert statuses(gpu, job) == (gpu.SGK_ERR_FORMAT, [0x400 | 3 if r == 2 else 0 for r in range(N)])
    recs = [zlib.compress(b[:-1] if r == 2 else b) for r, b in enumerate(bare)]
    stage(gpu, job, j, recs, room=room, aux=[])
    assert statuses(gpu, job) == (gpu.SGK_ERR_FORMAT, [0x400 | 1 if r == 2 else 0 for r in range(N)])
    job.close()


# ---------------------------------------------------------------------------------------------- CLI

AUX_TYPES = [("channel_number", "char*"), ("start_time", "uint64_t")]


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def with_aux(reads, long_at=None):
    return [blow5.Read(r.read_id, r.read_group, r.digitisation, r.offset, r.range, r.sampling_rate, r.raw,
                       aux=(b"x" * 300 if i == long_at else b"%d" % (100 + i), 7 + i)) for i, r in enumerate(reads)]


@pytest.fixture(scope="module")
def zlib_none(sp1, tmp_path_factory):
    """the 100 reads of sp1_dna.blow5, zlib records around plain samples, a string and an integer column behind them"""
    path = str(tmp_path_factory.mktemp("zrec_raw") / "sp1.zlib_none.blow5")
    blow5.write_blow5(path, with_aux(sp1.reads), ATTRS, 1, 0, aux_types=AUX_TYPES)
    return path


def run_timed(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True, env=dict(os.environ, SGK_CLI_TIMING="1"))
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def path_counts(stderr):
    m = re.search(r"records decompressed on the GPU: (\d+) of (\d+); batches redone on the host: (\d+)", stderr)
    assert m, stderr[-1500:]
    return tuple(int(x) for x in m.groups())


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


TOOLS = [(["stat"], "sp1_dna.stat.tsv"), (["event", "-c"], "sp1_dna.event_c.tsv"), (["pa"], None), (["jnn"], "sp1_dna.jnn.tsv"),
         (["prefix", "--print-stat"], "sp1_dna.prefix_stat.tsv"), (["ent"], "sp1_dna.ent.tsv")]
TOOL_IDS = ["stat", "event_c", "pa", "jnn", "prefix_stat", "ent"]


@pytest.mark.parametrize("tool,golden", TOOLS, ids=TOOL_IDS)
def test_cli_on_zlib_records_with_plain_samples(cli, zlib_none, tool, golden):
    rc, want, err = run_timed(cli, *tool, "--host-inflate", zlib_none)
    assert rc == 0 and path_counts(err) == (0, 100, 0), err[-1500:]
    rc, out, err = run_timed(cli, *tool, zlib_none)
    assert rc == 0, err[-1500:]
    assert out == want
    assert "records decompressed on the GPU: 100 of 100; batches redone on the host: 0" in err
    if golden:
        assert out == gold(golden)
    else:
        assert hashlib.sha256(out).hexdigest() == MANIFEST["sp1_dna.pa.tsv.sha256"]


@pytest.mark.parametrize("tool,golden", TOOLS, ids=TOOL_IDS)
def test_cli_on_the_zstd_fixture(cli, tool, golden):
    rc, want, err = run_timed(cli, *tool, "--host-inflate", FIXTURE)
    assert rc == 0 and path_counts(err) == (0, N, 0), err[-1500:]
    rc, out, err = run_timed(cli, *tool, FIXTURE)
    assert rc == 0, err[-1500:]
    assert out == want and out.count(b"\n") > N
    assert "records decompressed on the GPU: %d of %d; batches redone on the host: 0" % (N, N) in err
    if tool == ["stat"]:      # one row per read under one header line: the head of the 100-read golden
        assert out == b"".join(gold(golden).splitlines(True)[:N + 1])


def test_cli_host_decode_keeps_such_a_file_on_the_host(cli, zlib_none):
    rc, out, err = run_timed(cli, "stat", "--host-decode", zlib_none)
    assert rc == 0 and out == gold("sp1_dna.stat.tsv") and path_counts(err) == (0, 100, 0)


@pytest.mark.parametrize("path_of", ["zlib", "zstd"])
def test_cli_rows_written_on_the_gpu(cli, zlib_none, path_of):
    path = zlib_none if path_of == "zlib" else FIXTURE
    n = 100 if path_of == "zlib" else N
    for tool in (["event"], ["event", "-c"], ["pa"]):
        rc, want, err = run_timed(cli, *tool, "--host-inflate", path)
        assert rc == 0, err[-1500:]
        rc, out, err = run_timed(cli, *tool, "--gpu-text", path)
        assert rc == 0, err[-1500:]
        assert out == want and path_counts(err) == (n, n, 0)
    if path_of == "zlib":
        assert want and hashlib.sha256(want).hexdigest() == MANIFEST["sp1_dna.pa.tsv.sha256"]


def test_cli_without_slack_redoes_its_batches_on_the_host(cli, zlib_none):
    rc, out, err = run_timed(cli, "stat", "--aux-slack", "0", "--batch-samples", "150000", zlib_none)
    assert rc == 0, err[-1500:]
    assert out == gold("sp1_dna.stat.tsv")
    on_gpu, total, redone = path_counts(err)
    assert total == 100 and redone >= 1 and on_gpu < 100
    rc, out, err = run_timed(cli, "event", "-c", "--gpu-text", "--aux-slack", "0", "--batch-samples", "150000", zlib_none)
    assert rc == 0 and out == gold("sp1_dna.event_c.tsv") and path_counts(err)[2] >= 1


def test_cli_redoes_the_one_batch_with_a_long_string(cli, sp1, tmp_path):
    path = str(tmp_path / "long.blow5")
    blow5.write_blow5(path, with_aux(sp1.reads[:12], long_at=7), ATTRS, 1, 0, aux_types=AUX_TYPES)
    rc, want, err = run_timed(cli, "stat", "--host-inflate", path)
    assert rc == 0 and want.count(b"\n") == 13 and path_counts(err) == (0, 12, 0)
    assert want == b"".join(gold("sp1_dna.stat.tsv").splitlines(True)[:13])
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 0, err[-1500:]
    assert out == want and path_counts(err) == (0, 12, 1)
    blow5.write_blow5(path, with_aux(sp1.reads[:12]), ATTRS, 1, 0, aux_types=AUX_TYPES)
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 0 and out == want and path_counts(err) == (12, 12, 0)


def test_cli_a_record_cut_one_byte_short_ends_the_run(cli, zlib_none, tmp_path):
    """the fourth record re-deflated without its last byte (the u64 size in front fixed up)"""
    src = open(zlib_none, "rb").read()
    (hsize,) = struct.unpack_from("<I", src, 64)
    pos = 68 + hsize
    for _ in range(3):
        pos += 8 + struct.unpack_from("<Q", src, pos)[0]
    (size,) = struct.unpack_from("<Q", src, pos)
    rec = zlib.compress(zlib.decompress(src[pos + 8:pos + 8 + size])[:-1])
    path = str(tmp_path / "cut.blow5")
    open(path, "wb").write(src[:pos] + struct.pack("<Q", len(rec)) + rec + src[pos + 8 + size:])
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 1 and "Error in slow5_get_next" in err, (rc, err[-500:])
