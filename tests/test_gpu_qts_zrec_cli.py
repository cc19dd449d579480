"""GPU: `qts --gpu-inflate` -- the records go to the GPU as they sit in the file and come back as the new zlib streams --
against `qts --gpu-deflate` (the same streams, byte for byte: k_deflate is deterministic on equal input) and the
reference's digests; the batches it redoes on the host, the record that ends the run, the files it does not apply to."""
import json
import os
import re
import struct
import subprocess
import zlib

import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
SP1_ZSTD = os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5")
BATCH = ["--batch-samples", "150000"]     # the 100 fixture reads make several batches


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def run_timed(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True, env=dict(os.environ, SGK_CLI_TIMING="1"))
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def path_counts(stderr):
    m = re.search(r"records decompressed on the GPU: (\d+) of (\d+); batches redone on the host: (\d+)", stderr)
    assert m, stderr[-1500:]
    return tuple(int(x) for x in m.groups())


def qts(cli, flag, inp, outp, *more):
    rc, _, err = run_timed(cli, "qts", *flag, inp, "-o", outp, *BATCH, *more)
    assert rc == 0, err[-1500:]
    return open(outp, "rb").read(), path_counts(err)


@pytest.mark.parametrize("bits,method", [(1, "round"), (3, "round"), (2, "floor"), (4, "fill-ones")])
def test_gpu_inflate_writes_what_gpu_deflate_writes(cli, tmp_path, bits, method):
    a, b = str(tmp_path / "inflate.blow5"), str(tmp_path / "deflate.blow5")
    got, counts = qts(cli, ["--gpu-inflate"], SP1, a, "-b", str(bits), "-m", method)
    want, _ = qts(cli, ["--gpu-deflate"], SP1, b, "-b", str(bits), "-m", method)
    assert counts == (100, 100, 0)
    assert got == want
    assert blow5.digest(a) == MANIFEST["sp1_dna.qts_b%d_%s.sha256" % (bits, method)]


def test_gpu_inflate_zstd_input(cli, tmp_path):
    a, b = str(tmp_path / "inflate.blow5"), str(tmp_path / "deflate.blow5")
    got, counts = qts(cli, ["--gpu-inflate"], SP1_ZSTD, a, "-b", "1", "-m", "round")
    want, _ = qts(cli, ["--gpu-deflate"], SP1_ZSTD, b, "-b", "1", "-m", "round")
    assert counts == (100, 100, 0)
    assert got[9] == 1 and got == want
    assert blow5.digest(a) == MANIFEST["sp1_dna.qts_b1_round.sha256"]


def test_without_slack_the_batches_are_redone_on_the_host(cli, tmp_path):
    a, b = str(tmp_path / "inflate.blow5"), str(tmp_path / "deflate.blow5")
    got, (on_gpu, total, redone) = qts(cli, ["--gpu-inflate", "--aux-slack", "0"], SP1, a, "-b", "1")
    want, _ = qts(cli, ["--gpu-deflate"], SP1, b, "-b", "1")
    assert total == 100 and redone >= 1 and on_gpu < 100
    assert got == want


def test_the_one_batch_with_a_long_string_is_redone(cli, sp1, tmp_path):
    """the 12-read file of tests/test_gpu_zrec_aux.py: a 300-byte channel_number at read 7"""
    reads = sp1.reads[:12]
    with_aux = [blow5.Read(r.read_id, r.read_group, r.digitisation, r.offset, r.range, r.sampling_rate, r.raw,
                           aux=(b"x" * 300 if i == 7 else b"%d" % (100 + i), 7 + i)) for i, r in enumerate(reads)]
    path = str(tmp_path / "long.blow5")
    blow5.write_blow5(path, with_aux, {a: sp1.attr(a) for a in sp1.attrs}, aux_types=[("channel_number", "char*"), ("start_time", "uint64_t")])
    a, b = str(tmp_path / "inflate.blow5"), str(tmp_path / "deflate.blow5")
    got, counts = qts(cli, ["--gpu-inflate"], path, a, "-b", "1")
    want, _ = qts(cli, ["--gpu-deflate"], path, b, "-b", "1")
    assert counts == (0, 12, 1)
    assert got == want


def test_a_record_that_does_not_fill_its_fields_ends_the_run(cli, tmp_path):
    """sp1_dna.blow5 with its fourth record re-deflated one tail byte short (the u64 size in front fixed up)"""
    src = open(SP1, "rb").read()
    (hsize,) = struct.unpack_from("<I", src, 64)
    pos = 68 + hsize
    for _ in range(3):
        pos += 8 + struct.unpack_from("<Q", src, pos)[0]
    (size,) = struct.unpack_from("<Q", src, pos)
    rec = zlib.compress(zlib.decompress(src[pos + 8:pos + 8 + size])[:-1])
    path = str(tmp_path / "cut.blow5")
    open(path, "wb").write(src[:pos] + struct.pack("<Q", len(rec)) + rec + src[pos + 8 + size:])
    rc, _, err = run_timed(cli, "qts", "--gpu-inflate", path, "-o", str(tmp_path / "o.blow5"), *BATCH)
    assert rc == 1 and "Error in slow5_get_next" in err, (rc, err[-500:])


@pytest.mark.parametrize("record_press,signal_press", [(1, 0), (0, 1)])
def test_files_the_path_does_not_apply_to(cli, sp1, tmp_path, record_press, signal_press):
    recs = sp1.reads[:7]
    inp, a, b = str(tmp_path / "i.blow5"), str(tmp_path / "inflate.blow5"), str(tmp_path / "deflate.blow5")
    blow5.write_blow5(inp, recs, {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"}, record_press, signal_press)
    got, counts = qts(cli, ["--gpu-inflate"], inp, a, "-b", "2")
    want, _ = qts(cli, ["--gpu-deflate"], inp, b, "-b", "2")
    assert counts == (0, 7, 0)
    assert got == want


def test_the_output_reads_back_like_the_host_paths(cli, tmp_path):
    a, b = str(tmp_path / "inflate.blow5"), str(tmp_path / "host.blow5")
    qts(cli, ["--gpu-inflate"], SP1, a, "-b", "1")
    qts(cli, [], SP1, b, "-b", "1")
    sa, sb = (subprocess.run([cli, "stat", p], capture_output=True) for p in (a, b))
    assert sa.returncode == 0 and sb.returncode == 0
    assert sa.stdout == sb.stdout and sa.stdout.count(b"\n") == 101


def test_help_does_not_mention_the_option(cli):
    p = subprocess.run([cli, "qts", "-h"], capture_output=True)
    assert p.returncode == 0 and b"gpu-inflate" not in p.stdout and b"Usage: sigtk qts a.blow5 -o out.blow5" in p.stdout
