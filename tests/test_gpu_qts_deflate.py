"""GPU: `qts --gpu-deflate` -- the rewritten records assembled (k_qts_assemble) and deflated (k_deflate) on the GPU --
through the job (sgk_job_set_record_frames + SGK_QTS_RECORDS), and through the CLI against the reference's digests."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
SP1_ZSTD = os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5")


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def run(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def frames_for(n):
    rs = np.random.RandomState(77)
    heads = [rs.bytes(50) for _ in range(n)]
    tails = [rs.bytes((0, 1, 37)[r % 3]) for r in range(n)]
    return heads, tails


@pytest.mark.parametrize("svb_out", [True, False])
def test_job_records_are_the_host_records(gpu, svb_out):
    """zlib.decompress(record r) == head | u64 len_raw_signal | signal | tail, the signal as launch_qts hands it back
    without the flag"""
    lens = [0, 1, 5, 4096, 30001, 100000]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=41, kind=0)
    heads, tails = frames_for(len(lens))
    job = gpu.Job(0)
    try:
        blobs = [blow5.svb_zd_encode(r) for r in reads]
        job.stage(blobs, dig, off, rng, counts=[r.size for r in reads])
        job.launch_qts(3, 1, svb_out)
        plain = job.wait()
        job.set_record_frames([h + t for h, t in zip(heads, tails)], [len(h) for h in heads])
        job.launch_qts(3, 1, svb_out, records=True)
        res = job.wait()
        assert "blobs" not in res and "samples" not in res
        assert [int(s) for s in res["record_status"]] == [0] * len(lens)
        for r in range(len(lens)):
            if svb_out:
                sig, ln = plain["blobs"][r], len(plain["blobs"][r])
            else:
                sig, ln = plain["samples"][r].astype("<i2").tobytes(), lens[r]
            assert zlib.decompress(res["records"][r]) == heads[r] + struct.pack("<Q", ln) + sig + tails[r], r
        # without frames (a new batch forgets them), and for text input, the submit is refused
        job.stage(blobs, dig, off, rng, counts=[r.size for r in reads])
        with pytest.raises(gpu.SigtkGpuError):
            job.launch_qts(3, 1, svb_out, records=True)
    finally:
        job.close()


@pytest.mark.parametrize("svb_out", [True, False])
def test_job_records_at_every_head_and_source_alignment(gpu, svb_out):
    """k_qts_assemble copies a signal of 64 bytes or more as dwords when (source address + lead) % 4 == 0, where lead =
    (4 - head % 4) % 4 because records start on 16-byte boundaries; otherwise, and below 64 bytes, byte by byte.  The job's
    sources are aligned whatever the reads are: int16 samples start on 128-byte boundaries, svb-zd blobs on 8-byte ones.  So
    the condition is lead == 0: the dword branch is taken exactly by the reads with sbytes >= 64 and head % 4 == 0, and its
    lead > 0 form cannot be reached through the job.  The head lengths 40 .. 47 cycle over the reads, which puts every
    fourth read (heads 40 and 44) on the dword branch and the others, at leads 3, 2 and 1, on the byte loop.  The signals
    are 24 .. 60 samples, twice over and two more (int16: 48 .. 120 bytes, on both sides of the 64; svb-zd blobs of such
    reads likewise), then large reads: 30001, 4096 and 4097 samples under heads 44, 40 and 44, whose copies are several
    rounds of the 256-dword stride with (30001, 4097 as int16; whatever the blobs give) a byte tail behind them, and the
    same lengths under the heads between for the byte loop.  The test works out which reads take the dword branch and
    asserts that the cases named here are among them.  Every record must inflate to head | u64 | signal | tail: a dword
    copy from a wrong place, of a wrong count or with a wrong stride shows as other bytes."""
    lens = list(range(24, 61)) * 2 + [33, 35]
    assert len(lens) % 8 == 4
    lens += [30001, 4096, 30001, 4097, 4096, 30001, 4096, 30001, 4097]     # heads 44, 45, 46, 47, 40, 41, 42, 43, 44
    big = {len(lens) - 9: 30001, len(lens) - 5: 4096, len(lens) - 1: 4097}
    n = len(lens)
    reads, dig, off, rng = gpu.synth_reads_host(n, lens, seed=43, kind=0)
    rs = np.random.RandomState(78)
    heads = [rs.bytes(40 + r % 8) for r in range(n)]
    tails = [rs.bytes((0, 1, 37)[r % 3]) for r in range(n)]
    job = gpu.Job(0)
    try:
        blobs = [blow5.svb_zd_encode(r) for r in reads]
        job.stage(blobs, dig, off, rng, counts=[r.size for r in reads])
        job.launch_qts(3, 1, svb_out)
        plain = job.wait()
        job.set_record_frames([h + t for h, t in zip(heads, tails)], [len(h) for h in heads])
        job.launch_qts(3, 1, svb_out, records=True)
        res = job.wait()
        assert [int(s) for s in res["record_status"]] == [0] * n
        sbytes = []
        for r in range(n):
            if svb_out:
                sig, ln = plain["blobs"][r], len(plain["blobs"][r])
            else:
                sig, ln = plain["samples"][r].astype("<i2").tobytes(), lens[r]
            sbytes.append(len(sig))
            assert zlib.decompress(res["records"][r]) == heads[r] + struct.pack("<Q", ln) + sig + tails[r], (r, lens[r])
        # which reads took which path (the docstring's rule), and that every case it names is there
        dword = [r for r in range(n) if sbytes[r] >= 64 and len(heads[r]) % 4 == 0]
        loop = [r for r in range(n) if r not in dword]
        assert all(lens[r] == v and r in dword for r, v in big.items()), dword
        assert {len(heads[r]) for r in dword} == {40, 44} and {len(heads[r]) % 4 for r in loop} == {0, 1, 2, 3}
        small = sorted(sbytes[r] for r in dword if sbytes[r] <= 70)
        assert len(small) >= 2 and any(v % 4 for v in small), small                       # 64 .. 70 bytes, one with a tail
        assert any(60 <= sbytes[r] < 64 for r in loop) and any(sbytes[r] < 64 and len(heads[r]) % 4 == 0 for r in loop)
        strides = [r for r in dword if sbytes[r] // 4 > 512]
        assert any(sbytes[r] % 4 for r in strides) and any(sbytes[r] // 4 % 256 for r in strides), [sbytes[r] for r in strides]
        assert all(any(sbytes[r] > 4096 and len(heads[r]) % 4 == k for r in loop) for k in (1, 2, 3))
        print("dword copies: %d reads of %s bytes; byte loops: %d reads" % (len(dword), [sbytes[r] for r in dword], len(loop)))
    finally:
        job.close()


def test_fixture_records_are_no_longer_than_huffman_only(gpu, sp1):
    """-b 1 -m round over the 100 fixture reads: the GPU's records, summed, against zlib's Z_HUFFMAN_ONLY of the same
    records (Z_RLE is 8 % under that line: a run-plus-Huffman coder has room, a literal-only one fails)"""
    reads = sp1.reads
    recs = blow5.raw_records(SP1)
    heads, tails = [], []
    for rec in recs:
        (idl,) = struct.unpack_from("<H", rec, 0)
        sig = 2 + idl + 36
        (ln,) = struct.unpack_from("<Q", rec, sig)
        heads.append(rec[:sig]); tails.append(rec[sig + 8 + ln:])
    job = gpu.Job(0)
    try:
        job.stage([r.raw for r in reads], [r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads])
        job.set_record_frames([h + t for h, t in zip(heads, tails)], [len(h) for h in heads])
        job.launch_qts(1, 1, True, records=True)
        res = job.wait()
    finally:
        job.close()
    ours = theirs = 0
    for r, z in enumerate(res["records"]):
        plain = zlib.decompress(z)
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        theirs += len(c.compress(plain) + c.flush())
        ours += len(z)
        x = reads[r].raw.astype(np.int64)
        e = np.where((x & 1) < 1, x & ~1, (x & ~1) + 2).astype(np.int16)
        blob = blow5.svb_zd_encode(e)
        assert plain == heads[r] + struct.pack("<Q", len(blob)) + blob + tails[r], r
    print("GPU records %d bytes, Z_HUFFMAN_ONLY %d bytes" % (ours, theirs))
    assert ours <= theirs, (ours, theirs)


def check_records(inp, outp, header_byte9=None):
    src, dst = open(inp, "rb").read(), open(outp, "rb").read()
    (hsize,) = struct.unpack_from("<I", src, 64)
    want_hdr = bytearray(src[: 68 + hsize])
    if header_byte9 is not None:
        want_hdr[9] = header_byte9
    assert dst[: 68 + hsize] == bytes(want_hdr) and dst[-5:] == b"5WOLB"
    ra, rb = blow5.raw_records(inp) if src[9] != 2 else None, blow5.raw_records(outp)
    if ra is None:   # (zstd records: the same reads sit in the zlib fixture)
        ra = blow5.raw_records(SP1)
    assert len(ra) == len(rb) > 0
    for a, b in zip(ra, rb):
        (idl,) = struct.unpack_from("<H", a, 0)
        sig = 2 + idl + 36          # offset of len_raw_signal
        (la,) = struct.unpack_from("<Q", a, sig)
        (lb,) = struct.unpack_from("<Q", b, sig)
        la, lb = (la, lb) if src[14] == 1 else (2 * la, 2 * lb)
        assert a[:sig] == b[:sig]                                   # id, read group, scaling, sampling rate
        assert a[sig + 8 + la:] == b[sig + 8 + lb:]                 # auxiliary fields


@pytest.mark.parametrize("bits,method", [(1, "round"), (3, "round"), (2, "floor"), (4, "fill-ones")])
def test_cli_gpu_deflate_has_the_references_digest(cli, tmp_path, bits, method):
    outp = str(tmp_path / "q.blow5")
    run(cli, "qts", "--gpu-deflate", SP1, "-o", outp, "-b", str(bits), "-m", method, "--batch-samples", "150000")
    assert blow5.digest(outp) == MANIFEST["sp1_dna.qts_b%d_%s.sha256" % (bits, method)]
    check_records(SP1, outp)
    assert len(blow5.raw_records(SP1)[0]) > 2 + 36 + 36 + 8   # (the fixture's records do carry auxiliary fields)


def test_cli_gpu_deflate_zstd_input(cli, tmp_path):
    outp = str(tmp_path / "q.blow5")
    run(cli, "qts", "--gpu-deflate", SP1_ZSTD, "-o", outp, "-b", "1", "-m", "round", "--batch-samples", "150000")
    assert open(outp, "rb").read()[9] == 1
    assert blow5.digest(outp) == MANIFEST["sp1_dna.qts_b1_round.sha256"]
    check_records(SP1_ZSTD, outp, header_byte9=1)


def test_cli_gpu_deflate_int16_signal_and_uncompressed_records(cli, tmp_path, sp1):
    recs = sp1.reads[:7]
    attrs = {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"}
    for rp, sp in ((1, 0), (0, 1)):     # (0, 1): nothing to deflate, the flag is accepted and changes nothing
        inp, outp, ref = str(tmp_path / "i.blow5"), str(tmp_path / "o.blow5"), str(tmp_path / "r.blow5")
        blow5.write_blow5(inp, recs, attrs, rp, sp)
        run(cli, "qts", "--gpu-deflate", inp, "-o", outp, "-b", "2")
        got = blow5.read_blow5(outp)
        assert (got.record_press, got.signal_press) == (rp, sp)
        for g, r in zip(got.reads, recs):
            x = r.raw.astype(np.int64)
            e = np.where((x & 3) < 2, x & ~3, (x & ~3) + 4).astype(np.int16)
            assert g.read_id == r.read_id and np.array_equal(g.raw, e)
        check_records(inp, outp)
        if rp == 0:
            run(cli, "qts", inp, "-o", ref, "-b", "2")
            assert open(outp, "rb").read() == open(ref, "rb").read()


@pytest.fixture(scope="module")
def both_outputs(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("qtsdef")
    host, dev = str(d / "host.blow5"), str(d / "gpu.blow5")
    run(cli, "qts", SP1, "-o", host, "-b", "1", "--batch-samples", "150000")
    run(cli, "qts", "--gpu-deflate", SP1, "-o", dev, "-b", "1", "--batch-samples", "150000")
    return host, dev


@pytest.mark.parametrize("extra", [[], ["--host-inflate"]])
def test_the_output_reads_back_through_both_inflate_paths(cli, both_outputs, extra):
    host, dev = both_outputs
    assert open(host, "rb").read() != open(dev, "rb").read()     # other streams ...
    a, b = run(cli, "stat", *extra, host), run(cli, "stat", *extra, dev)
    assert a == b and a.count(b"\n") == 101                      # ... the same reads


def test_help_is_the_references(cli):
    p = subprocess.run([cli, "qts", "-h"], capture_output=True)
    assert p.returncode == 0 and b"gpu-deflate" not in p.stdout and b"Usage: sigtk qts a.blow5 -o out.blow5" in p.stdout
