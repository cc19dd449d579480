"""GPU: qts record mode with SGK_QTS_ZREC_FRAMES -- head and tail of every rewritten record are read where the record
was inflated on the GPU (k_qts_zrec_sizes, k_qts_assemble with two sources), no frames are staged.  Hand-made records over
every head residue, both sides of the assemble kernel's 64-byte threshold and every tail shape; the staged-frames path of
the same batch is the oracle for the streams (k_deflate is deterministic on equal input)."""
import os
import struct
import zlib

import numpy as np
import pytest

from sigtk_amd import blow5

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
SP1_ZSTD = os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5")
SLACK = 256                       # room per array column of a zlib record behind its count word (the CLI's default)
ID_LENS = (0, 1, 2, 3, 36)        # head = 2 + id + 36 bytes: every residue mod 4
LENS = [0, 1, 5] + list(range(24, 61)) + [4096, 4097, 30001, 100000]
STORED = LENS.index(4097)         # the one record compressed at level 0 (stored blocks)
BITS, METHOD = 3, 1               # -b 3 -m round

TABLES = {
    "none": [],
    "fixed": [(8, 0), (4, 0), (1, 0), (2, 0)],
    "array": [(8, 0), (1, 1), (4, 0)],
}
ARRAY_BYTES = (0, 1, 37, SLACK)   # the array's lengths, cycling over the reads


def make_tail(table, k, rs):
    out = b""
    for eb, is_array in table:
        if is_array:
            n = ARRAY_BYTES[k % len(ARRAY_BYTES)]
            out += struct.pack("<Q", n) + rs.bytes(n * eb)
        else:
            out += rs.bytes(eb)
    return out


def make_head(k, rs):
    rid = rs.bytes(ID_LENS[k % len(ID_LENS)])
    return struct.pack("<H", len(rid)) + rid + struct.pack("<Idddd", 0, 8192.0, 3.0 + k, 1400.0, 4000.0)


def zlib_room(sig_end, table, slack=SLACK):
    return sig_end + sum(eb for eb, a in table if not a) + sum(8 + slack for eb, a in table if a)


def quantise_round(x, bits):
    x = x.astype(np.int64)
    m = (1 << bits) - 1
    return np.where((x & m) < (1 << (bits - 1)), x & ~m, (x & ~m) + (1 << bits)).astype(np.int16)


class Batch:
    """hand-made records of one column table: plain = head | u64 blob length | svb-zd blob | tail"""

    def __init__(self, gpu, lens, table, seed):
        rs = np.random.RandomState(seed)
        self.n = len(lens)
        self.lens = list(lens)
        self.table = table
        self.reads, self.dig, self.off, self.rng = gpu.synth_reads_host(self.n, self.lens, seed=seed, kind=0)
        self.blobs = [blow5.svb_zd_encode(r) for r in self.reads]
        self.heads = [make_head(k, rs) for k in range(self.n)]
        self.tails = [make_tail(table, k, rs) for k in range(self.n)]
        self.plain = [h + struct.pack("<Q", len(b)) + b + t for h, b, t in zip(self.heads, self.blobs, self.tails)]
        self.sig_off = [len(h) + 8 for h in self.heads]
        self.sig_len = [len(b) for b in self.blobs]
        self.room = [zlib_room(o + n, table) for o, n in zip(self.sig_off, self.sig_len)]
        self.scal = (self.dig, self.off, self.rng)

    def compressed(self, stored=None):
        return [zlib.compress(p, 0 if k == stored else 6) for k, p in enumerate(self.plain)]

    def stage(self, job, records=None, room=None):
        job.stage_zrec(records if records is not None else self.compressed(), self.lens, self.sig_off, self.sig_len,
                       room if room is not None else self.room, *self.scal, aux=self.table)

    def oracle(self, gpu, job):
        """the same reads staged as blobs: the new blobs, and the records of the staged-frames path"""
        job.stage(self.blobs, *self.scal, counts=self.lens)
        job.launch_qts(BITS, METHOD, True)
        new_blobs = job.wait()["blobs"]
        job.set_record_frames([h + t for h, t in zip(self.heads, self.tails)], [len(h) for h in self.heads])
        job.launch_qts(BITS, METHOD, True, records=True)
        res = job.wait()
        assert [int(s) for s in res["record_status"]] == [0] * self.n
        return new_blobs, res["records"]

    def want(self, new_blobs, r):
        return self.heads[r] + struct.pack("<Q", len(new_blobs[r])) + new_blobs[r] + self.tails[r]


@pytest.fixture(scope="module")
def job(gpu):
    j = gpu.Job(0)
    yield j
    j.close()


@pytest.mark.parametrize("name", sorted(TABLES))
def test_records_come_from_the_inflated_arena(gpu, job, name):
    b = Batch(gpu, LENS, TABLES[name], seed=51)
    assert {len(h) % 4 for h in b.heads} == {0, 1, 2, 3} and any(len(h) == 38 for h in b.heads)
    if name == "array":
        assert {len(t) for t in b.tails} == {12 + 8 + k for k in ARRAY_BYTES}
        assert any(len(p) == r for p, r in zip(b.plain, b.room))      # (an array of exactly the slack fills the room)
    if name == "none":
        assert all(t == b"" for t in b.tails)
    new_blobs, frame_records = b.oracle(gpu, job)
    for r in range(b.n):   # the quantiser and the encoder, independently of the GPU
        assert new_blobs[r] == blow5.svb_zd_encode(quantise_round(b.reads[r], BITS)), r
    b.stage(job, b.compressed(stored=STORED))
    job.launch_qts(BITS, METHOD, True, records=True, zrec_frames=True)
    res = job.wait()
    assert "blobs" not in res and [int(s) for s in res["record_status"]] == [0] * b.n
    for r in range(b.n):
        assert zlib.decompress(res["records"][r]) == b.want(new_blobs, r), (r, b.lens[r])
    assert res["records"] == frame_records
    small = [len(x) for x in new_blobs if len(x) <= 80]
    assert any(x < 64 for x in small) and any(x >= 64 for x in small)     # both sides of the dword copy's threshold


def test_more_records_than_one_workgroup_of_the_sizing_kernel(gpu, job):
    lens = [(7 * k) % 41 for k in range(333)]
    b = Batch(gpu, lens, TABLES["array"], seed=52)
    new_blobs, frame_records = b.oracle(gpu, job)
    b.stage(job)
    job.launch_qts(BITS, METHOD, True, records=True, zrec_frames=True)
    res = job.wait()
    assert [int(s) for s in res["record_status"]] == [0] * b.n
    assert all(zlib.decompress(res["records"][r]) == b.want(new_blobs, r) for r in range(b.n))
    assert res["records"] == frame_records


def file_records(path, n):
    buf = open(path, "rb").read()
    (hsize,) = struct.unpack_from("<I", buf, 64)
    pos, recs = 68 + hsize, []
    while len(recs) < n:
        (size,) = struct.unpack_from("<Q", buf, pos)
        recs.append(buf[pos + 8:pos + 8 + size])
        pos += 8 + size
    return recs


def zstd_content_size(frame):
    """Frame_Content_Size of a zstd frame header (RFC 8878 3.1.1.1)"""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    d = frame[4]
    single, fcs_flag, dict_flag = (d >> 5) & 1, d >> 6, d & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag]
    n = (1 if single else 0, 2, 4, 8)[fcs_flag]
    assert n
    return int.from_bytes(frame[pos:pos + n], "little") + (256 if n == 2 else 0)


def test_zstd_frames_at_exact_room_give_the_zlib_fixtures_records(gpu, job, sp1):
    n = 24
    table = [(8, 0), (4, 0), (1, 0), (8, 0), (1, 0), (1, 1)]     # the fixture's columns (tests/test_gpu_zrec_aux.py pins them)
    reads = sp1.reads[:n]
    zl, zs = file_records(SP1, n), file_records(SP1_ZSTD, n)
    plain = [zlib.decompress(r) for r in zl]
    place = []
    for p in plain:
        (idl,) = struct.unpack_from("<H", p, 0)
        (ln,) = struct.unpack_from("<Q", p, 2 + idl + 36)
        place.append((2 + idl + 44, ln))
    lens = [r.raw.size for r in reads]
    scal = ([r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads])
    so, sl = [o for o, _ in place], [ln for _, ln in place]
    out = {}
    for key, recs, room, fmt in (("zlib", zl, [zlib_room(o + ln, table) for o, ln in place], gpu.RECORD_ZLIB),
                                 ("zstd", zs, [zstd_content_size(f) for f in zs], gpu.RECORD_ZSTD)):
        job.stage_zrec(recs, lens, so, sl, room, *scal, record_format=fmt, aux=table)
        job.launch_qts(1, 1, True, records=True, zrec_frames=True)
        res = job.wait()
        assert [int(s) for s in res["record_status"]] == [0] * n
        out[key] = res["records"]
    assert [zstd_content_size(f) for f in zs] == [len(p) for p in plain]
    assert out["zstd"] == out["zlib"]
    for r in range(n):
        blob = blow5.svb_zd_encode(quantise_round(reads[r].raw, 1))
        o, ln = place[r]
        assert zlib.decompress(out["zstd"][r]) == plain[r][:o - 8] + struct.pack("<Q", len(blob)) + blob + plain[r][o + ln:], r


def test_unsound_records_are_left_out_and_the_others_are_right(gpu, job):
    lens = [5, 30, 4096, 47, 1, 60, 33, 4097, 0, 25]
    b = Batch(gpu, lens, TABLES["array"], seed=53)
    new_blobs, _ = b.oracle(gpu, job)
    recs = b.compressed()
    room = list(b.room)
    long_r, cut_r, adler_r = 2, 5, 7
    # a 300-byte string in the array column: more than the record's room -> 0x108
    assert TABLES["array"][1] == (1, 1)
    head_sig = b.plain[long_r][:b.sig_off[long_r] + b.sig_len[long_r]]
    recs[long_r] = zlib.compress(head_sig + b"\x11" * 8 + struct.pack("<Q", 300) + b"c" * 300 + b"\x22" * 4)
    # re-deflated a tail byte short: it inflates, its fields do not fill it -> 0x400 | 2
    recs[cut_r] = zlib.compress(b.plain[cut_r][:-1])
    # a flipped byte of the Adler-32 behind the stream
    z = bytearray(recs[adler_r])
    z[-2] ^= 0x40
    recs[adler_r] = bytes(z)
    bad = (long_r, cut_r, adler_r)
    b.stage(job, recs, room)
    job.launch(gpu.TOOL_STAT)
    rc, want_ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT
    assert int(want_ds[long_r]) == 0x108 and int(want_ds[cut_r]) == 0x400 | 2 and int(want_ds[adler_r]) & 0xf00 == 0x100
    assert all(int(want_ds[r]) == 0 for r in range(b.n) if r not in bad)
    job.launch_qts(BITS, METHOD, True, records=True, zrec_frames=True)
    rc, ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT and [int(x) for x in ds] == [int(x) for x in want_ds]
    res = job.output()
    for r in range(b.n):
        if r in bad:
            assert int(res["record_status"][r]) == 2 and res["records"][r] == b"", r
        else:
            assert int(res["record_status"][r]) == 0 and zlib.decompress(res["records"][r]) == b.want(new_blobs, r), r


def test_the_flag_is_refused_where_it_does_not_apply(gpu, job):
    b = Batch(gpu, [30, 100], TABLES["fixed"], seed=54)
    # control: on a blob-staged batch (refused before the flag existed as well: 0x200 was no format then)
    job.stage(b.blobs, *b.scal, counts=b.lens)
    job.set_record_frames([h + t for h, t in zip(b.heads, b.tails)], [len(h) for h in b.heads])
    with pytest.raises(gpu.SigtkGpuError):
        job.launch_qts(BITS, METHOD, True, records=True, zrec_frames=True)
    b.stage(job)
    with pytest.raises(gpu.SigtkGpuError):      # without SGK_QTS_RECORDS
        job.launch_qts(BITS, METHOD, True, records=False, zrec_frames=True)
    with pytest.raises(gpu.SigtkGpuError):      # int16 out: a ZREC batch is svb-zd
        job.launch_qts(BITS, METHOD, False, records=True, zrec_frames=True)
    with pytest.raises(gpu.SigtkGpuError):      # text out
        job.launch_qts(BITS, METHOD, True, records=True, out_text=True, zrec_frames=True)
    job.launch_qts(BITS, METHOD, True, records=True, zrec_frames=True)     # the batch is still good for the real thing
    assert [int(s) for s in job.wait()["record_status"]] == [0, 0]
    assert gpu.QTS_ZREC_FRAMES == 0x200
