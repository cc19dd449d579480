"""GPU: sgk_inflate (csrc/inflate_kernels.hip) -- zlib streams inflated one wavefront each -- against Python's zlib
(the library slow5lib itself calls, slow5lib/src/slow5_press.c:77-98): every block type, every level and window size,
sizes around the kernel's chunk / flush / window boundaries, and the malformed streams zlib rejects.  zlib's compressor
writes a small corner of what its inflate accepts: the rest comes from tests/deflate_craft.py, hand-built streams that
tests/test_deflate_craft_cpu.py has zlib judge."""
import zlib

import numpy as np
import pytest

import deflate_craft

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted_valid():
    return deflate_craft.valid_streams()


@pytest.fixture(scope="module")
def crafted_invalid():
    return deflate_craft.invalid_streams()


def _payloads():
    rs = np.random.RandomState(5)
    text = (b"the quick brown fox jumps over the lazy dog, 0123456789; " * 6000)
    from sigtk_amd import api, blow5
    reads, *_ = api.synth_reads_host(2, 100000, 3, 0)
    svb = blow5.svb_zd_encode(reads[0])
    out = {"empty": b"", "one": b"x", "five": b"hello", "zeros": bytes(70000), "text": text,
           "random": rs.bytes(200000), "svb": svb, "svb2": blow5.svb_zd_encode(reads[1]) + rs.bytes(333),
           "runs": b"".join(bytes([i % 251]) * (1 + (i * 7) % 300) for i in range(3000)),
           "walk": np.cumsum(rs.randint(-2, 3, size=150000)).astype(np.int8).tobytes()}
    for n in (255, 256, 257, 1023, 1024, 1025, 32767, 32768, 32769, 65535, 65536, 65537):
        out["text%d" % n] = text[:n]
        out["rand%d" % n] = rs.bytes(n)
    return out


def test_every_block_type_level_and_window(gpu):
    from sigtk_amd import device
    pay = _payloads()
    streams, want = [], []
    for name, data in pay.items():
        for level in (0, 1, 6, 9):
            streams.append(zlib.compress(data, level)); want.append(data)
        for wbits in (9, 12, 15):
            c = zlib.compressobj(6, zlib.DEFLATED, wbits)
            streams.append(c.compress(data) + c.flush()); want.append(data)
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)      # fixed Huffman blocks
        streams.append(c.compress(data) + c.flush()); want.append(data)
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        streams.append(c.compress(data) + c.flush()); want.append(data)
        c = zlib.compressobj(6)                                          # several blocks, sync flushes (empty stored blocks)
        parts = [c.compress(data[i:i + 7001]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(data), 7001)]
        streams.append(b"".join(parts) + c.flush()); want.append(data)
    got, olen, st = device.inflate(streams, caps=[len(w) + 5 for w in want])
    for r, w in enumerate(want):
        assert st[r] == 0, (r, st[r])
        assert olen[r] == len(w), (r, olen[r], len(w))
        assert got[r] == w, r


def test_room(gpu):
    """out_caps[r] must hold the whole stream (far matches read the stream's own earlier bytes from the output): exactly
    enough is enough, one byte less is status 8"""
    from sigtk_amd import device
    pay = _payloads()
    data = pay["svb"] + pay["text"][:50000]
    s = zlib.compress(data)
    caps = [0, 1, 1024, len(pay["svb"]), len(data) - 1, len(data), len(data) + 100]
    got, olen, st = device.inflate([s] * len(caps), caps=caps)
    for r, c in enumerate(caps):
        if c >= len(data):
            assert st[r] == 0 and olen[r] == len(data) and got[r] == data
        else:
            assert st[r] == 8, (c, st[r])


def test_streams_zlib_rejects(gpu):
    from sigtk_amd import device
    pay = _payloads()
    good = zlib.compress(pay["svb"])
    bad = {}
    bad["truncated"] = good[:len(good) // 2]
    bad["no adler"] = good[:-4]
    bad["adler"] = good[:-1] + bytes([good[-1] ^ 1])
    bad["header"] = bytes([0x79]) + good[1:]
    bad["method"] = bytes([0x77, 0x9c]) + good[2:]          # CM != 8 (FCHECK still fine? 0x779c % 31 -> adjusted below)
    bad["dict"] = bytes([0x78, 0xbb]) + good[2:]            # FDICT set, 0x78bb % 31 == 0
    bad["short"] = good[:3]
    stored = zlib.compress(pay["random"][:1000], 0)
    bad["stored len"] = stored[:3] + bytes([stored[3] ^ 0xff]) + stored[4:]
    bad["block type 3"] = bytes([0x78, 0x9c, 0x07]) + good[3:]
    rs = np.random.RandomState(7)
    for k in range(24):                                     # a flipped bit somewhere in the middle
        i = int(rs.randint(2, len(good) - 4))
        bad["flip%d" % k] = good[:i] + bytes([good[i] ^ (1 << int(rs.randint(8)))]) + good[i + 1:]
    names = list(bad)
    got, olen, st = device.inflate([bad[k] for k in names], caps=[len(pay["svb"]) + 64] * len(names))
    for r, k in enumerate(names):
        try:
            zlib.decompress(bad[k])
            ok = True
        except zlib.error:
            ok = False
        assert not ok, k           # (zlib rejects every one of these)
        assert st[r] != 0, (k, st[r])
    # ... and the good one among them is still fine
    got, olen, st = device.inflate([good, bad["adler"], good], caps=[1 << 20] * 3)
    assert list(st) == [0, 7, 0] and got[0] == pay["svb"] and got[2] == pay["svb"]


def test_many_streams_at_once(gpu):
    """more streams than the GPU holds at once, of very different sizes"""
    from sigtk_amd import device
    rs = np.random.RandomState(11)
    base = _payloads()["walk"]
    want = [base[int(a):int(a) + int(n)] for a, n in zip(rs.randint(0, 50000, 3000), rs.randint(0, 90000, 3000))]
    got, olen, st = device.inflate([zlib.compress(w, int(rs.randint(1, 10))) for w in want], caps=[len(w) for w in want])
    assert (st == 0).all()
    assert all(g == w for g, w in zip(got, want))


def _check_exact(names, want, res):
    """status 0, the exact length, the exact bytes, and nothing written behind them (caps were the exact lengths: a byte
    too many lands in the gap up to the next stream's area, or in that stream's bytes)"""
    got, olen, st, gaps = res
    wrong = [(n, int(st[r]), int(olen[r]), len(w)) for r, (n, w) in enumerate(zip(names, want))
             if st[r] != 0 or olen[r] != len(w) or got[r] != w or any(gaps[r])]
    assert not wrong, "(name, status, out_length, expected length):\n" + "\n".join(map(str, wrong))


def test_crafted_valid_streams_with_exact_room(gpu, crafted_valid):
    """every well-formed stream of the crafted catalogue (long distance and literal codes, the ring's seams, overlapping
    matches, every length / distance symbol, 1-bit literal codes, every way a literal run ends, the code length
    encoding's corners, stored blocks at every bit offset, empty blocks, 200+ random ones) in one launch"""
    from sigtk_amd import device
    names = [n for n, _, _ in crafted_valid]
    want = [w for _, _, w in crafted_valid]
    _check_exact(names, want, device.inflate([s for _, s, _ in crafted_valid], caps=[len(w) for w in want], with_gaps=True))


def test_crafted_invalid_streams_give_their_status(gpu, crafted_valid, crafted_invalid):
    """one fault per stream, the status include/sigtk_gpu.h documents for it -- with valid streams in between, which
    must not notice"""
    from sigtk_amd import device
    good = [crafted_valid[k] for k in range(0, len(crafted_valid), 23)]
    streams, expect = [], []
    for k, (name, stream, status, _) in enumerate(crafted_invalid):
        streams.append(stream); expect.append((name, status, None))
        if k % 4 == 0:
            g = good[(k // 4) % len(good)]
            streams.append(g[1]); expect.append((g[0], 0, g[2]))
    got, olen, st = device.inflate(streams, caps=[1 << 17] * len(streams))
    wrong = [(name, int(st[r]), status) for r, (name, status, w) in enumerate(expect)
             if st[r] != status or (w is not None and (got[r] != w or olen[r] != len(w)))]
    assert not wrong, "(name, status, expected status):\n" + "\n".join(map(str, wrong))


def test_ring_seams_at_other_offsets(gpu, crafted_valid):
    """the matches at the ring's reach (3838: ring, 3839: global memory), at 32768 and at distance == position, behind 0, 1,
    1023, 1024 and 1025 literals (the flush boundary either side of the match's source and destination) -- in a launch
    of their own and in reverse order, so that every stream sits at another alignment than in the catalogue's launch"""
    from sigtk_amd import device
    seams = [c for c in crafted_valid if c[0].startswith(("seam_", "stored_header_at_bit"))][::-1]
    assert len(seams) >= 40
    for shift in (0, 1):
        part = [("pad", zlib.compress(b"x"), b"x")] * shift + seams
        _check_exact([n for n, _, _ in part], [w for _, _, w in part],
                     device.inflate([s for _, s, _ in part], caps=[len(w) for _, _, w in part], with_gaps=True))


def test_literal_runs_that_end_at_the_input_windows_seam(gpu, crafted_valid):
    """the kernel reads its input 256 bytes at a time, counted from the 4-byte boundary in front of the stream's first
    byte; run_ends_at_input_seam_lead<k>_* have a run of 1-bit literals end at that seam (and one bit either side of it,
    in a match or in more literals) when the stream's first byte sits at address % 4 == k -- so each is put there, and
    at the three other alignments too, where the seam falls inside the run"""
    from sigtk_amd import device
    cases = [c for c in crafted_valid if deflate_craft.lead_of(c[0]) is not None]
    assert len(cases) == 24 and {deflate_craft.lead_of(c[0]) for c in cases} == {0, 1, 2, 3}
    for shift in range(4):
        leads = [(deflate_craft.lead_of(c[0]) + shift) & 3 for c in cases]
        offs, _ = device.inflate_input_offsets([s for _, s, _ in cases], leads)
        assert [int(o) % 4 for o in offs] == leads
        if shift == 0:
            assert [int(o) % 4 for o in offs] == [deflate_craft.lead_of(c[0]) for c in cases]
        res = device.inflate([s for _, s, _ in cases], caps=[len(w) for _, _, w in cases], with_gaps=True, leads=leads)
        _check_exact([n for n, _, _ in cases], [w for _, _, w in cases], res)


def test_adler_sums_at_their_largest(gpu, crafted_valid):
    """70 000 bytes of 0xff, and of 0xff 0x00: through zlib's compressor (every level) and as stored blocks only"""
    from sigtk_amd import device
    names, streams, want = [], [], []
    for tag, data in (("ff", b"\xff" * 70000), ("ff00", b"\xff\x00" * 35000), ("ff_odd", b"\xff" * 65521),
                      ("ff_5552", b"\xff" * 5553)):
        for level in (0, 1, 6, 9):
            names.append("%s level %d" % (tag, level)); streams.append(zlib.compress(data, level)); want.append(data)
    for n, s, w in crafted_valid:
        if n.startswith("adler_"):
            names.append(n); streams.append(s); want.append(w)
    assert len(names) == 18
    _check_exact(names, want, device.inflate(streams, caps=[len(w) for w in want], with_gaps=True))
