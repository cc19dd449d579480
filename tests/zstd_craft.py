"""A zstd frame WRITER for tests (RFC 8878), written from the RFC: frame and block headers of every layout, Raw / RLE
literals, a sequences section whose three symbol codings are all in RLE mode -- the FSE states then take no bits and the
bitstream holds the extra bits alone, so any literal-length, offset and match-length code is written without an FSE
encoder -- and what no compressor writes and no decoder may accept.  Two catalogues, a walker and the fixture's payloads:

    valid_frames()     -> [(name, frame, expected bytes)]
    invalid_frames()   -> [(name, frame, status of sgk_zstd_decompress / zstd_dec.c, True if libzstd's one-shot decoder takes it)]
    walk(frame)        -> the set of coverage items its blocks show ("block:raw", "lit:treeless", "streams:4", "ll:fse", ...)
    COVERAGE           -> every item the fixture and the crafted catalogue together must show
    payload(gen, seed, n) / fixture() -> the payloads of tests/golden/zstd_frames.npz, regenerated from their recipes
    mutations(frames, n, seed) -> seeded bit flips, truncations and overwritten spans

The cases sit on the constants of sigtk_amd/csrc/zstd_kernels.hip (NEAR = 4032: the furthest match served from the LDS
ring, FLUSH = 1024: bytes per flush, 64 bytes per copy step), named here only as numbers."""
import os
import struct
import zlib

import numpy as np

NEAR, FLUSH, STEP, BLOCK_MAX = 4032, 1024, 64, 128 << 10
MAGIC = b"\x28\xb5\x2f\xfd"

LL_BASE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024,
           2048, 4096, 8192, 16384, 32768, 65536)
LL_BITS = (0,) * 16 + (1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
ML_BASE = tuple(range(3, 35)) + (35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387,
                                 32771, 65539)
ML_BITS = (0,) * 32 + (1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)

ST_HEADER, ST_BLOCK, ST_TABLE, ST_SECTION, ST_OFFSET, ST_TRUNCATED, ST_CHECKSUM, ST_SIZE = 1, 2, 3, 4, 5, 6, 7, 8

COVERAGE = frozenset(["block:raw", "block:rle", "block:compressed", "lit:raw", "lit:rle", "lit:compressed", "lit:treeless",
                      "streams:1", "streams:4"] +
                     ["%s:%s" % (t, m) for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")])


# ------------------------------------------------------------------------------------------------ XXH64 (seed 0)

_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(data):
    n, p = len(data), 0
    if n >= 32:
        v = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        while p + 32 <= n:
            w = struct.unpack_from("<4Q", data, p)
            v = [_round(v[k], w[k]) for k in range(4)]
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _round(0, v[k])) * _P1 + _P4) & _M
    else:
        h = _P5
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, p)[0] * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & _M), 11) * _P1) & _M
        p += 1
    h ^= h >> 33
    h = h * _P2 & _M
    h ^= h >> 29
    h = h * _P3 & _M
    h ^= h >> 32
    return h


# ------------------------------------------------------------------------------------------------ the writer

def frame_header(size, fcs_bytes=None, single=True, checksum=False, window_exp=7, dict_id=None, reserved=False):
    """size None: no Frame_Content_Size field; fcs_bytes 1 / 2 / 4 / 8 (None: the smallest that holds size; 1 needs
    single); dict_id: bytes of the Dictionary_ID field (1, 2 or 4 of them)"""
    if size is None:
        flag, fcs, single = 0, b"", False
    else:
        if fcs_bytes is None:
            fcs_bytes = 1 if size < 256 and single else (2 if 256 <= size < 65792 else (4 if size < 1 << 32 else 8))
        assert fcs_bytes != 1 or single
        flag = {1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        fcs = (size - 256 if fcs_bytes == 2 else size).to_bytes(fcs_bytes, "little")
    did = dict_id or b""
    d = (flag << 6) | (int(single) << 5) | (int(reserved) << 3) | (int(checksum) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[len(did)]
    return MAGIC + bytes([d]) + (b"" if single else bytes([window_exp << 3])) + did + fcs


def block(btype, last, content, size=None):
    """btype 0 raw, 1 RLE (content: the byte; size: the count), 2 compressed, 3 reserved"""
    if size is None:
        size = len(content)
    return (int(last) | (btype << 1) | (size << 3)).to_bytes(3, "little") + content


def lit_header(ltype, regen, fmt=None):
    """Raw (0) / RLE (1) literals section header; fmt: size format 0 / 2 (one byte), 1 (two), 3 (three)"""
    if fmt is None:
        fmt = 0 if regen < 32 else (1 if regen < 4096 else 3)
    if fmt in (0, 2):
        assert regen < 32
        return bytes([ltype | (fmt << 2) | (regen << 3)])
    if fmt == 1:
        assert regen < 4096
        return (ltype | (1 << 2) | (regen << 4)).to_bytes(2, "little")
    assert regen < 1 << 20
    return (ltype | (3 << 2) | (regen << 4)).to_bytes(3, "little")


def nseq_bytes(n, width=None):
    if width is None:
        width = 1 if n < 128 else (2 if n < 0x7f00 else 3)
    if width == 1:
        assert n < 128
        return bytes([n])
    if width == 2:
        assert n < 0x7f00
        return bytes([128 + (n >> 8), n & 255])
    assert n >= 0x7f00
    return b"\xff" + (n - 0x7f00).to_bytes(2, "little")


def rev_bits(reads):
    """a bitstream read backwards: `reads` are (value, bits) in the order the decoder reads them"""
    acc, total = 1, 1
    for v, nb in reads:
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        acc = (acc << nb) | v
        total += nb
    return acc.to_bytes((total + 7) // 8, "little")


def fse_dist(probas, log):
    """an FSE distribution as 4.1.1 writes it (probas: -1 'less than one', 0 followed by its repeat flags as (0, flags))"""
    acc, nbits = log - 5, 4
    remaining = 1 << log
    for p in probas:
        flags = ()
        if isinstance(p, tuple):
            p, flags = p
        x = p + 1
        nb = (remaining + 1).bit_length()
        lower, thresh = (1 << (nb - 1)) - 1, (1 << nb) - 1 - (remaining + 1)
        if x < thresh:
            acc |= x << nbits
            nbits += nb - 1
        else:
            acc |= (x if x <= lower else x + thresh) << nbits
            nbits += nb
        remaining -= 1 if p < 0 else p
        for f in flags:
            acc |= f << nbits
            nbits += 2
    return acc.to_bytes((nbits + 7) // 8, "little")


class Frame:
    """blocks appended one by one, the expected output and the repeat offsets simulated on the way"""

    def __init__(self):
        self.blocks = []
        self.out = bytearray()
        self.rep = [1, 4, 8]

    def raw(self, data):
        self.blocks.append((0, bytes(data), None))
        self.out += data
        return self

    def rle(self, byte, n):
        self.blocks.append((1, bytes([byte]), n))
        self.out += bytes([byte]) * n
        return self

    def seqs(self, lits, codes, extras, tail=0, nseq_width=None, lit_fmt=None):
        """a compressed block: lits = bytes (Raw literals) or (byte, count) (RLE literals); codes = (ll, of, ml) codes, all
        in RLE mode; extras = [(ll extra, of extra, ml extra)] per sequence; tail: literals behind the last sequence"""
        llc, ofc, mlc = codes
        rle = isinstance(lits, tuple)
        src = bytes([lits[0]]) * lits[1] if rle else bytes(lits)
        at, reads = 0, []
        for lx, ox, mx in extras:
            ll, ml, ov = LL_BASE[llc] + lx, ML_BASE[mlc] + mx, (1 << ofc) + ox
            reads += [(ox, ofc), (mx, ML_BITS[mlc]), (lx, LL_BITS[llc])]
            self.out += src[at:at + ll]
            at += ll
            rep = self.rep
            if ov > 3:
                off = ov - 3
                self.rep = [off, rep[0], rep[1]]
            else:
                idx = ov - 1 + (ll == 0)
                if idx == 0:
                    off = rep[0]
                else:
                    off = rep[0] - 1 if idx == 3 else rep[idx]
                    self.rep = [off, rep[0], rep[2] if idx == 1 else rep[1]]
            assert 0 < off <= len(self.out), (off, len(self.out))
            for _ in range(ml):
                self.out.append(self.out[-off])
        assert at + tail == len(src), (at, tail, len(src))
        self.out += src[at:]
        body = lit_header(1 if rle else 0, len(src), lit_fmt) + (src[:1] if rle else src)
        body += nseq_bytes(len(extras), nseq_width)
        if extras:
            body += bytes([0x54, llc, ofc, mlc]) + rev_bits(reads)
        self.blocks.append((2, body, None))
        return self

    def body(self, body):
        """a compressed block given as bytes (its output is the caller's business)"""
        self.blocks.append((2, bytes(body), None))
        return self

    def build(self, size="auto", checksum=False, bad_checksum=False, **hdr):
        n = len(self.out) if size == "auto" else size
        out = frame_header(n, checksum=checksum, **hdr)
        for k, (t, content, sz) in enumerate(self.blocks):
            out += block(t, k == len(self.blocks) - 1, content, sz)
        if checksum:
            out += ((xxh64(bytes(self.out)) ^ int(bad_checksum)) & 0xffffffff).to_bytes(4, "little")
        return out


def _rs(seed):
    return np.random.RandomState(seed)


def valid_frames():
    out = []

    def add(name, f, **kw):
        out.append((name, f.build(**kw), bytes(f.out)))

    rnd = _rs(3).bytes(70000)
    add("empty_raw_block", Frame().raw(b""))
    add("rle_block", Frame().rle(0x41, 1000))
    add("rle_block_128k", Frame().rle(7, BLOCK_MAX).rle(9, 1).raw(b"xyz"))
    add("raw_then_rle_then_raw", Frame().raw(rnd[:100]).rle(0, 5000).raw(rnd[100:333]))
    # Frame_Content_Size widths, window descriptor, checksum
    for w in (1, 2, 4, 8):
        n = 200 if w == 1 else 300
        add("fcs_%d_bytes" % w, Frame().raw(rnd[:n]), fcs_bytes=w)
    add("fcs_2_bytes_at_256", Frame().raw(rnd[:256]), fcs_bytes=2)
    add("fcs_2_bytes_at_65791", Frame().raw(rnd[:65791]), fcs_bytes=2)
    add("window_descriptor", Frame().raw(rnd[:500]), single=False, fcs_bytes=4)
    add("window_descriptor_fcs_8", Frame().raw(rnd[:77]), single=False, fcs_bytes=8, window_exp=20)
    add("dictionary_id_zero", Frame().raw(rnd[:77]), dict_id=b"\0\0")
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025, 70000):
        add("checksum_%d" % n, Frame().raw(rnd[:n]), checksum=True)
    add("checksum_sequences", Frame().raw(rnd[:50]).seqs((0x55, 20), (4, 5, 7), [(0, 3, 0), (0, 30, 0)], tail=12), checksum=True)
    # RLE literals, Raw literals in every size format, literals only
    add("rle_literals_only", Frame().seqs((0x33, 700), (0, 0, 0), [], tail=700))
    for fmt, n in ((0, 31), (2, 17), (1, 31), (1, 4095), (3, 31), (3, 4096), (3, 70000)):
        add("raw_literals_fmt%d_%d" % (fmt, n), Frame().seqs(rnd[:n], (0, 0, 0), [], tail=n, lit_fmt=fmt))
        add("rle_literals_fmt%d_%d" % (fmt, n), Frame().seqs((n & 255, n), (0, 0, 0), [], tail=n, lit_fmt=fmt))
    add("rle_literals_128k", Frame().seqs((1, BLOCK_MAX), (0, 0, 0), [], tail=BLOCK_MAX, lit_fmt=3))
    # offsets and match lengths in RLE mode; every offset code that fits; overlapping matches
    for ofc in range(2, 17):
        f = Frame().raw(rnd[:60000]).raw(rnd[60000:70000])
        top = min((1 << ofc) - 1, 70003 - (1 << ofc))
        f.seqs(rnd[:9], (3, ofc, 5), [(0, 0, 0), (0, top, 0), (0, top // 2, 0)])
        add("offset_code_%d" % ofc, f)
    for off in (1, 2, 3, 5, 63, 64, 65, 100):
        ofc = (off + 3).bit_length() - 1
        f = Frame().raw(rnd[:200]).seqs(rnd[:4], (2, ofc, 40), [(0, off + 3 - (1 << ofc), 9), (0, off + 3 - (1 << ofc), 15)])
        add("overlap_offset_%d" % off, f)
    add("offset_1_long_run", Frame().raw(b"Q").seqs(b"", (0, 2, 52), [(0, 0, 65530)]))
    # the repeat offsets: value 1 / 2 / 3 with literals and without; the offsets are set by a first block
    for ll in (1, 0):
        for val in (1, 2, 3):
            f = Frame().raw(rnd[:300])
            f.seqs(rnd[:6], (2, 5, 3), [(0, 7, 0), (0, 19, 0), (0, 30, 0)])           # offsets 36, 48, 59 -> rep = 59, 48, 36
            ofc, ox = (0, 0) if val == 1 else (1, val - 2)
            f.seqs(rnd[:3 * ll], (ll, ofc, 6), [(0, ox, 0)] * 3)
            add("repeat_offset_%d_ll%d" % (val, ll), f)
    f = Frame().raw(rnd[:64]).seqs(rnd[:2], (1, 3, 0), [(0, 2, 0), (0, 5, 0)]).rle(3, 10).seqs(b"", (0, 1, 9), [(0, 1, 0)])
    add("repeat_offsets_across_blocks", f)
    # the largest length codes (a block holds 128 KB: one at a time)
    add("literal_length_code_35", Frame().seqs((0x5a, 65536 + 60000), (35, 2, 0), [(60000, 1, 0)]))
    add("match_length_code_52", Frame().raw(rnd[:5000]).seqs(rnd[:1], (1, 10, 52), [(0, 77, 65532)]))
    for c in range(16, 35):
        add("literal_length_code_%d" % c, Frame().seqs((c, LL_BASE[c] + (1 << LL_BITS[c]) - 1), (c, 2, 1), [((1 << LL_BITS[c]) - 1, 0, 0)]))
    for c in range(32, 52):
        add("match_length_code_%d" % c, Frame().raw(rnd[:100]).seqs(b"", (0, 6, c), [(0, 9, (1 << ML_BITS[c]) - 1)]))
    # the three encodings of the sequence count
    add("nseq_1_byte", Frame().raw(rnd[:40]).seqs(rnd[:127], (1, 4, 0), [(0, k % 16, 0) for k in range(127)]))
    add("nseq_2_bytes_small", Frame().raw(rnd[:40]).seqs(rnd[:5], (1, 4, 0), [(0, k, 0) for k in range(5)], nseq_width=2))
    add("nseq_2_bytes", Frame().raw(rnd[:40]).seqs(rnd[:300], (1, 4, 0), [(0, k % 16, 0) for k in range(300)]))
    add("nseq_3_bytes", Frame().raw(b"ab").seqs((0x21, 0x7f00 + 5), (1, 0, 0), [(0, 0, 0)] * (0x7f00 + 5)))
    # the ring's reach (4032: ring, 4033: global memory), the flush boundary, long far matches, far matches across blocks
    for pre in (0, 1, 1023, 1024, 1025):
        for off in (NEAR - 1, NEAR, NEAR + 1, NEAR + 63, NEAR + 64, 8192, 65536):
            ofc = (off + 3).bit_length() - 1
            f = Frame().raw(rnd[:65536]).raw(rnd[:pre])
            f.seqs(rnd[7:10], (3, ofc, 47), [(0, off + 3 - (1 << ofc), 200)])
            add("seam_pre%d_off%d" % (pre, off), f)
    f = Frame().raw(rnd[:66000])
    f.seqs(rnd[:10], (5, 16, 50), [(0, 0, 100), (0, 400, 16000)])
    add("far_match_65k_twice", f)
    add("tail_literals_after_last_sequence", Frame().raw(rnd[:9]).seqs(rnd[:50], (4, 2, 0), [(0, 1, 0)], tail=46))
    add("many_blocks", _many_blocks(rnd))
    return out


def _many_blocks(rnd):
    f = Frame()
    for k in range(40):
        if k % 3 == 0:
            f.raw(rnd[k * 100:k * 100 + 50 + k])
        elif k % 3 == 1:
            f.rle(k, 3 * k)
        else:
            f.seqs(rnd[k:k + 8], (4, 4, k % 32), [(0, k % 16, 0), (0, (k * 7) % 16, 0)])
    return f


def _huf_literals_body(weights_direct):
    """a compressed block whose literals are Huffman coded, one stream, with the weights given directly"""
    n = len(weights_direct)
    tree = bytes([127 + n]) + bytes((weights_direct[i] << 4) | (weights_direct[i + 1] if i + 1 < n else 0) for i in range(0, n, 2))
    comp = tree + b"\x01"
    hdr = (2 | (0 << 2) | (1 << 4) | (len(comp) << 14)).to_bytes(3, "little")
    return hdr + comp + b"\x00"


def invalid_frames():
    out = []
    rnd = _rs(4).bytes(3000)

    def add(name, frame, status, libzstd_takes=False):
        out.append((name, bytes(frame), status, libzstd_takes))

    good = Frame().raw(rnd[:100]).seqs(rnd[:20], (4, 5, 7), [(0, 3, 0), (0, 30, 0)], tail=12)
    g = good.build()
    # frame header
    add("no_content_size", frame_header(None) + block(0, True, rnd[:10]), ST_HEADER)
    add("dictionary_id", Frame().raw(rnd[:10]).build(dict_id=b"\x07"), ST_HEADER)
    add("dictionary_id_4_bytes", Frame().raw(rnd[:10]).build(dict_id=b"\0\0\0\x01"), ST_HEADER)
    add("reserved_bit", Frame().raw(rnd[:10]).build(reserved=True), ST_HEADER)
    add("skippable_frame", b"\x50\x2a\x4d\x18" + (4).to_bytes(4, "little") + b"abcd", ST_HEADER, True)
    add("bad_magic", b"\x28\xb5\x2f\xfc" + g[4:], ST_HEADER)
    add("trailing_byte", g + b"\0", ST_HEADER)
    add("second_frame", g + Frame().raw(b"").build(), ST_HEADER, True)
    # block header
    add("block_type_3", frame_header(10) + block(3, True, rnd[:10]), ST_BLOCK)
    add("block_larger_than_128k", frame_header(BLOCK_MAX + 1, fcs_bytes=4) + block(0, True, bytes(BLOCK_MAX + 1)), ST_BLOCK, True)
    add("block_larger_than_the_input", frame_header(100) + block(0, True, rnd[:99], size=100), ST_TRUNCATED)
    # table descriptions
    add("huffman_weights_no_power_of_two", Frame().body(_huf_literals_body([2, 2, 1])).build(size=1), ST_TABLE)
    add("huffman_weights_all_zero", Frame().body(_huf_literals_body([0, 0, 0])).build(size=1), ST_TABLE)
    lit = lit_header(0, 4) + b"abcd" + b"\x01"
    for name, modes, desc in (
            ("fse_ll_log_10", 0x80, bytes([5])), ("fse_of_log_9", 0x20, bytes([4])), ("fse_ml_log_10", 0x08, bytes([5])),
            ("fse_ll_underfilled", 0x80, fse_dist([1] * 36, 6)),
            ("fse_ll_too_many_symbols", 0x80, fse_dist([(0, (3,) * 12)], 5)),
            ("fse_of_underfilled", 0x20, fse_dist([1] * 32, 6)),
            ("rle_ll_symbol_36", 0x40, bytes([36])), ("rle_of_symbol_32", 0x10, bytes([32])), ("rle_ml_symbol_53", 0x04, bytes([53])),
            ("repeat_ll_without_table", 0xc0, b""), ("repeat_of_without_table", 0x30, b""), ("repeat_ml_without_table", 0x0c, b"")):
        add(name, Frame().body(lit + bytes([modes]) + desc + b"\x01\x01\x01\x01").build(size=10), ST_TABLE)
    add("huffman_weights_fse_log_7", Frame().body((2 | (1 << 4) | (6 << 14)).to_bytes(3, "little") + bytes([4, 2, 0, 0, 0, 1]) + b"\0").build(size=1), ST_TABLE)
    add("treeless_without_table", Frame().body((3 | (1 << 4) | (2 << 14)).to_bytes(3, "little") + b"\x01\x01" + b"\0").build(size=1), ST_TABLE)
    # literals / sequences sections
    seq = lit_header(0, 4) + b"abcd" + b"\x01" + bytes([0x54, 1, 2, 0])
    add("bitstream_last_byte_zero", Frame().raw(rnd[:9]).body(seq + b"\x00").build(size=16), ST_SECTION)
    add("bitstream_too_short", Frame().raw(rnd[:9]).body(seq + b"\x01").build(size=16), ST_SECTION, True)
    add("bitstream_not_used_up", Frame().raw(rnd[:9]).body(seq + b"\x00\x01").build(size=16), ST_SECTION)
    add("sequence_modes_reserved_bits", Frame().raw(rnd[:9]).body(lit_header(0, 4) + b"abcd" + b"\x01" + bytes([0x55, 1, 2, 0]) + b"\x04").build(size=16), ST_SECTION, True)
    add("literals_missing", Frame().raw(rnd[:9]).body(lit_header(0, 1) + b"a" + b"\x01" + bytes([0x54, 2, 2, 0]) + b"\x04").build(size=14), ST_SECTION)
    add("no_sequences_but_more_bytes", Frame().body(lit_header(0, 2) + b"ab" + b"\x00\x00").build(size=2), ST_SECTION)
    add("raw_literals_past_the_block", Frame().body(lit_header(0, 20) + b"abc" + b"\x00").build(size=20), ST_SECTION)
    add("literals_larger_than_128k", Frame().body(lit_header(1, BLOCK_MAX + 1, 3) + b"a" + b"\x00").build(size=BLOCK_MAX + 1, fcs_bytes=4), ST_SECTION)
    add("no_sequences_section", Frame().body(lit_header(0, 2) + b"ab").build(size=2), ST_SECTION)
    # offsets
    add("offset_in_front_of_the_frame", Frame().raw(rnd[:9]).body(lit_header(0, 1) + b"a" + b"\x01" + bytes([0x54, 1, 4, 0]) + rev_bits([(0, 4), (0, 0), (0, 0)])).build(size=14), ST_OFFSET)
    add("offset_in_front_of_the_frame_first_block", Frame().body(lit_header(0, 1) + b"a" + b"\x01" + bytes([0x54, 1, 2, 0]) + rev_bits([(1, 2)])).build(size=4), ST_OFFSET)
    # (repeat offset 1 is 1 at the start: value 3 without literals asks for 1 - 1; libzstd makes that 1)
    add("offset_zero", Frame().raw(rnd[:9]).body(lit_header(0, 0) + b"\x01" + bytes([0x54, 0, 1, 0]) + rev_bits([(1, 1)])).build(size=12), ST_OFFSET, True)
    # the input's end
    for cut in (3, 4, 5, 7, 9, 50, len(g) - 1):
        add("cut_at_%d" % cut, g[:cut], ST_TRUNCATED)
    c = good.build(checksum=True)
    add("checksum_cut", c[:-2], ST_TRUNCATED)
    add("rle_block_without_its_byte", frame_header(5) + block(1, True, b"", size=5), ST_TRUNCATED)
    add("checksum_mismatch", good.build(checksum=True, bad_checksum=True), ST_CHECKSUM)
    # sizes
    add("shorter_than_declared", good.build(size=len(good.out) + 1), ST_SIZE)
    add("longer_than_declared", good.build(size=len(good.out) - 1), ST_SIZE)
    add("longer_than_declared_raw_block", Frame().raw(rnd[:100]).build(size=99), ST_SIZE)
    add("longer_than_declared_rle_block", Frame().rle(1, 100).build(size=99), ST_SIZE)
    add("longer_than_declared_match", Frame().raw(rnd[:100]).seqs(b"", (0, 4, 40), [(0, 0, 0)]).build(size=120), ST_SIZE)
    f = Frame().raw(b"a")
    f.seqs(b"", (0, 2, 52), [(0, 0, 65535)])
    f.seqs(b"", (0, 2, 52), [(0, 0, 65535)])
    add("block_decodes_to_more_than_128k", Frame().raw(b"a").body(
        lit_header(1, 3) + b"z" + b"\x02" + bytes([0x54, 0, 2, 52]) + rev_bits([(0, 2), (65535, 16), (0, 0)] * 2)).build(size=1 + 2 * 131074 + 3, fcs_bytes=4), ST_SIZE, True)
    return out


# ------------------------------------------------------------------------------------------------ the walker

def walk(frame):
    """the coverage items of a well-formed frame's blocks (block, literals and sequences headers only)"""
    items = set()
    assert frame[:4] == MAGIC
    d = frame[4]
    single = (d >> 5) & 1
    fcs = (1 << (d >> 6)) if d >> 6 else single
    at = 5 + (0 if single else 1) + {0: 0, 1: 1, 2: 2, 3: 4}[d & 3] + fcs
    last = False
    while not last:
        bh = int.from_bytes(frame[at:at + 3], "little")
        at += 3
        last, btype, bsize = bool(bh & 1), (bh >> 1) & 3, bh >> 3
        items.add("block:" + ("raw", "rle", "compressed")[btype])
        if btype != 2:
            at += bsize if btype == 0 else 1
            continue
        p = frame[at:at + bsize]
        at += bsize
        ltype, sf = p[0] & 3, (p[0] >> 2) & 3
        items.add("lit:" + ("raw", "rle", "compressed", "treeless")[ltype])
        if ltype < 2:
            hl = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
            regen = int.from_bytes(p[:hl], "little") >> (3 if hl == 1 else 4)
            q = hl + (regen if ltype == 0 else 1)
        else:
            hl, nb = (3, 10) if sf < 2 else ((4, 14) if sf == 2 else (5, 18))
            v = int.from_bytes(p[:hl], "little") >> 4
            q = hl + ((v >> nb) & ((1 << nb) - 1))
            items.add("streams:%d" % (1 if sf == 0 else 4))
        n = p[q]
        q += 1 if n < 128 else (2 if n < 255 else 3)
        if n:
            m = p[q]
            for k, t in enumerate(("ll", "of", "ml")):
                items.add("%s:%s" % (t, ("predefined", "rle", "fse", "repeat")[(m >> (6 - 2 * k)) & 3]))
    return items


# ------------------------------------------------------------------------------------------------ the fixture's payloads

_WORDS = None


def payload(gen, seed, n):
    """the payload a recipe (generator name, seed, length) stands for"""
    global _WORDS
    rs = _rs(seed)
    if gen == "zeros":
        return bytes(n)
    if gen == "text":
        return (b"the quick brown fox jumps over the lazy dog, 0123456789; " * (n // 57 + 1))[:n]
    if gen == "prose":
        if _WORDS is None:
            w = _rs(99)
            _WORDS = [bytes(w.randint(97, 123, size=w.randint(2, 10)).astype(np.uint8)) for _ in range(300)]
        out, size = [], 0
        idx = rs.randint(0, 300, size=n // 2 + 2)
        for i in idx:
            out.append(_WORDS[i])
            size += len(_WORDS[i]) + 1
            if size >= n:
                break
        return b" ".join(out)[:n].ljust(n, b".")
    if gen == "runs":
        vals, lens = rs.randint(0, 256, size=n), rs.randint(1, 300, size=n)
        out, size = [], 0
        for v, k in zip(vals, lens):
            out.append(bytes([v]) * int(k))
            size += int(k)
            if size >= n:
                break
        return b"".join(out)[:n]
    if gen == "random":
        return rs.bytes(n)
    if gen == "svb":
        from sigtk_amd import blow5
        sig = 500 + np.cumsum(rs.randint(-30, 31, size=n)) % 700 + rs.randint(-8, 9, size=n)
        return blow5.svb_zd_encode(sig.astype(np.int16))
    raise ValueError(gen)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    """tests/golden/zstd_frames.npz -> [(name, frame, payload or None for the frame the decoders must refuse, flags)]:
    the payloads are regenerated from their recipes and checked against the recorded length and CRC-32"""
    z = np.load(os.path.join(GOLDEN, "zstd_frames.npz"))
    blob, offs = z["frames"].tobytes(), z["frame_offsets"]
    cache, out = {}, []
    for k in range(len(z["gen"])):
        gen, seed, n, level, flags = str(z["gen"][k]), int(z["seed"][k]), int(z["n"][k]), int(z["level"][k]), str(z["flags"][k])
        key = (gen, seed, n)
        if key not in cache:
            cache[key] = payload(gen, seed, n)
        data = cache[key]
        assert len(data) == int(z["length"][k]) and zlib.crc32(data) == int(z["crc32"][k]), ("payload recipe drifted", key)
        name = "%s_%d_level%d%s" % (gen, n, level, "_" + flags if flags else "")
        out.append((name, blob[int(offs[k]):int(offs[k + 1])], None if flags == "nosize" else data, flags))
    return out


def mutations(frames, count, seed):
    """`count` seeded mutations of the given frames: bit flips, truncations, overwritten spans -> [(name, bytes)]"""
    rs = _rs(seed)
    out = []
    for it in range(count):
        src = frames[int(rs.randint(len(frames)))]
        d = bytearray(src)
        kind = it % 3
        if kind == 0:
            for _ in range(int(rs.randint(1, 4))):
                d[int(rs.randint(len(d)))] ^= 1 << int(rs.randint(8))
        elif kind == 1:
            d = d[:int(rs.randint(1, len(d)))]
        else:
            i = int(rs.randint(4, max(5, len(d) - 4)))
            k = int(rs.randint(1, 9))
            d[i:i + k] = rs.bytes(k)[:max(0, min(k, len(d) - i))]
        out.append(("mut%d_%s" % (it, ("flip", "cut", "span")[kind]), bytes(d)))
    return out


def recode_blow5(src, dst, press, compress):
    """the records of BLOW5 file `src` with an svb-zd signal, each compressed with compress(bytes) -> bytes, written to
    `dst` with record compression byte `press` and signal compression byte 1 (file version at least 0.2.0)"""
    from sigtk_amd import blow5
    buf = open(src, "rb").read()
    version, rpress = tuple(buf[6:9]), buf[9]
    spress = buf[14] if version >= (0, 2, 0) else 0
    (hsize,) = struct.unpack_from("<I", buf, 64)
    head = bytearray(buf[:68 + hsize])
    if version < (0, 2, 0):
        head[6:9] = bytes((0, 2, 0))
    head[9], head[14] = press, 1
    pos, out = 68 + hsize, [bytes(head)]
    while buf[pos:pos + 5] != blow5.EOF_MARK or pos + 5 != len(buf):
        (size,) = struct.unpack_from("<Q", buf, pos)
        rec = buf[pos + 8:pos + 8 + size]
        pos += 8 + size
        if rpress == 1:
            rec = zlib.decompress(rec)
        (idl,) = struct.unpack_from("<H", rec, 0)
        p = 2 + idl + 36
        (ln,) = struct.unpack_from("<Q", rec, p)
        if spress == 0:
            sig = blow5.svb_zd_encode(np.frombuffer(rec, dtype="<i2", count=ln, offset=p + 8))
            rec = rec[:p] + struct.pack("<Q", len(sig)) + sig + rec[p + 8 + 2 * ln:]
        c = compress(bytes(rec))
        out.append(struct.pack("<Q", len(c)) + c)
    out.append(blow5.EOF_MARK)
    open(dst, "wb").write(b"".join(out))
