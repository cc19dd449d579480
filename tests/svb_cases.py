"""The inputs of the svb-zd codec tests (tests/test_svb_cases_cpu.py here, tests/test_gpu_svb_cases.py on k_svbzd_decode,
k_svbzd_size and k_svbzd_encode) and a plain serial codec to compare with.  No GPU, no torch.

Format (include/sigtk_gpu.h, header of sigtk_amd/csrc/svb_kernels.hip): u32 count | ceil(count / 4) key bytes, value j of
a key byte at bits 2 * (j % 4), a 2-bit code c standing for c + 1 little-endian data bytes | the data bytes.  A value is
zigzag(delta) against the sample before it (0 before the first); a sample is the low 16 bits of the running sum.

Every case says where it lies: `blob_lead` bytes behind a 16-byte boundary, `sample_lead` samples behind a 64-sample
boundary.  The shapes are the smallest that reach each path of the kernels: tiles of 1024 values (64 lanes x 16)."""
import functools
import struct
from dataclasses import dataclass

import numpy as np

TILE = 1024
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1008, 1023, 1024, 1025, 1039, 1040, 2048, 2049, 3077)
DECODE_SAMPLE_LEADS = (0, 1, 4, 7)
ENCODE_SAMPLE_LEADS = (0, 1, 3, 4, 7)
ENCODE_BLOB_LEADS = (0, 4, 8, 12)

# what the malformed kinds must give (include/sigtk_gpu.h; where 1 and 2 both apply either may be reported, never 0)
MALFORMED_STATUS = {
    "short_blob": (1,), "count_mismatch": (1,), "cut_in_keys": (2,), "len4_count5": (2,), "data_short_1": (2,),
    "data_short_2": (2,), "data_short_tile": (2,), "data_short_second_tile": (2,), "left_over_single": (2,),
    "left_over_multi": (2,), "count0_len4": (0,), "count0_len5": (2,), "count_wrap": (1, 2),
}


# ---------------------------------------------------------------------- the plain codec

def ref_rules(blob, expected_count):
    """-> (the statuses whose rule applies, as a sorted tuple; int16 samples if none does, else None).  One byte cursor
    and one running sum.  Rule 1: fewer than 4 bytes, or the count word is not expected_count.  Rule 2: fewer bytes than
    4 + ceil(count / 4); data shorter than the keys promise; data bytes left over."""
    blob = bytes(blob)
    if len(blob) < 4:
        return (1,), None
    count = int.from_bytes(blob[0:4], "little")
    rules = set()
    if count != expected_count:
        rules.add(1)
    nkeys = (count + 3) // 4
    if len(blob) < 4 + nkeys:
        rules.add(2)
        return tuple(sorted(rules)), None
    out = np.empty(count, dtype=np.int16)
    cur = 4 + nkeys
    prev = 0
    for i in range(count):
        n = ((blob[4 + (i >> 2)] >> (2 * (i & 3))) & 3) + 1
        if cur + n > len(blob):
            rules.add(2)
            return tuple(sorted(rules)), None
        v = int.from_bytes(blob[cur:cur + n], "little")
        cur += n
        prev += (v >> 1) ^ -(v & 1)          # exact integer sum
        low = prev & 0xFFFF
        out[i] = low - 0x10000 if low & 0x8000 else low
    if cur != len(blob):
        rules.add(2)
    if rules:
        return tuple(sorted(rules)), None
    return (), out


def ref_decode(blob, expected_count):
    """-> (status, int16 array or None): 0 and the samples, or the first rule that applies (ref_rules has them all)"""
    rules, out = ref_rules(blob, expected_count)
    return (rules[0], None) if rules else (0, out)


def ref_encode(samples) -> bytes:
    """the canonical blob: every value in the fewest bytes"""
    x = [int(v) for v in np.asarray(samples, dtype=np.int16)]
    keys = bytearray((len(x) + 3) // 4)
    data = bytearray()
    prev = 0
    for i, s in enumerate(x):
        d = s - prev
        prev = s
        z = (d << 1) if d >= 0 else ((-d << 1) - 1)
        code = (z > 0xFF) + (z > 0xFFFF) + (z > 0xFFFFFF)
        keys[i >> 2] |= code << (2 * (i & 3))
        data += z.to_bytes(code + 1, "little")
    return struct.pack("<I", len(x)) + bytes(keys) + bytes(data)


def key_codes(blob) -> np.ndarray:
    """the 2-bit codes of a blob whose keys are all there, read from its own bytes"""
    count = int.from_bytes(blob[0:4], "little")
    keys = np.frombuffer(blob, dtype=np.uint8, count=(count + 3) // 4, offset=4)
    return ((keys[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)[None, :]) & 3).reshape(-1)[:count].astype(np.int64)


def pack_u32(values, codes=None, pad_ones=False, count_word=None) -> bytes:
    """a blob of generic u32 values; codes: the code of each (default: the shortest), pad_ones: the unused bits of the
    last key byte are set; count_word: written in place of len(values)"""
    values = [int(v) for v in values]
    if codes is None:
        codes = [(v > 0xFF) + (v > 0xFFFF) + (v > 0xFFFFFF) for v in values]
    keys = bytearray((len(values) + 3) // 4)
    data = bytearray()
    for i, (v, c) in enumerate(zip(values, codes)):
        assert v < 1 << (8 * (int(c) + 1))
        keys[i >> 2] |= int(c) << (2 * (i & 3))
        data += v.to_bytes(int(c) + 1, "little")
    if pad_ones and len(values) % 4:
        keys[-1] |= (0xFF << (2 * (len(values) % 4))) & 0xFF
    return struct.pack("<I", len(values) if count_word is None else count_word) + bytes(keys) + bytes(data)


def full_width(codes, rs) -> list:
    """a value for every code that uses the code's whole width: random low bytes, a non-zero top byte"""
    out = []
    for c in codes:
        c = int(c)
        low = int(rs.randint(0, 1 << 30)) & ((1 << (8 * c)) - 1)
        out.append(low | (int(rs.randint(1, 256)) << (8 * c)))
    return out


# ---------------------------------------------------------------------- cases

@dataclass(frozen=True)
class DecodeCase:
    name: str
    blob: bytes
    expected_count: int
    blob_lead: int          # 0 - 15
    sample_lead: int        # 0 - 7
    status: tuple = (0,)    # the statuses the decoder may give
    kind: str = ""          # malformed cases: a key of MALFORMED_STATUS


@dataclass(frozen=True)
class EncodeCase:
    name: str
    samples: np.ndarray     # int16
    sample_lead: int
    blob_lead: int          # 0, 4, 8 or 12


def _walk(rs, n, wide=0.1):
    """a signal-like read: mostly 1-byte deltas, a share of `wide` 2-byte ones, kept inside int16"""
    d = rs.randint(-60, 61, size=n).astype(np.int64)
    m = rs.rand(n) < wide
    d[m] = rs.randint(-3000, 3001, size=int(m.sum()))
    x = np.cumsum(d)
    return (((x + 20000) % 40000) - 20000).astype(np.int16) if n else np.zeros(0, dtype=np.int16)


@functools.lru_cache(maxsize=None)
def encode_cases():
    out = []

    def add(name, samples, i):
        x = np.asarray(samples, dtype=np.int64)
        assert x.size == 0 or (-32768 <= x.min() and x.max() <= 32767), name
        out.append(EncodeCase(name, x.astype(np.int16), ENCODE_SAMPLE_LEADS[i % 5], ENCODE_BLOB_LEADS[(i // 5 + i) % 4]))

    # every length at every sample lead and every blob lead
    for i, n in enumerate(LENGTHS):
        for j, sl in enumerate(ENCODE_SAMPLE_LEADS):
            for bl in ENCODE_BLOB_LEADS:
                rs = np.random.RandomState(70000 + 32 * i + 4 * j + bl // 4)
                out.append(EncodeCase("len%d_s%d_b%d" % (n, sl, bl), _walk(rs, n), sl, bl))
    # every (key bytes % 4, data bytes % 4): 1-byte deltas and as many 2-byte ones as steer the data length; in the
    # multi-tile form t1 of them lie in tile 1, so that (key bytes + data bytes of tile 1) % 4, the bytes carried into
    # tile 2, is (k + d) % 4: all four values
    i = 0
    for k in range(4):
        for d in range(4):
            for multi in (False, True):
                nkeys = (260 if multi else 8) + k
                n = 4 * nkeys - 2
                rs = np.random.RandomState(7400 + 8 * k + 2 * d + multi)
                delta = rs.randint(-60, 61, size=n).astype(np.int64)
                t1 = d if multi else (d - n) % 4
                t2 = (d - n - t1) % 4 if multi else 0
                for p in list(3 + 37 * np.arange(t1)) + list(TILE + 2 + 5 * np.arange(t2)):
                    delta[int(p) % n if not multi else int(p)] = 300
                x = np.cumsum(delta)
                assert np.abs(x).max() < 32000
                add("pair_k%d_d%d_%s" % (k, d, "multi" if multi else "single"), x, i)
                i += 1
    # n = 1, 2, 3 all of one code: the whole blob is less than a dword or little more (no int16 sample is 3 bytes away
    # from 0, so the 3-byte form starts with a 1-byte code and n = 1 has none)
    for n in (1, 2, 3):
        add("tiny%d_code0" % n, 5 * np.arange(1, n + 1), i)
        add("tiny%d_code1" % n, 300 * np.arange(1, n + 1), i + 1)
        if n > 1:
            add("tiny%d_code2" % n, [-1, 32767, -2][:n], i + 2)
        i += 3
    # deltas at the edges of the code lengths: zigzag 254 | 255 | 256 | 257, 65534 | 65535 | 65536 | 65537, and the
    # largest an int16 pair has
    for dlt in (-128, 127, 128, -129, -32768, 32767):
        add("first_delta%d" % dlt, [dlt, dlt, 7, 7, 7], i)
        i += 1
    for dlt, base in ((-128, 100), (127, 100), (128, 100), (-129, 100), (-32768, 0), (32767, 0), (32768, -1), (-32769, 1),
                      (65535, -32768), (-65535, 32767)):
        x = np.full(20, base, dtype=np.int64)
        x[7:] = base + dlt
        x[12:] = 3
        add("mid_delta%d" % dlt, x, i)
        i += 1
    # a large jump exactly at a lane seam (16 k, 16 k - 1) and at a tile seam (1024 k, 1024 k - 1)
    for idx in (15, 16, 31, 32, 1007, 1008, 1023, 1024, 2047, 2048):
        n = 70 if idx < 64 else idx + 40
        x = _walk(np.random.RandomState(7600 + idx), n, wide=0.0).astype(np.int64) // 4 - 20000
        x[idx:] += 45000
        add("jump_at%d" % idx, x, i)
        i += 1
    add("constant", np.full(1040, 1234), i)
    add("alternating_extremes", np.where(np.arange(1040) % 2 == 0, -32768, 32767), i + 1)
    add("ramp", 13 * np.arange(2049) - 13000, i + 2)
    add("random_full_range", np.random.RandomState(7700).randint(-32768, 32768, size=3077), i + 3)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def decode_cases():
    """the valid blobs (status 0)"""
    out = []

    def add(name, blob, blob_lead, sample_lead):
        out.append(DecodeCase(name, blob, int.from_bytes(blob[0:4], "little"), blob_lead % 16, sample_lead))

    # alignment: every blob_lead % 4 x key bytes % 4 at every sample lead; the two larger sample leads are multi-tile
    for bl4 in range(4):
        for nk4 in range(4):
            for j, sl in enumerate(DECODE_SAMPLE_LEADS):
                nkeys = (20, 4, 260, 516)[j] + nk4
                n = 4 * nkeys - (bl4 + j) % 4
                rs = np.random.RandomState(8000 + 16 * bl4 + 4 * nk4 + j)
                vals = full_width(rs.randint(0, 4, size=n), rs)
                add("align_b%d_k%d_s%d_n%d" % (bl4, nk4, sl, n), pack_u32(vals), bl4 + 4 * ((nk4 + j) % 4), sl)
    # one code throughout a full tile; the 4-byte ones also where the data starts 3 bytes behind a dword (the most the
    # staged tile can hold) and with a second tile behind them
    rs = np.random.RandomState(8300)
    for c in range(4):
        add("all_code%d_tile" % c, pack_u32(full_width([c] * TILE, rs)), 4 * c, DECODE_SAMPLE_LEADS[c])
    add("all_code3_tile_shift3", pack_u32(full_width([3] * TILE, rs)), 3, 1)
    add("all_code3_tile_shift3_lead15", pack_u32(full_width([3] * TILE, rs)), 15, 0)
    add("all_code3_two_tiles", pack_u32(full_width([3] * (TILE + 17), rs)), 6, 4)
    add("all_code3_two_tiles_shift3", pack_u32(full_width([3] * (2 * TILE), rs)), 11, 7)
    for phase in range(4):
        add("codes_phase%d" % phase, pack_u32(full_width((np.arange(1040) + phase) % 4, rs)), 5 * phase, DECODE_SAMPLE_LEADS[phase])
    # one 4-byte value among 1-byte ones: every slot of lanes 0, 31 and 63 and the first two of tile 2
    for p in list(range(16)) + list(range(496, 512)) + list(range(1008, 1024)) + [1024, 1025]:
        codes = [0] * 1026
        codes[p] = 3
        add("one_code3_at%d" % p, pack_u32(full_width(codes, rs)), p % 16, DECODE_SAMPLE_LEADS[(p // 4) % 4])
    add("random_codes", pack_u32(full_width(rs.randint(0, 4, size=3077), rs)), 9, 1)
    special = [0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 1, 0x80000001, 0xFFFFFFFF, 0, 0x7FFFFFFF, 0xFFFFFFFE, 0x80000000]
    for bl in range(4):
        add("special_values_b%d" % bl, pack_u32(special[bl:] + special[:bl]), bl, DECODE_SAMPLE_LEADS[bl])
    # the running sum leaves int32 (three deltas of 2^31 - 1, then more): the samples are the low 16 bits of the exact sum
    add("sum_leaves_int32", pack_u32([0xFFFFFFFE] * 5 + [77, 0xFFFFFFFD] * 6 + [0xFFFFFFFE] * 9), 2, 1)
    # counts that are no multiple of 4 with the unused bits of the last key byte set: they must be ignored
    for j, n in enumerate((1, 2, 3, 5, 17, 1023, 1025, 1038)):
        add("pad_bits_set_n%d" % n, pack_u32(full_width(rs.randint(0, 3, size=n), rs), pad_ones=True), 5 * j, DECODE_SAMPLE_LEADS[j % 4])
    # what the encoder's cases encode to, off the encoder's own alignment
    for i, c in enumerate(encode_cases()):
        add("enc:" + c.name, ref_encode(c.samples), (5 * i + 1) % 16, (0, 1, 4, 7, 2, 3, 5, 6)[i % 8])
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """blobs the decoder must refuse (and count 0 in 4 bytes, which it must not), each with one defect but for count_wrap"""
    out = []

    def add(kind, name, blob, expected, i):
        out.append(DecodeCase("bad:" + name, bytes(blob), expected, (7 * i + 1) % 16, (3 * i) % 8, MALFORMED_STATUS[kind], kind))

    rs = np.random.RandomState(9000)
    b17 = pack_u32(full_width(rs.randint(0, 4, size=17), rs))
    b1025 = pack_u32(full_width(rs.randint(0, 3, size=1025), rs))
    b2049 = pack_u32(full_width(rs.randint(0, 3, size=2049), rs))
    i = 0
    for n in range(4):
        add("short_blob", "length%d" % n, b17[:n], 17, i); i += 1
    add("count_mismatch", "count17_expected18", b17, 18, i); i += 1
    add("count_mismatch", "count17_expected16", b17, 16, i); i += 1
    add("count_mismatch", "count1025_expected1024", b1025, 1024, i); i += 1
    add("count_mismatch", "count0_expected17", struct.pack("<I", 0), 17, i); i += 1
    add("count_mismatch", "count17_expected0", b17, 0, i); i += 1
    for n in range(4, 9):   # 17 values have 5 key bytes: 0 to 4 of them left
        add("cut_in_keys", "count17_length%d" % n, b17[:n], 17, i); i += 1
    add("len4_count5", "count5_length4", struct.pack("<I", 5), 5, i); i += 1
    add("data_short_1", "count17_short1", b17[:-1], 17, i); i += 1
    add("data_short_1", "count1024_short1", pack_u32(full_width([1] * TILE, rs))[:-1], TILE, i); i += 1
    add("data_short_2", "count17_short2", b17[:-2], 17, i); i += 1
    add("data_short_tile", "count2049_short_a_tile", b2049[:-int((key_codes(b2049)[TILE:2 * TILE] + 1).sum())], 2049, i); i += 1
    add("data_short_second_tile", "count1025_short1", b1025[:-1], 1025, i); i += 1
    for n in range(1, 5):
        add("left_over_single", "count17_plus%d" % n, b17 + b"\x00\x01\x02\x03"[:n], 17, i); i += 1
        add("left_over_multi", "count1025_plus%d" % n, b1025 + b"\xff\x00\x00\x00"[:n], 1025, i); i += 1
    add("count0_len4", "count0_length4", struct.pack("<I", 0), 0, i); i += 1
    add("count0_len5", "count0_length5", struct.pack("<I", 0) + b"\x00", 0, i); i += 1
    for w in (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF):   # (count + 3) / 4 wraps in 32 bits
        add("count_wrap", "count_word_%08x" % w, struct.pack("<I", w) + b17[4:], 17, i); i += 1
        add("count_wrap", "count_word_%08x_length4" % w, struct.pack("<I", w), 1, i); i += 1
    assert len({c.name for c in out}) == len(out)
    assert {c.kind for c in out} == set(MALFORMED_STATUS)
    return tuple(out)


def first_tile_data_bytes(blob) -> int:
    """data bytes of the first 1024 values, from the blob's keys"""
    return int((key_codes(blob)[:TILE] + 1).sum())
