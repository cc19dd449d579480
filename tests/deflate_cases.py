"""The inputs of the deflate tests (tests/test_deflate_proto.py on the CPU model, tests/test_gpu_deflate.py on k_deflate):
the smallest at which each piece of the compressor can go wrong.  B is the compressor's block size."""
import functools
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fibonacci_block(block: int) -> bytes:
    """byte value i repeated F(i) times, i = 1 .. 18 (6 764 bytes; 17 terms, 4 180 bytes, for a smaller block), in a
    seeded random order without equal neighbours: value by value, rarest first, each value's copies go into distinct
    gaps of what is there, drawn with a fixed seed.  With no runs the literal counts are the Fibonacci numbers
    themselves (and 1 for the end of block): an unlimited Huffman code reaches 17 - 18 bits (the test checks that)."""
    terms = 18 if block >= 6764 else 17
    f = [1, 1]
    while len(f) < terms:
        f.append(f[-1] + f[-2])
    rs = np.random.RandomState(1951)
    seq = np.zeros(0, dtype=np.uint8)
    for i in range(1, terms + 1):
        k = f[i - 1]
        gaps = np.sort(rs.choice(seq.size + 1, size=k, replace=False))
        seq = np.insert(seq, gaps, np.uint8(i))
    assert seq.size == sum(f) and not (seq[1:] == seq[:-1]).any()
    return seq.tobytes()


def svb_bytes(n: int) -> bytes:
    """n bytes of svb-zd data: the signal blob of read 0 of the fixture (5 947 bytes), repeated to the length"""
    blob = _svb_blob()
    return (blob * (n // len(blob) + 1))[:n]


@functools.lru_cache(maxsize=None)
def _svb_blob() -> bytes:
    from sigtk_amd import blow5
    return blow5.read_signal_blobs(os.path.join(GOLDEN, "sp1_dna.blow5"))[0][1]


def cases(block: int):
    """-> dict name -> bytes"""
    B = block
    rs = np.random.RandomState(1950)
    out = {}
    for n in (0, 1, 2, 3):
        out["same%d" % n] = b"\x55" * n
    for n in (3, 4, 258, 259, 260, 261, 262, 517):
        out["run%d" % n] = b"a" + b"\x00" * n + b"b"
    out["run_from_lane_byte_15"] = bytes(range(1, 16)) + b"\xee" * 40 + b"z"
    out["run_over_tile_end"] = bytes(rs.randint(1, 250, size=1000).astype(np.uint8)) + b"\xfa" * 300 + b"tail"
    out["run_over_block_end"] = svb_bytes(B - 7) + b"\xfb" * 20 + b"tail"
    for name, n in (("svb_B-1", B - 1), ("svb_B", B), ("svb_B+1", B + 1), ("svb_2B+1", 2 * B + 1)):
        out[name] = svb_bytes(n)
    flat = np.tile(np.arange(256, dtype=np.uint8), B // 256)
    rs.shuffle(flat)
    flat[1:][flat[1:] == flat[:-1]] ^= 0x80   # (most equal neighbours broken up; the counts stay equal but for a few)
    out["flat"] = np.tile(np.arange(256, dtype=np.uint8), B // 256).tobytes()   # every value equally often, no runs
    out["flat_shuffled"] = flat.tobytes()
    out["two_values"] = bytes([0, 1]) * (B // 2)
    out["pairs"] = bytes([7, 7, 9]) * (B // 3)
    out["fibonacci"] = fibonacci_block(B)
    out["random70000"] = rs.bytes(70000)
    out["zeros100000"] = bytes(100000)
    return out


# ---- the edge inputs: off the aligned path and at the decision edges (tests/test_deflate_edges_cpu.py,
# tests/test_gpu_deflate_edges.py).  Background bytes never repeat a neighbour and never equal a run's byte.
RUN_BYTE = 0xEE
RUN_STARTS = (0, 1, 14, 15, 16, 17, 1007, 1008, 1022, 1023, 1024, 1025)
RUN_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 257, 258, 259, 260, 261, 262, 516, 517, 518, 775, 1024, 1025, 1291, 2049, 2323)
EDGE_GROUPS = ("run", "end", "staircase", "len", "even", "hclen", "cl", "high")


def _model():
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto")
    if p not in sys.path:
        sys.path.insert(0, p)
    import deflate_proto
    return deflate_proto


def background(n: int, seed: int, values=tuple(range(0x10, 0x18))) -> bytes:
    """n bytes drawn from `values` with a fixed seed, no two neighbours equal (any slice of it is such a string too)"""
    x = np.random.RandomState(seed).randint(0, len(values), size=n).tolist()
    for i in range(1, n):
        if x[i] == x[i - 1]:
            x[i] = (x[i] + 1) % len(values)
    return bytes(values[v] for v in x)


def spread(groups):
    """groups: [(value, count)] -> all of them in one list without equal neighbours: the most frequent first, over the
    even places and then the odd ones (no count may exceed half the total, rounded up)"""
    groups = sorted(groups, key=lambda g: (-g[1], g[0]))
    n = sum(c for _, c in groups)
    assert groups[0][1] <= (n + 1) // 2
    flat = [v for v, c in groups for _ in range(c)]
    out = [None] * n
    out[0::2] = flat[:(n + 1) // 2]
    out[1::2] = flat[(n + 1) // 2:]
    return out


def dyadic_block():
    """16 383 bytes without runs whose literal counts are 2^(14 - length) for a set of 257 code lengths (the end of block
    has 14) that no two neighbouring symbols share: the Huffman code has exactly these lengths, the header no 16, and the
    code length code sees one count per length.  The lengths come from a seeded walk (split one code into two of the next
    length, merge two elsewhere: 257 codes and a full Kraft sum stay) that keeps a step unless an unlimited Huffman code
    over the counts gets shallower, until that code is 9 deep: two bits beyond what the header can carry."""
    dp = _model()

    def depth(n):
        return max(dp.build_lengths([1] + n[1:15] + [0] * 4, 30))   # (a single 0: the distance length)

    rs = np.random.RandomState(0)
    n = [0] + [1] * 13 + [2]
    while sum(n) < 257:
        k = int(rs.randint(1, 14))
        if n[k] > 0:
            n[k] -= 1
            n[k + 1] += 2
    d = depth(n)
    while d < 9:
        m = list(n)
        a, b = int(rs.randint(1, 14)), int(rs.randint(1, 14))
        if m[a] < 1:
            continue
        m[a] -= 1
        m[a + 1] += 2
        if m[b + 1] < 2:
            continue
        m[b + 1] -= 2
        m[b] += 1
        if m[14] < 1 or depth(m) < d:
            continue
        n, d = m, depth(m)
    assert sum(n) == 257 and sum(n[k] << (14 - k) for k in range(1, 15)) == 1 << 14
    lens = spread([(k, n[k] - (1 if k == 14 else 0)) for k in range(1, 15) if n[k]])   # byte values 0 .. 255
    assert lens[255] != 14
    data = spread([(v, 1 << (14 - k)) for v, k in enumerate(lens)])
    assert len(data) == (1 << 14) - 1
    return bytes(data)


def _near_even(block: int):
    """-> {(pos, margin): bytes}: a first block of `block` svb bytes, dynamic, behind which the second block starts at bit
    `pos` of its byte, and a second block -- about a tile of random bytes and a run -- whose dynamic form has `margin`
    bits more than its stored form from there.  Found with the model, in a fixed order from fixed seeds."""
    dp = _model()
    pad = lambda pos: (-(pos + 3)) % 8
    want = sorted({pad(pos) + m for pos in range(8) for m in (-1, 0, 1)})   # dynamic bits - 8 n - 35 of the second block
    second = {}
    seed = 0
    while len(second) < len(want):
        assert seed < 2000
        x = np.random.RandomState(5000 + seed).randint(0, 256, size=1000 + 7 * (seed % 8)).tolist()
        for i in range(len(x)):
            while x[i] == RUN_BYTE or (i and x[i] == x[i - 1]):
                x[i] = (x[i] + 1) % 256
        head = bytes(x)
        d0 = dp.plan_block(np.frombuffer(head, dtype=np.uint8))["bits"] - 8 * len(head) - 35
        for run in range(d0 // 8 + 2, d0 // 8 + 16):   # (a match token and its code cost some 80 bits)
            cand = head + bytes([RUN_BYTE]) * run
            d = dp.plan_block(np.frombuffer(cand, dtype=np.uint8))["bits"] - 8 * len(cand) - 35
            if d in want and d not in second:
                second[d] = cand
        seed += 1
    first = {}
    rep = _svb_blob() * (block // len(_svb_blob()) + 2)
    o = 0
    while len(first) < 8:
        assert o < len(_svb_blob())
        cand = rep[o:o + block]
        bits = dp.plan_block(np.frombuffer(cand, dtype=np.uint8))["bits"]
        if bits < 35 + 5 + 8 * block:
            first.setdefault((16 + bits) & 7, cand)
        o += 1
    return {(pos, m): first[pos] + second[pad(pos) + m] for pos in range(8) for m in (-1, 0, 1)}


@functools.lru_cache(maxsize=None)
def edge_cases(block: int):
    """-> dict name -> bytes (the same object for every caller: do not change it); the name's first word is its group"""
    B = block
    run = bytes([RUN_BYTE])
    bg = background(B + 512, 1951)
    out = {}
    # a run of every length from every start: lane, tile and chunk boundaries under its start, its end and its chunks
    for s in RUN_STARTS:
        for n in RUN_LENGTHS:
            out["run_s%d_L%d" % (s, n)] = bg[:s] + run * n + bg[s:s + 64]
    # runs that end with the block (the last chunk 1, 2, 3, 4 and 258 bytes), as the stream's end and with more behind
    for n in (259, 260, 261, 262, 516):
        assert (n - 1) % 258 in (0, 1, 2, 3, 257)
        out["end_L%d_last" % n] = bg[:B - n] + run * n
        out["end_L%d_more" % n] = bg[:B - n] + run * n + bg[B - n:B - n + 64]
    # ... and runs that cross it
    for k in (1, 2, 3, 4, 259):
        for j in (1, 2, 3, 4, 300):
            out["end_cross_k%d_j%d" % (k, j)] = bg[:B - k] + run * (k + j) + bg[B - k:B - k + 64]
    out["staircase"] = b"".join(bytes([k]) * k for k in range(1, 21))
    for n in list(range(0, 1057)) + list(range(B - 20, B + 21)):
        out["len_%d" % n] = svb_bytes(n)
    for (pos, m), x in _near_even(B).items():
        out["even_pos%d_m%+d" % (pos, m)] = x
    out["hclen_four"] = bytes([0x31, 0x32, 0x33, 0x34]) * 300
    out["hclen_eight"] = bytes(range(0x41, 0x49)) * 200
    out["hclen_two_symbols"] = b"\x07" + b"\x09" * 3000
    out["cl_limit_dyadic"] = dyadic_block()
    out["high_ff_fe"] = bytes([255, 254]) * (B // 2)
    out["high_ff_5000"] = b"\xff" * 5000
    assert all(k.split("_")[0] in EDGE_GROUPS for k in out)
    return out
