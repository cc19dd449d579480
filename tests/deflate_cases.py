"""The inputs of the deflate tests (tests/test_deflate_proto.py on the CPU model, tests/test_gpu_deflate.py on k_deflate):
the smallest at which each piece of the compressor can go wrong.  B is the compressor's block size."""
import os

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
    from sigtk_amd import blow5
    blob = blow5.read_signal_blobs(os.path.join(GOLDEN, "sp1_dna.blow5"))[0][1]
    return (blob * (n // len(blob) + 1))[:n]


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
