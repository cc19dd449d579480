"""CPU: tools/proto/deflate_proto.py -- the model of k_deflate's output -- judged by zlib: every input of
tests/deflate_cases.py inflates back, stays under sgk_deflate_bound (a host function of the library: no GPU), and the
Fibonacci block exercises the 15-bit limit of the literal/length code."""
import ctypes
import os
import sys
import zlib

import pytest

import deflate_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import deflate_proto  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from sigtk_amd import api
    return api.load_library()


@pytest.fixture(scope="module")
def block(lib):
    b = int(lib.sgk_deflate_block_bytes())
    assert b >= 4181
    return b


def test_bound_is_the_all_stored_size(lib, block):
    per = min(block, 65535)
    for n in (0, 1, per - 1, per, per + 1, 70000, 10 ** 9, 2 ** 40):
        assert int(lib.sgk_deflate_bound(n)) == n + 5 * max(1, -(-n // per)) + 6
        assert deflate_proto.deflate_bound(n, block) == int(lib.sgk_deflate_bound(n))


def test_model_streams_inflate_and_stay_under_the_bound(lib, block):
    for name, x in deflate_cases.cases(block).items():
        z = deflate_proto.deflate(x, block)
        assert zlib.decompress(z) == x, name
        assert len(z) <= int(lib.sgk_deflate_bound(len(x))), name
        assert z[:2] == b"\x78\x9c", name


def test_model_block_types_and_sizes(block):
    cs = deflate_cases.cases(block)
    info = []
    z = deflate_proto.deflate(cs["random70000"], block, info=info)
    assert all(b["type"] == "stored" for b in info) and len(z) <= 70000 + 5 * len(info) + 6
    z = deflate_proto.deflate(cs["zeros100000"], block)
    assert len(z) < 100000 // 64                    # Huffman codes alone cannot go below n / 8: the runs are coded
    info = []
    deflate_proto.deflate(cs["flat"], block, info=info)
    # (8 bits and a little per byte: the block goes out stored; its dynamic form is what is looked at here)
    assert set(info[0]["lens"][:257]) <= {8, 9} and info[0]["type"] == "stored"
    info = []
    deflate_proto.deflate(cs["run_over_block_end"], block, info=info)
    assert len(info) == 2 and info[1]["has_match"]   # the run is cut at the block's end and goes on behind it
    for n, want in ((3, 0), (4, 1), (258, 1), (259, 1), (260, 1), (261, 1), (262, 2), (517, 2)):
        info = []
        z = deflate_proto.deflate(cs["run%d" % n], block, info=info)
        assert int(info[0]["ism"].sum()) == want, n


def test_fibonacci_block_hits_the_length_limit(block):
    x = deflate_cases.fibonacci_block(block)
    info = []
    z = deflate_proto.deflate(x, block, info=info)
    assert zlib.decompress(z) == x
    assert len(info) == 1 and info[0]["type"] == "dynamic"
    freq = [0] * 286
    for s in info[0]["sym"]:
        freq[int(s)] += 1
    freq[256] = 1
    assert max(deflate_proto.build_lengths(freq, 30)) > 15      # what an unlimited code would need
    lens = info[0]["lens"]
    assert max(lens) == 15
    assert sum(2.0 ** -v for v in lens if v) == 1.0             # the repaired code is complete
