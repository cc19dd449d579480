"""CPU: the model of k_deflate (tools/proto/deflate_proto.py) before an independent judge (tests/deflate_parse.py): every
stream it writes for tests/deflate_cases.py's cases() and edge_cases() is read bit by bit and held against the format --
tokens, header fields, complete and optimal codes, the greedy code length items, the choice between the two block forms.
Then the judge is judged: six wrong tokenizers and choosers, each caught at a named input; and every property the edge
inputs were made for is shown to fire."""
import os
import sys
import zlib

import numpy as np
import pytest

import deflate_cases
import deflate_parse as dz

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import deflate_proto  # noqa: E402


def plan_of(piece: bytes):
    return deflate_proto.plan_block(np.frombuffer(piece, dtype=np.uint8))


@pytest.fixture(scope="module")
def B():
    from sigtk_amd import api
    return int(api.load_library().sgk_deflate_block_bytes())


@pytest.fixture(scope="module")
def streams(B):
    """name -> (input, the model's stream, the model's info per block), cases() and edge_cases() together"""
    out = {}
    for name, x in list(deflate_cases.cases(B).items()) + list(deflate_cases.edge_cases(B).items()):
        assert name not in out
        info = []
        out[name] = (x, deflate_proto.deflate(x, B, info=info), info)
    return out


@pytest.fixture(scope="module")
def judged(streams, B):
    """name -> (check_stream's parse, block_choice's list): every stream passes both"""
    out = {}
    for name, (x, z, info) in streams.items():
        try:
            out[name] = (dz.check_stream(z, x, B), dz.block_choice(z, x, B, plan_of))
        except (AssertionError, dz.FormatError) as e:
            raise AssertionError("%s: %s" % (name, e))
        assert zlib.decompress(z) == x, name
    return out


def test_every_model_stream_passes_the_judge(streams, judged):
    assert len(judged) == len(streams) >= 26 + 1400
    kinds = {}
    for name, (p, choice) in judged.items():
        for t, _, _ in choice:
            kinds[t] = kinds.get(t, 0) + 1
    print("%d streams judged, blocks: %s" % (len(judged), kinds))
    assert kinds["dynamic"] > 1000 and kinds["stored"] > 50


def test_plan_bits_are_the_bits_written(streams, B):
    """plan_block()["bits"], the figure the choice rests on, against the size of the block when it is forced dynamic:
    every block of every input"""
    n = 0
    for name, (x, z, info) in streams.items():
        forced = deflate_proto.deflate(x, B, choose=lambda bits, pos, size: True)
        blocks = dz.parse(forced)["blocks"]
        assert zlib.decompress(forced) == x and len(blocks) == len(info), name
        for blk, inf in zip(blocks, info):
            assert blk["type"] == "dynamic" and blk["nbits"] == inf["bits"], (name, blk["nbits"], inf["bits"])
            n += 1
    assert n == sum(len(info) for _, _, info in streams.values())
    print("%d blocks forced dynamic: plan bits == written bits" % n)


# ---- wrong variants: (data, B, block index) -> the tokens of that block
def _chunk_257(data, B, bi):
    toks = []
    piece = data[bi * B:(bi + 1) * B]
    i = 0
    while i < len(piece):
        j = i
        while j < len(piece) and piece[j] == piece[i]:
            j += 1
        toks.append(("L", piece[i]))
        rest = j - i - 1
        while rest >= 257:
            toks.append(("M", 257, 1))
            rest -= 257
        toks += [("M", rest, 1)] if rest >= 3 else [("L", piece[i])] * rest
        i = j
    return toks


def _rest_3_as_literals(data, B, bi):
    toks, byte = [], None
    for t in dz.ref_tokens(data[bi * B:(bi + 1) * B]):
        if t[0] == "L":
            byte = t[1]            # (the run's byte: a 258 may stand between it and the rest)
        toks += [("L", byte)] * 3 if t == ("M", 3, 1) else [t]
    return toks


def _carry_dropped_at_tiles(data, B, bi):
    piece = data[bi * B:(bi + 1) * B]
    return [t for t0 in range(0, len(piece), 1024) for t in dz.ref_tokens(piece[t0:t0 + 1024])]


def _run_not_cut_at_block_end(data, B, bi):
    piece = data[bi * B:(bi + 1) * B]
    m = 0
    if bi > 0:
        while m < len(piece) and piece[m] == data[bi * B - 1]:
            m += 1
    if m == 0:
        return dz.ref_tokens(piece)
    # the run goes on: no literal of its own, matches over all m bytes
    return dz.ref_tokens(bytes([piece[0]]) * (m + 1))[1:] + dz.ref_tokens(piece[m:])


def _with_tokens(variant, data, B):
    """the model's stream with the variant as its tokenizer"""
    calls = []

    def tokens(b):
        toks = variant(data, B, len(calls))
        calls.append(1)
        sym = [t[1] if t[0] == "L" else dz.length_symbol(t[1])[0] for t in toks]
        ext = [0 if t[0] == "L" else dz.length_symbol(t[1])[1] for t in toks]
        val = [0 if t[0] == "L" else t[1] - dz.LEN_BASE[dz.length_symbol(t[1])[0] - 257] for t in toks]
        ism = [t[0] == "M" for t in toks]
        return (np.asarray(sym, dtype=np.int64), np.asarray(ext, dtype=np.int64), np.asarray(val, dtype=np.int64),
                np.asarray(ism, dtype=bool))

    keep = deflate_proto.tokens
    deflate_proto.tokens = tokens
    try:
        return deflate_proto.deflate(data, B)
    finally:
        deflate_proto.tokens = keep


WRONG_TOKENIZERS = [
    ("chunk of 257", _chunk_257, "run_s0_L259"),
    ("rest of 3 written as literals", _rest_3_as_literals, "run_s17_L4"),
    ("carry dropped at a tile boundary", _carry_dropped_at_tiles, "run_s1023_L4"),
    ("run not cut at the block end", _run_not_cut_at_block_end, "end_cross_k1_j3"),
]
WRONG_CHOOSERS = [
    ("<= in the choice", lambda bits, pos, size: bits <= 3 + (-(pos + 3)) % 8 + 32 + 8 * size, "even_pos0_m+0"),
    ("pos ignored in the padding", lambda bits, pos, size: bits < 3 + 5 + 32 + 8 * size, "even_pos7_m-1"),
]


def test_wrong_variants_are_caught(B, judged):
    """each wrong stream still inflates to the input (zlib alone would pass it) and fails the judge at the named input"""
    cs = deflate_cases.edge_cases(B)
    for what, variant, name in WRONG_TOKENIZERS:
        assert name in judged
        z = _with_tokens(variant, cs[name], B)
        assert zlib.decompress(z) == cs[name], (what, name)
        with pytest.raises(AssertionError, match="the format asks for"):
            dz.check_stream(z, cs[name], B)
        print("wrong tokenizer '%s': caught by %s" % (what, name))
    for what, choose, name in WRONG_CHOOSERS:
        assert name in judged
        z = deflate_proto.deflate(cs[name], B, choose=choose)
        assert zlib.decompress(z) == cs[name], (what, name)
        dz.check_stream(z, cs[name], B)            # (a well-formed stream: only the choice is wrong)
        with pytest.raises(AssertionError, match="its (dynamic|stored) form has"):
            dz.block_choice(z, cs[name], B, plan_of)
        print("wrong chooser '%s': caught by %s" % (what, name))
    assert len(WRONG_TOKENIZERS) + len(WRONG_CHOOSERS) >= 6


def test_the_judge_refuses_what_the_format_forbids():
    def stream(bits):   # bits: [(value, n)] behind the zlib header; padded, any check value
        v = n = 0
        for val, nb in bits:
            v |= val << n
            n += nb
        return b"\x78\x9c" + v.to_bytes((n + 7) // 8, "little") + bytes(4)

    dyn = [(1, 1), (2, 2), (0, 5), (0, 5)]
    # HCLEN 4: lengths of 16, 17, 18, 0 in that order
    cases = {
        "incomplete": dyn + [(0, 4), (1, 3), (0, 3), (0, 3), (0, 3)],
        "over-subscribed": dyn + [(0, 4), (1, 3), (1, 3), (1, 3), (0, 3)],
        "a 16 with nothing before it": dyn + [(0, 4), (1, 3), (0, 3), (1, 3), (0, 3), (0, 1)],
        "run past HLIT": dyn + [(0, 4), (0, 3), (0, 3), (1, 3), (1, 3), (1, 1), (127, 7), (1, 1), (127, 7)],
        "block type 3": [(1, 1), (3, 2)],
        "LEN": [(1, 1), (0, 2), (0, 5), (5, 16), (5, 16)],
    }
    for what, bits in cases.items():
        with pytest.raises(dz.FormatError, match=what):
            dz.parse(stream(bits))
    assert dz.ref_tokens(b"abbbb" + b"c" * 262) == [("L", 97), ("L", 98), ("M", 3, 1), ("L", 99), ("M", 258, 1), ("M", 3, 1)]
    assert dz.ref_tokens(b"c" * 261) == [("L", 99), ("M", 258, 1), ("L", 99), ("L", 99)]
    assert dz.huffman_cost([1, 1, 2, 3, 5]) == (1 * 4 + 1 * 4 + 2 * 3 + 3 * 2 + 5 * 1, 4)


def test_the_properties_the_inputs_were_made_for_fire(streams, judged, B):
    cs = deflate_cases.edge_cases(B)
    # the run sweep and the block-end runs are judged as dynamic blocks (a stored block would hide the tokens)
    for name in cs:
        if name.split("_")[0] in ("run", "end", "staircase"):
            assert all(t == "dynamic" for t, _, _ in judged[name][1]), name
    # near break-even: the margins are what the names say, at the position they say; one second block flips with pos
    seconds = {}
    for pos in range(8):
        for m in (-1, 0, 1):
            name = "even_pos%d_m%+d" % (pos, m)
            x, z, info = streams[name]
            (t1, _, _), (t2, a, b) = judged[name][1]
            blk = judged[name][0]["blocks"][1]
            assert t1 == "dynamic" and blk["start"] % 8 == pos == info[1]["pos"], name
            assert (a - b if t2 == "dynamic" else b - a) == m and t2 == ("dynamic" if m < 0 else "stored"), (name, t2, a, b)
            seconds.setdefault(x[B:], set()).add(t2)
    flips = sum(1 for v in seconds.values() if len(v) == 2)
    assert flips >= 1
    # HCLEN: short headers are written (the code lengths stop at 3 and 2: the last used place in the order is 14 or 16)
    ncl = {name: [b["hclen"] + 4 for b in judged[name][0]["blocks"] if b["type"] == "dynamic"] for name in judged}
    assert ncl["hclen_four"][0] in (14, 16) and ncl["hclen_eight"][0] in (14, 16)
    assert 14 in ncl["hclen_four"] + ncl["hclen_eight"]
    seen = sorted({v for k in ncl for v in ncl[k]})
    assert min(seen) < 18 and 18 in seen and 19 in seen
    # the code length code: 9 deep without the limit, 7 as written; the svb blocks reach 8
    def cl_depth(blk):
        clfreq = [0] * 19
        for s, _ in blk["items"]:
            clfreq[s] += 1
        return max(deflate_proto.build_lengths(clfreq, 30)), max(blk["cllens"])
    assert len(cs["cl_limit_dyadic"]) == 16383
    deep = cl_depth(judged["cl_limit_dyadic"][0]["blocks"][0])
    assert deep[0] >= 9 and deep[1] == 7, deep
    svb = max(cl_depth(judged[k][0]["blocks"][0]) for k in ("svb_B-1", "svb_B", "svb_B+1", "svb_2B+1", "run_over_block_end"))
    assert svb[0] >= 8 and svb[1] == 7, svb
    # stream lengths in every residue mod 4, stored and dynamic (the tail leaves byte-wise)
    res = {(len(z) % 4, judged[name][1][-1][0]) for name, (x, z, info) in streams.items() if name.startswith("len_")}
    assert res == {(r, t) for r in range(4) for t in ("stored", "dynamic")}
    # Adler-32 over tiles of 0xFF / 0xFE
    assert judged["high_ff_fe"][0]["adler"] == zlib.adler32(cs["high_ff_fe"])
    print("margins -1 / 0 / +1 at pos 0 - 7, %d second blocks flip with pos; HCLEN + 4 seen: %s; code length code depth "
          "unlimited %d (dyadic) and %d (svb), written %d; stream length residues mod 4: all, stored and dynamic"
          % (flips, seen, deep[0], svb[0], deep[1]))


def test_size_against_zlibs_rle(streams):
    """svb inputs of 4096 bytes and more: at most 1.005 of zlib's Z_RLE size (the margin: fixed 16 KB blocks against
    zlib's adaptive ones)"""
    worst = 0.0
    n = 0
    for name, (x, z, info) in streams.items():
        if (name.startswith("svb_") or name.startswith("len_")) and len(x) >= 4096:
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
            ref = len(c.compress(x) + c.flush())
            print("%s: %d bytes, Z_RLE %d, ratio %.4f" % (name, len(z), ref, len(z) / ref))
            worst = max(worst, len(z) / ref)
            assert len(z) <= 1.005 * ref, (name, len(z), ref)
            n += 1
    assert n >= 5
    print("worst ratio to Z_RLE over %d inputs: %.4f" % (n, worst))
