"""GPU: k_deflate (csrc/deflate_kernels.hip) off its aligned path and at its decision edges.  The inputs are
deflate_cases.edge_cases(): every stream must be the model's (tools/proto/deflate_proto.py) byte for byte and pass the
independent judge (tests/deflate_parse.py) on the GPU's own bytes; the same inputs at input addresses that are no
multiple of 16 must give the same streams; room is tested at its boundaries; and one launch has more streams than are
resident at once."""
import os
import sys
import zlib

import pytest

import deflate_cases
import deflate_parse as dz

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import deflate_proto  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFTS = (1, 3, 4, 8, 13, 15)


@pytest.fixture(scope="module")
def batch(gpu):
    """(names, inputs, model streams, device result at shift 0, block size) -- one launch, computed once"""
    from sigtk_amd import device
    block = int(gpu.load_library().sgk_deflate_block_bytes())
    cs = deflate_cases.edge_cases(block)
    names = list(cs)
    data = [cs[k] for k in names]
    model = [deflate_proto.deflate(x, block) for x in data]
    got = device.deflate(data, with_gaps=True, fill=0xA5)
    return names, data, model, got, block


def test_every_edge_stream_is_the_models(batch):
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    assert [int(s) for s in st] == [0] * len(names)
    wrong = [name for r, name in enumerate(names) if kept[r] != model[r]]
    assert not wrong, (len(wrong), wrong[:10])
    for r, name in enumerate(names):
        assert len(gaps[r]) >= 48 and gaps[r] == b"\xa5" * len(gaps[r]), name


@pytest.mark.parametrize("group", deflate_cases.EDGE_GROUPS)
def test_the_gpu_bytes_pass_the_judge(batch, group):
    """check_stream on what the kernel wrote, not on the model's copy; zlib reads it back"""
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    n = 0
    for r, name in enumerate(names):
        if name.split("_")[0] == group:
            assert kept[r] is not None, name
            try:
                dz.check_stream(kept[r], data[r], block)
            except (AssertionError, dz.FormatError) as e:
                raise AssertionError("%s: %s" % (name, e))
            assert zlib.decompress(kept[r]) == data[r], name
            n += 1
    assert n > 0


def test_unaligned_input_gives_the_same_streams(batch):
    """in + in_offsets[r] at every residue mod 16 that matters (odd, 4, 8, one below 16): every lane of every tile then
    loads byte-wise, with prv and nxt at odd addresses"""
    from sigtk_amd import device
    names, data, model, first, block = batch
    base = dict(zip(names, first[0]))
    cs = dict(zip(names, data))
    cs["svb_2B+1"] = deflate_cases.svb_bytes(2 * block + 1)
    base["svb_2B+1"] = deflate_proto.deflate(cs["svb_2B+1"], block)
    jobs = [(name, s) for name in cs if name.split("_")[0] in ("run", "end", "even") or name == "svb_2B+1" for s in SHIFTS]
    jobs += [("len_%d" % n, s) for n in range(41) for s in range(1, 16)]
    kept, olen, st, gaps, capat = device.deflate([cs[name] for name, s in jobs], with_gaps=True, fill=0xA5,
                                                 in_shift=[s for name, s in jobs])
    assert [int(s) for s in st] == [0] * len(jobs)
    wrong = [(name, s) for r, (name, s) in enumerate(jobs) if kept[r] != base[name]]
    assert not wrong, (len(wrong), wrong[:10])
    assert all(g == b"\xa5" * len(g) for g in gaps)
    print("%d streams; shifts %s, and lengths 0 - 40 at shifts 1 - 15" % (len(jobs), SHIFTS))


def test_room_at_its_boundaries(batch):
    """eight streams whose lengths cover every residue mod 4, stored and dynamic, each with room for exactly its length,
    one byte less, the dwords below it, one byte less than those, 3 and 0 bytes; a neighbour with full room behind each"""
    from sigtk_amd import device
    names, data, model, first, block = batch
    victims = {}
    for r, name in enumerate(names):
        if name.startswith("len_"):
            kind = "stored" if model[r][2] & 6 == 0 else "dynamic"
            victims.setdefault((len(model[r]) % 4, kind), r)
    assert sorted(victims) == [(q, k) for q in range(4) for k in ("dynamic", "stored")]
    nb = names.index("staircase")
    rows, caps, want = [], [], []
    for (q, kind), r in sorted(victims.items()):
        ln = len(model[r])
        for cap in (ln, ln - 1, ln - ln % 4, ln - ln % 4 - 1, 3, 0):
            rows += [r, nb]
            caps += [cap, device.deflate_bound(len(data[nb]))]
            want += [cap >= ln, True]
    kept, olen, st, gaps, capat = device.deflate([data[r] for r in rows], caps=caps, with_gaps=True, fill=0xA5)
    for i, r in enumerate(rows):
        what = (names[r], caps[i], len(model[r]))
        if want[i]:
            assert int(st[i]) == 0 and kept[i] == model[r], what
            assert gaps[i] == b"\xa5" * len(gaps[i]), what
        else:
            assert int(st[i]) == 1 and kept[i] is None, what
            tail = gaps[i][capat[i]:]                    # from out_caps[r] on
            assert tail == b"\xa5" * len(tail) and len(tail) >= 48, what
    assert sum(1 for w in want if not w) >= 8 * 4


def test_more_streams_than_are_resident(gpu, batch):
    from sigtk_amd import device
    block = batch[4]
    data = [deflate_cases.svb_bytes(r % 97) for r in range(3000)]
    model = [deflate_proto.deflate(data[r], block) for r in range(97)]
    kept, olen, st = device.deflate(data)
    assert [int(s) for s in st] == [0] * 3000
    wrong = [r for r in range(3000) if kept[r] != model[r % 97]]
    assert not wrong, (len(wrong), wrong[:10])
