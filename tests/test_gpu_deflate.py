"""GPU: sgk_deflate (csrc/deflate_kernels.hip) -- zlib streams written one wavefront each -- against the CPU model
(tools/proto/deflate_proto.py), byte for byte, and against zlib and our own k_inflate, which must both read them back.
The inputs are those of tests/deflate_cases.py, in one batch; the output regions are pre-filled with 0xA5 and have gaps
between them, which must stay as they were."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import deflate_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import deflate_proto  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(gpu):
    """(names, inputs, model streams, device result) -- computed once"""
    from sigtk_amd import device
    block = int(gpu.load_library().sgk_deflate_block_bytes())
    cs = deflate_cases.cases(block)
    names = list(cs)
    data = [cs[k] for k in names]
    model = [deflate_proto.deflate(x, block) for x in data]
    got = device.deflate(data, with_gaps=True, fill=0xA5)
    return names, data, model, got, block


def test_every_stream_is_the_models(batch):
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    assert [int(s) for s in st] == [0] * len(names)
    for r, name in enumerate(names):
        assert kept[r] == model[r], (name, len(kept[r]), len(model[r]))


def test_zlib_reads_them_back_and_the_bound_holds(batch):
    from sigtk_amd import device
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    for r, name in enumerate(names):
        assert zlib.decompress(kept[r]) == data[r], name
        assert int(olen[r]) == len(kept[r]) <= device.deflate_bound(len(data[r])), name


def test_nothing_written_behind_the_streams(batch):
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    for r, name in enumerate(names):
        assert len(gaps[r]) >= 48 and gaps[r] == b"\xa5" * len(gaps[r]), name


def test_stored_and_run_coded_sizes(batch):
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    z = kept[names.index("random70000")]
    # stored blocks, none above 65 535 bytes: walk them
    pos, seen = 2, 0
    while True:
        hdr = z[pos]
        assert hdr & 6 == 0
        ln, nln = int.from_bytes(z[pos + 1:pos + 3], "little"), int.from_bytes(z[pos + 3:pos + 5], "little")
        assert ln ^ nln == 0xFFFF and ln <= 65535
        pos += 5 + ln
        seen += ln
        if hdr & 1:
            break
    assert seen == 70000 and pos + 4 == len(z) <= 70000 + 5 * max(1, -(-70000 // min(block, 65535))) + 6
    assert len(kept[names.index("zeros100000")]) < 100000 // 64


def test_our_inflate_reads_them_back(batch):
    from sigtk_amd import device
    names, data, model, (kept, olen, st, gaps, capat), block = batch
    got, ilen, ist = device.inflate(kept, caps=[len(x) + 5 for x in data])
    assert [int(s) for s in ist] == [0] * len(names)
    for r, name in enumerate(names):
        assert got[r] == data[r], name


def test_too_little_room_is_reported_and_respected(batch):
    from sigtk_amd import device
    names, data, model, first, block = batch
    victims = {names.index("svb_2B+1"), names.index("random70000"), names.index("same1"), names.index("fibonacci")}
    caps = [len(m) // 2 if r in victims else device.deflate_bound(len(data[r])) for r, m in enumerate(model)]
    kept, olen, st, gaps, capat = device.deflate(data, caps=caps, with_gaps=True, fill=0xA5)
    for r, name in enumerate(names):
        if r in victims:
            assert int(st[r]) == 1 and kept[r] is None, name
            tail = gaps[r][capat[r]:]                    # from out_caps[r] on
            assert tail == b"\xa5" * len(tail) and len(tail) >= 48, name
        else:
            assert int(st[r]) == 0 and kept[r] == model[r], name
            assert gaps[r] == b"\xa5" * len(gaps[r]), name


def test_streams_of_half_a_gigabyte_are_refused(gpu):
    import torch
    L = gpu.load_library()
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_out = torch.full((256,), 0xA5, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2, dtype=torch.int64, device=dev)
    d_ooff = torch.tensor([0, 64], dtype=torch.int64, device=dev)
    d_len = torch.tensor([5, 1 << 29], dtype=torch.int32, device=dev)
    d_caps = torch.tensor([64, 64], dtype=torch.int32, device=dev)
    d_olen = torch.zeros(2, dtype=torch.int32, device=dev)
    d_st = torch.zeros(2, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.sgk_deflate(p(d_in), p(d_off), p(d_len), 2, p(d_out), p(d_ooff), p(d_caps), p(d_olen), p(d_st),
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1   # SGK_ERR_ARG
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 256
