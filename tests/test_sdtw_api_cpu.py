"""sgk_sdtw_f32 without a GPU: the symbols, the record, the workspace function and every refusal that is decided on the
host, in the order the header gives them (arguments, workspace, device)."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from sigtk_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return api._float_lib()


class _Call:
    """host buffers standing in for device memory: the entry point may not look into them before it has found a device"""

    def __init__(self, lib, nq=3, max_q=200, nt=2, max_t=1000):
        self.lib, self.nq, self.max_q, self.nt, self.max_t = lib, nq, max_q, nt, max_t
        self.x = np.zeros(64, dtype=np.float32)
        self.offsets = np.zeros(8, dtype=np.uint64)
        self.lengths = np.zeros(8, dtype=np.uint32)
        self.out = np.full(256, 0xA5, dtype=np.uint8)
        self.need = int(lib.sgk_sdtw_f32_workspace_bytes(nq, max_q, nt, max_t))
        self.ws = np.full(max(self.need, 64) + 16, 0x5A, dtype=np.uint8)

    def __call__(self, options=0, ws_bytes=None, q=True, qo=True, ql=True, t=True, to=True, tl=True, out=True, ws=True, ws_shift=0):
        p = lambda arr, on: arr.ctypes.data if on else None   # noqa: E731
        wsp = (((self.ws.ctypes.data + 15) & ~15) + ws_shift) if ws else None
        return self.lib.sgk_sdtw_f32(p(self.x, q), p(self.offsets, qo), p(self.lengths, ql), self.nq, self.max_q, 64,
                                     p(self.x, t), p(self.offsets, to), p(self.lengths, tl), self.nt, self.max_t, 64,
                                     options, p(self.out, out), wsp, self.need if ws_bytes is None else ws_bytes, None)

    def untouched(self):
        return bool((self.out == 0xA5).all() and (self.ws == 0x5A).all())


def test_symbols_record_and_constants(lib):
    for s in ("sgk_sdtw_f32_workspace_bytes", "sgk_sdtw_f32"):
        assert hasattr(lib, s), s
        assert s in api.ABI_SYMBOLS
    assert C.sizeof(api.SdtwRec) == 16 and api.SDTW_DTYPE.itemsize == 16
    assert [api.SDTW_DTYPE.fields[f][1] for f in ("score", "end", "start", "flags")] == [0, 4, 8, 12]
    src = open(os.path.join(ROOT, "include", "sigtk_gpu.h")).read()
    for name, value in (("SGK_SDTW_NO_START", api.SDTW_NO_START), ("SGK_SDTW_EMPTY", api.SDTW_EMPTY),
                        ("SGK_SDTW_NONFINITE", api.SDTW_NONFINITE), ("SGK_SDTW_TOO_LONG", api.SDTW_TOO_LONG)):
        assert re.search(r"#define %s +%du\b" % (name, value), src), name


def test_unknown_option_bits_are_refused(lib):
    c = _Call(lib)
    for options in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
        assert c(options=options) == api.SGK_ERR_ARG, options
    assert c.untouched()


@pytest.mark.parametrize("missing", ["q", "qo", "ql", "t", "to", "tl", "out", "ws"])
def test_a_null_pointer_with_a_count_is_refused(lib, missing):
    c = _Call(lib)
    assert c(**{missing: False}) == api.SGK_ERR_ARG
    assert c.untouched()


def test_alignment_and_lengths_of_2_31(lib):
    c = _Call(lib)
    assert c(ws_shift=8) == api.SGK_ERR_ARG                     # the workspace is 16-byte aligned
    assert _Call(lib, max_q=2 ** 31)() == api.SGK_ERR_ARG
    assert _Call(lib, max_t=2 ** 31)() == api.SGK_ERR_ARG
    c.x = np.zeros(65, dtype=np.float32)[1:]                    # q and t are 4-byte aligned: any element of an array will do
    assert c(ws_bytes=0) == api.SGK_ERR_WORKSPACE
    c.x = np.zeros(260, dtype=np.uint8)[2:]                     # ... but not half an element
    assert c() == api.SGK_ERR_ARG
    assert c.untouched()


def test_an_empty_side_is_ok_and_looks_at_nothing(lib):
    for nq, nt in ((0, 2), (3, 0), (0, 0)):
        c = _Call(lib, nq=nq, nt=nt)
        assert c(q=nq > 0, qo=nq > 0, ql=nq > 0, t=nt > 0, to=nt > 0, tl=nt > 0, out=False, ws=False, ws_bytes=0) == api.SGK_OK
        assert c() == api.SGK_OK
        assert c.untouched()
    # ... but the other side's null pointer is still an argument error, and so is an unknown option
    assert _Call(lib, nq=0)(t=False) == api.SGK_ERR_ARG
    assert _Call(lib, nt=0)(ql=False) == api.SGK_ERR_ARG
    assert _Call(lib, nq=0)(options=2) == api.SGK_ERR_ARG


def test_a_short_workspace_comes_after_the_arguments_and_writes_nothing(lib):
    for max_q in (200, 5000):
        c = _Call(lib, max_q=max_q)
        assert c(ws_bytes=c.need - 1) == api.SGK_ERR_WORKSPACE
        assert c(ws_bytes=0) == api.SGK_ERR_WORKSPACE
        assert c(ws_bytes=c.need - 1, options=2) == api.SGK_ERR_ARG
        assert c(ws_bytes=c.need - 1, out=False) == api.SGK_ERR_ARG
        assert c.untouched()


def test_no_device_comes_last(lib):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    for max_q in (200, 5000):
        c = _Call(lib, max_q=max_q)
        assert c() == api.SGK_ERR_NODEVICE
        assert c(options=api.SDTW_NO_START) == api.SGK_ERR_NODEVICE
        assert c(ws_bytes=c.need - 1) == api.SGK_ERR_WORKSPACE
        assert c(options=2) == api.SGK_ERR_ARG
        assert c.untouched()


GRID_NQ = [0, 1, 2, 1023, 1024, 1025, 10000, 200000]
GRID_MQ = [0, 1, 64, 65, 1024, 1025, 4096, 100000, 2 ** 31 - 1]
GRID_NT = [0, 1, 2, 7, 1000]
GRID_MT = [0, 1, 63, 64, 65, 30000, 10 ** 8, 2 ** 31 - 1]


def test_workspace_is_monotone_in_every_argument(lib):
    f = lib.sgk_sdtw_f32_workspace_bytes
    size = {(a, b, c, d): int(f(a, b, c, d)) for a in GRID_NQ for b in GRID_MQ for c in GRID_NT for d in GRID_MT}
    for b in GRID_MQ:
        for c in GRID_NT:
            for d in GRID_MT:
                got = [size[a, b, c, d] for a in GRID_NQ]
                assert got == sorted(got), ("n_queries", b, c, d, got)
    for a in GRID_NQ:
        for c in GRID_NT:
            for d in GRID_MT:
                got = [size[a, b, c, d] for b in GRID_MQ]
                assert got == sorted(got), ("max_query_len", a, c, d, got)
    for a in GRID_NQ:
        for b in GRID_MQ:
            for d in GRID_MT:
                got = [size[a, b, c, d] for c in GRID_NT]
                assert got == sorted(got), ("n_targets", a, b, d, got)
            for c in GRID_NT:
                got = [size[a, b, c, d] for d in GRID_MT]
                assert got == sorted(got), ("max_target_len", a, b, c, got)
    assert all(v > 0 for (a, b, c, d), v in size.items() if a and c)


def test_queries_of_one_band_need_no_band_rows(lib):
    """up to 1 024 values the workspace is a few words per read, whatever the targets' length ..."""
    f = lib.sgk_sdtw_f32_workspace_bytes
    for nq in (1, 1000, 200000):
        for max_q in (1, 250, 1024):
            sizes = {int(f(nq, max_q, 2, max_t)) for max_t in (1, 30000, 10 ** 8, 2 ** 31 - 1)}
            assert len(sizes) == 1, (nq, max_q, sizes)
            assert sizes.pop() <= 1024 + 16 * nq, (nq, max_q)


def test_band_rows_are_a_fixed_number_of_slots(lib):
    """... and above that it holds band rows for the waves in flight, not for the pairs: the same for 2 048 pairs and for
    200 000 x 2, never n_pairs x max_target_len, one row at least"""
    f = lib.sgk_sdtw_f32_workspace_bytes
    base = lambda nq, nt: int(f(nq, 1024, nt, 30000))   # noqa: E731
    rows = lambda nq, nt, max_t=30000: int(f(nq, 4096, nt, max_t)) - int(f(nq, 1024, nt, max_t))   # noqa: E731
    assert base(10, 2) > 0
    assert rows(1024, 2) == rows(200000, 2) == rows(5000, 7)
    assert rows(1, 1) >= 30000 * 8 and rows(1, 2) <= 2 * rows(1, 1)
    assert rows(200000, 2) <= 2048 * (30000 + 64) * 8
    assert rows(200000, 2, 10 ** 8) <= max(2 ** 30, (10 ** 8 + 64) * 8)
    assert rows(200000, 2, 2 ** 31 - 1) >= (2 ** 31 - 1) * 8
