"""The float batch entry points (sgk_stat_f32, sgk_jnn_f32) without a GPU: the symbols, the workspace functions and every
refusal that is decided on the host, in the order the header gives them (arguments, workspace, device)."""
import ctypes as C

import numpy as np
import pytest

from sigtk_amd import api

SYMBOLS = ("sgk_stat_f32_workspace_bytes", "sgk_stat_f32", "sgk_jnn_f32_workspace_bytes", "sgk_jnn_f32")


@pytest.fixture(scope="module")
def lib():
    return api._float_lib()


def _ok_params():
    return api.JnnParam(0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0)


class _Call:
    """host buffers standing in for device memory: no entry point may look into them before it has found a device"""

    def __init__(self, lib, n_reads=3, max_len=1000, n_values=4000):
        self.lib, self.n_reads, self.max_len, self.n_values = lib, n_reads, max_len, n_values
        self.x = np.zeros(64, dtype=np.float32)
        self.offsets = np.zeros(8, dtype=np.uint64)
        self.lengths = np.zeros(8, dtype=np.uint32)
        self.out = np.full(64, 0xA5, dtype=np.uint8)
        self.misc = np.zeros(64, dtype=np.uint8)
        self.stat_ws = int(lib.sgk_stat_f32_workspace_bytes(n_reads, n_values, max_len))
        self.jnn_ws = int(lib.sgk_jnn_f32_workspace_bytes(n_reads, n_values, max_len))
        self.ws = np.zeros(max(self.stat_ws, self.jnn_ws, 64) + 16, dtype=np.uint8)

    def _ws(self):
        return (self.ws.ctypes.data + 15) & ~15

    def stat(self, ws_bytes=None):
        return self.lib.sgk_stat_f32(self.x.ctypes.data, self.offsets.ctypes.data, self.lengths.ctypes.data, self.n_reads,
                                     self.max_len, self.n_values, self.out.ctypes.data, self._ws(),
                                     self.stat_ws if ws_bytes is None else ws_bytes, None)

    def jnn(self, p, top=False, bot=False, ws_bytes=None):
        m = self.misc.ctypes.data
        return self.lib.sgk_jnn_f32(self.x.ctypes.data, self.offsets.ctypes.data, self.lengths.ctypes.data, self.n_reads,
                                    self.max_len, self.n_values, C.byref(p) if p is not None else None,
                                    m if top else None, m if bot else None, m, m, m, m, self._ws(),
                                    self.jnn_ws if ws_bytes is None else ws_bytes, None)


def test_symbols_are_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.ABI_SYMBOLS
    assert C.sizeof(api.StatFRec) == 16 and api.STATF_DTYPE.itemsize == 16


@pytest.mark.parametrize("fn", ["sgk_stat_f32_workspace_bytes", "sgk_jnn_f32_workspace_bytes"])
def test_workspace_is_monotone_and_nonzero(lib, fn):
    f = getattr(lib, fn)
    grid_r = [1, 2, 63, 64, 1023, 1024, 1025, 5000, 200000]
    grid_v = [1, 100, 4096, 10 ** 6, 10 ** 9]
    grid_l = [1, 17, 1024, 100000, 2 ** 31 - 1]
    for r in grid_r:
        for v in grid_v:
            for m in grid_l:
                assert int(f(r, v, m)) > 0
    for v in grid_v:
        for m in grid_l:
            got = [int(f(r, v, m)) for r in grid_r]
            assert got == sorted(got), (fn, "n_reads", v, m, got)
    for r in grid_r:
        for m in grid_l:
            got = [int(f(r, v, m)) for v in grid_v]
            assert got == sorted(got), (fn, "n_values", r, m, got)
        for v in grid_v:
            got = [int(f(r, v, m)) for m in grid_l]
            assert got == sorted(got), (fn, "max_read_len", r, v, got)


def test_refused_parameter_sets(lib):
    c = _Call(lib)
    bad = [api.JnnParam(0.75, 50, 50, 31, 0.25, 5, 0.0, 0.0),             # window < 32
           api.JnnParam(0.75, 0, 50, 150, 0.25, 5, 0.0, 0.0),              # corrector < 1
           api.JnnParam(0.75, 50, 50, 150, 0.25, -1, 0.0, 0.0),            # error < 0
           api.JnnParam(0.75, 50, -1, 150, 0.25, 5, 0.0, 0.0),             # seg_dist < 0
           api.JnnParam(float("nan"), 50, 50, 150, 0.25, 5, 0.0, 0.0),     # std_scale not finite
           api.JnnParam(0.75, 50, 50, 150, float("inf"), 5, 0.0, 0.0)]     # stall_len not finite
    for p in bad:
        assert api._param_lib().sgk_jnn_params_check(C.byref(p)) == api.SGK_ERR_ARG
        assert c.jnn(p) == api.SGK_ERR_ARG
    assert c.jnn(None) == api.SGK_ERR_ARG


def test_per_read_thresholds_come_in_pairs_and_with_fixed_sets_only(lib):
    c = _Call(lib)
    fixed = api.JnnParam(-1.0, 50, 200, 250, 1.0, 30, 0.0, 0.0)
    assert c.jnn(fixed, top=True, bot=False) == api.SGK_ERR_ARG
    assert c.jnn(fixed, top=False, bot=True) == api.SGK_ERR_ARG
    assert c.jnn(_ok_params(), top=True, bot=True) == api.SGK_ERR_ARG   # std_scale > 0


def test_a_read_of_2_31_values_is_refused(lib):
    c = _Call(lib, n_reads=1, max_len=2 ** 31, n_values=2 ** 31 + 8)
    c.lengths[0] = 2 ** 31
    assert c.stat() == api.SGK_ERR_ARG
    assert c.jnn(_ok_params()) == api.SGK_ERR_ARG
    assert (c.out == 0xA5).all()


def test_short_workspace_and_empty_batch(lib):
    c = _Call(lib)
    assert c.stat(ws_bytes=c.stat_ws - 1) == api.SGK_ERR_WORKSPACE
    assert c.jnn(_ok_params(), ws_bytes=c.jnn_ws - 1) == api.SGK_ERR_WORKSPACE
    assert (c.out == 0xA5).all()
    empty = _Call(lib, n_reads=0, max_len=0, n_values=0)
    assert empty.stat() == api.SGK_OK and empty.jnn(_ok_params()) == api.SGK_OK


def test_valid_calls_without_a_gpu_are_a_loud_error(lib):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call(lib)
    assert c.stat() == api.SGK_ERR_NODEVICE
    assert c.jnn(_ok_params()) == api.SGK_ERR_NODEVICE
    assert c.jnn(api.JnnParam(-1.0, 50, 200, 250, 1.0, 30, 0.0, 0.0), top=True, bot=True) == api.SGK_ERR_NODEVICE
    assert (c.out == 0xA5).all()


# What the parent of the commit that made the scratch-row rule one function (literal_rows, stat_args.h) returned: both
# workspaces hold min(n_reads, 1024) rows for the longest read, fewer above SGK_LITERAL_MAX_BYTES, never less than one --
# int16 rows behind sgk_stat's long-read part, float rows behind sgk_stat_f32's dispatch order.  n_samples = n_reads x
# max_read_len.
WS_N_READS = [0, 1, 2, 1023, 1024, 1025, 200000]
WS_MAX_READ_LEN = [0, 1, 3, 4, 5000, 3000001, 0x7fffffff]
WS_BYTES = {
    "sgk_stat_workspace_bytes": [
        [4749952, 4749952, 4749952, 4749952, 4749952, 4749984, 4749984],
        [4750016, 4750032, 4750032, 4750032, 4760016, 10808640, 4316494528],
        [4750016, 4750048, 4750048, 4750048, 4770016, 16860208, 4316494528],
        [4754048, 4770416, 4770416, 4770416, 14984048, 285531968, 4316498560],
        [4754048, 4770432, 4770432, 4770432, 14994048, 285531968, 4316498560],
        [4754112, 4770496, 4770496, 4770496, 14994112, 285532032, 4316498624],
        [5549952, 5566336, 5566336, 5566336, 15789952, 286327872, 4317294464],
    ],
    "sgk_stat_f32_workspace_bytes": [
        [576, 576, 576, 576, 576, 576, 576],
        [640, 656, 656, 656, 20640, 12000656, 8589935232],
        [640, 672, 672, 672, 40640, 24000672, 8589935232],
        [4672, 21040, 21040, 21040, 20464672, 264005024, 8589939264],
        [4672, 21056, 21056, 21056, 20484672, 264005024, 8589939264],
        [4736, 21120, 21120, 21120, 20484736, 264005088, 8589939328],
        [800576, 816960, 816960, 816960, 21280576, 264800928, 8590735168],
    ],
}


@pytest.mark.parametrize("fn", sorted(WS_BYTES))
def test_scratch_rows_of_both_workspaces_are_what_they_were(lib, fn):
    api.load_library()   # (binds the int16 workspace functions)
    f = getattr(lib, fn)
    for r, row in zip(WS_N_READS, WS_BYTES[fn]):
        got = [int(f(r, r * m, m)) for m in WS_MAX_READ_LEN]
        assert got == row, (fn, r, got)
