"""Normalised signals without a GPU: the numpy model (tests/normalise_model.py) against reads worked out by hand, every
refusal of sgk_normalise_f32 / sgk_normalise / sgk_job_set_normalise and the two size functions that is decided on the
host (arguments, then workspace, then device), and what `sigtk-amd pa --normalise` refuses before it opens a file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import normalise_model as nm
from sigtk_amd import api, build

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP1 = os.path.join(ROOT, "tests", "golden", "sp1_dna.blow5")
NOFILE = "/nonexistent/reads.blow5"
SYMBOLS = ("sgk_normalise_f32_workspace_bytes", "sgk_normalise_f32", "sgk_normalise_workspace_bytes", "sgk_normalise",
           "sgk_job_set_normalise")
METHODS = (nm.ZSCORE, nm.MEDMAD)


@pytest.fixture(scope="module")
def lib():
    return api._float_lib()


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI):
        build.build_lib()
        build.build_cli()
    return build.CLI


# ------------------------------------------------------------------------------------------------ the model, by hand

def _model(x, method, oracle, reflib):
    return nm.normalise(np.array(x, dtype=F), method, nm.statf_of(oracle, reflib))


def test_model_constant_read(oracle, reflib):
    for method in METHODS:
        y, (shift, scale, n, flags) = _model([5, 5, 5], method, oracle, reflib)
        assert np.isnan(y).all() and y.size == 3                      # 0 / 0
        assert (float(shift), float(scale), n, flags) == (5.0, 0.0, 3, nm.ZERO_SCALE)


def test_model_two_values(oracle, reflib):
    # mean 2, squared deviations 1 + 1, std sqrt(2 / 2) = 1
    y, rec = _model([1, 3], nm.ZSCORE, oracle, reflib)
    assert y.tolist() == [-1.0, 1.0] and (float(rec[0]), float(rec[1]), rec[2], rec[3]) == (2.0, 1.0, 2, 0)
    # rank n / 2 = 1: the median is 3; d = [2, 0], its rank 1 is 2; scale = 2 * 1.4826f
    y, rec = _model([1, 3], nm.MEDMAD, oracle, reflib)
    scale = F(2) * F(1.4826)
    assert nm.bits(rec[0]) == nm.bits(F(3)) and nm.bits(rec[1]) == nm.bits(scale) and rec[2:] == (2, 0)
    assert nm.bits(y).tolist() == nm.bits(np.array([F(-2) / scale, F(0)], dtype=F)).tolist()
    assert abs(float(y[0]) + 1 / 1.4826) < 1e-7


def test_model_read_with_a_nan_or_an_infinity(oracle, reflib):
    for bad in (float("nan"), float("inf"), -float("inf")):
        for method in METHODS:
            y, (shift, scale, n, flags) = _model([1, bad, 2], method, oracle, reflib)
            assert np.isnan(y).all() and np.isnan(shift) and np.isnan(scale) and (n, flags) == (3, nm.NONFINITE)


def test_model_zeros_of_either_sign(oracle, reflib):
    pz, nz = nm.bits(F(0.0))[()], nm.bits(F(-0.0))[()]
    # the median of a read of -0 is -0; its mean is +0: the sum starts from +0 and +0 + -0 = +0
    y, rec = _model([-0.0] * 3, nm.MEDMAD, oracle, reflib)
    assert nm.bits(rec[0]) == nz and nm.bits(rec[1]) == pz and rec[3] == nm.ZERO_SCALE and np.isnan(y).all()
    y, rec = _model([-0.0] * 3, nm.ZSCORE, oracle, reflib)
    assert nm.bits(rec[0]) == pz and rec[3] == nm.ZERO_SCALE and np.isnan(y).all()
    y, rec = _model([0.0] * 3, nm.MEDMAD, oracle, reflib)
    assert nm.bits(rec[0]) == pz and rec[3] == nm.ZERO_SCALE
    # a zero median with a scale that is not zero: -0 - (+0) = -0 but +0 - (+0) = +0, and the quotient keeps the sign.
    # Sorted by value the middle of the five is the +0 (it is the only zero)
    y, rec = _model([-2.0, -1.0, 0.0, 1.0, 2.0], nm.MEDMAD, oracle, reflib)
    assert nm.bits(rec[0]) == pz and nm.bits(rec[1]) == nm.bits(F(1) * F(1.4826)) and rec[3] == 0
    assert nm.bits(y[2]) == pz
    x = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, -0.0], dtype=F)   # (whichever zero the reference picks, the model follows)
    y, rec = nm.normalise(x, nm.MEDMAD, nm.statf_of(oracle, reflib))
    assert float(rec[0]) == 0.0
    with np.errstate(all="ignore"):
        assert nm.bits(y).tolist() == nm.bits((x - rec[0]) / rec[1]).tolist()
    assert nm.bits(y[2]) != nm.bits(y[5]) or np.signbit(rec[0])   # -0 - (-0) = +0: only a -0 median merges the two


def test_model_empty_read(oracle, reflib):
    y, (shift, scale, n, flags) = _model([], nm.ZSCORE, oracle, reflib)
    assert y.size == 0 and np.isnan(shift) and np.isnan(scale) and (n, flags) == (0, 0)


def test_model_constants_are_the_headers():
    assert (api.NORM_ZSCORE, api.NORM_MEDMAD, api.NORM_ZERO_SCALE, api.NORM_NONFINITE) == (nm.ZSCORE, nm.MEDMAD, nm.ZERO_SCALE, nm.NONFINITE)
    hdr = open(os.path.join(ROOT, "include", "sigtk_gpu.h")).read()
    for name, v in (("SGK_NORM_ZSCORE", "1"), ("SGK_NORM_MEDMAD", "2"), ("SGK_NORM_ZERO_SCALE", "1u"), ("SGK_NORM_NONFINITE", "2u")):
        assert "#define %s %s" % (name, v) in hdr
    assert api.NORM_DTYPE.itemsize == 16 and api.NORM_METHODS == {"zscore": 1, "medmad": 2}


# ------------------------------------------------------------------------------------------------ the entry points

class _Call:
    """host buffers standing in for device memory: no entry point may look into them before it has found a device"""

    def __init__(self, lib, n_reads=3, max_len=1000, n_values=4000):
        self.lib, self.n_reads, self.max_len, self.n_values = lib, n_reads, max_len, n_values
        self.x = np.zeros(64, dtype=F)
        self.offsets = np.zeros(8, dtype=np.uint64)
        self.lengths = np.zeros(8, dtype=np.uint32)
        self.dbl = np.zeros(8, dtype=np.float64)
        self.samples = np.zeros(64 + 8, dtype=np.int16)
        self.y = np.full(64, 0xA5, dtype=np.uint8)
        self.rec = np.full(64, 0xA5, dtype=np.uint8)
        self.need_f = int(lib.sgk_normalise_f32_workspace_bytes(n_reads, n_values, max_len))
        self.need_i = int(lib.sgk_normalise_workspace_bytes(n_reads, n_values, max_len))
        self.ws = np.zeros(max(self.need_f, self.need_i, 64) + 16, dtype=np.uint8)

    def _ws(self):
        return (self.ws.ctypes.data + 15) & ~15

    def f32(self, method=nm.ZSCORE, ws_bytes=None, **over):
        a = dict(x=self.x.ctypes.data, offsets=self.offsets.ctypes.data, lengths=self.lengths.ctypes.data, y=self.y.ctypes.data,
                 rec=self.rec.ctypes.data, ws=self._ws())
        a.update(over)
        return self.lib.sgk_normalise_f32(a["x"], a["offsets"], a["lengths"], self.n_reads, self.max_len, self.n_values, method,
                                          a["y"], a["rec"], a["ws"], self.need_f if ws_bytes is None else ws_bytes, None)

    def i16(self, method=nm.ZSCORE, ws_bytes=None, batch=True, **over):
        a = dict(y=self.y.ctypes.data, rec=self.rec.ctypes.data, ws=self._ws())
        a.update(over)
        d = self.dbl.ctypes.data
        samples = (self.samples.ctypes.data + 15) & ~15
        view = api.Batch(samples, self.offsets.ctypes.data, self.lengths.ctypes.data, d, d, d, self.n_reads, self.max_len,
                         self.n_values)
        return self.lib.sgk_normalise(C.addressof(view) if batch else None, method, a["y"], a["rec"], a["ws"],
                                      self.need_i if ws_bytes is None else ws_bytes, None)

    def untouched(self):
        return bool((self.y == 0xA5).all() and (self.rec == 0xA5).all())


def test_symbols_are_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.ABI_SYMBOLS


def test_bad_method_is_refused(lib):
    c = _Call(lib)
    for m in (0, 3, -1, 255):
        assert c.f32(method=m) == api.SGK_ERR_ARG and c.i16(method=m) == api.SGK_ERR_ARG
    empty = _Call(lib, n_reads=0, max_len=0, n_values=0)
    assert empty.f32(method=0) == api.SGK_ERR_ARG and empty.i16(method=7) == api.SGK_ERR_ARG
    assert c.untouched()


def test_null_and_misaligned_pointers_are_refused(lib):
    c = _Call(lib)
    for m in METHODS:
        for name in ("x", "offsets", "lengths", "y", "rec", "ws"):
            assert c.f32(method=m, **{name: None}) == api.SGK_ERR_ARG, name
        for name in ("y", "rec", "ws"):
            assert c.i16(method=m, **{name: None}) == api.SGK_ERR_ARG, name
        assert c.i16(method=m, batch=False) == api.SGK_ERR_ARG
        assert c.f32(method=m, x=c.x.ctypes.data + 2) == api.SGK_ERR_ARG      # x, y: 4-byte aligned
        assert c.f32(method=m, y=c.y.ctypes.data + 2) == api.SGK_ERR_ARG
        assert c.i16(method=m, y=c.y.ctypes.data + 2) == api.SGK_ERR_ARG
        assert c.f32(method=m, ws=c._ws() + 4) == api.SGK_ERR_ARG             # the workspace: 16-byte aligned
        assert c.i16(method=m, ws=c._ws() + 4) == api.SGK_ERR_ARG
    assert c.untouched()


def test_y_is_x_or_apart(lib):
    c = _Call(lib, n_reads=1, max_len=16, n_values=32)
    assert c.f32(y=c.x.ctypes.data + 4) == api.SGK_ERR_ARG                    # overlapping, not the same
    assert c.f32(y=c.x.ctypes.data + 4 * 31) == api.SGK_ERR_ARG
    if api.device_count() == 0:   # (with a device these two would launch on host memory)
        assert c.f32(y=c.x.ctypes.data) == api.SGK_ERR_NODEVICE                # in place
        assert c.f32(y=c.x.ctypes.data + 4 * 32) == api.SGK_ERR_NODEVICE       # touching


def test_a_read_of_2_31_values_is_refused(lib):
    c = _Call(lib, n_reads=1, max_len=2 ** 31, n_values=2 ** 31 + 8)
    c.lengths[0] = 2 ** 31
    assert c.f32() == api.SGK_ERR_ARG and c.i16() == api.SGK_ERR_ARG and c.untouched()


def test_short_workspace_and_empty_batch(lib):
    c = _Call(lib)
    for m in METHODS:
        assert c.f32(method=m, ws_bytes=c.need_f - 1) == api.SGK_ERR_WORKSPACE
        assert c.i16(method=m, ws_bytes=c.need_i - 1) == api.SGK_ERR_WORKSPACE
        assert c.f32(method=m, ws_bytes=0) == api.SGK_ERR_WORKSPACE
    assert c.untouched()
    empty = _Call(lib, n_reads=0, max_len=0, n_values=0)
    for m in METHODS:
        assert empty.f32(method=m) == api.SGK_OK and empty.i16(method=m) == api.SGK_OK
        assert empty.f32(method=m, x=None, y=None, rec=None, ws=None) == api.SGK_OK
    assert empty.untouched()


def test_valid_calls_without_a_gpu_are_a_loud_error(lib):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call(lib)
    for m in METHODS:
        assert c.f32(method=m) == api.SGK_ERR_NODEVICE and c.i16(method=m) == api.SGK_ERR_NODEVICE
    assert c.untouched()


@pytest.mark.parametrize("fn", ["sgk_normalise_f32_workspace_bytes", "sgk_normalise_workspace_bytes"])
def test_workspace_holds_the_statistics_workspace_and_the_records(lib, fn):
    f = getattr(lib, fn)
    for r in (0, 1, 2, 1023, 1024, 1025, 200000):
        for m in (0, 1, 3, 4, 5000, 3000001, 0x7fffffff):
            stat = int(lib.sgk_stat_f32_workspace_bytes(r, r * m, m))
            got = int(f(r, r * m, m))
            assert got == (stat + 15) // 16 * 16 + 16 * r, (fn, r, m)
            assert got % 16 == 0 and got > 0


def test_job_set_normalise_refuses_a_bad_method(lib):
    """a job needs a device: without one only the null job can be asked (tests/test_gpu_normalise.py asks a real one)"""
    for m in (0, 1, 2, 3, -1):
        assert lib.sgk_job_set_normalise(None, m) == api.SGK_ERR_ARG
    if api.device_count() > 0:
        job = api.Job(0)
        for m in (3, -1, 256):
            with pytest.raises(api.SigtkGpuError):
                job.set_normalise(m)
        for m in (1, 2, 0):
            job.set_normalise(m)
        job.close()


# ------------------------------------------------------------------------------------------------ the command line

def _run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True)


def _refused_unopened(p, word):
    return p.returncode == 1 and word in p.stderr and "cannot open" not in p.stderr and "Error in opening" not in p.stderr


def test_cli_refuses_an_unknown_method_before_opening_a_file(cli):
    for bad in ("mad", "", "ZSCORE", "zscore,medmad", "1"):
        p = _run(cli, "pa", "--normalise", bad, NOFILE)
        assert _refused_unopened(p, "--normalise") and "zscore" in p.stderr and p.stdout == "", (bad, p.stderr)
    for good in ("zscore", "medmad"):   # a known method gets as far as the file
        p = _run(cli, "pa", "--normalise", good, NOFILE)
        assert p.returncode != 0 and "cannot open" in p.stderr


def test_cli_refuses_normalise_with_gpu_text(cli):
    for args in (("--normalise", "zscore", "--gpu-text"), ("--gpu-text", "--normalise", "medmad")):
        p = _run(cli, "pa", *args, NOFILE)
        assert _refused_unopened(p, "--gpu-text") and "--normalise" in p.stderr and p.stdout == ""


def test_cli_normalise_belongs_to_pa(cli):
    for tool in ("event", "stat", "jnn", "prefix"):
        p = _run(cli, tool, "--normalise", "zscore", NOFILE)
        assert _refused_unopened(p, "--normalise"), (tool, p.stderr)
    p = _run(cli, "pa", "-h")
    assert p.returncode == 0 and "--normalise zscore|medmad" in p.stdout
    p = _run(cli, "stat", "-h")
    assert p.returncode == 0 and "--normalise" not in p.stdout


def test_cli_without_a_device_fails_as_pa_does(cli):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    plain = _run(cli, "pa", SP1)
    assert plain.returncode != 0 and "no usable GPU" in plain.stderr
    for m in ("zscore", "medmad"):
        p = _run(cli, "pa", "--normalise", m, SP1)
        assert p.returncode == plain.returncode and "no usable GPU" in p.stderr
        assert p.stdout.replace("norm", "pa") == plain.stdout
