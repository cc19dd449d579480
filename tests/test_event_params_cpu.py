"""CPU: event detection with caller-supplied detector parameters -- the yardstick (tests/event_params_model.py) is pinned
to the oracle on the presets, the order and spacing of the peaks that the arena capacity and the peak bitmap rest on hold
for the parameter grid, the host-only ABI (presets, domain check) and the CLI's --detector parsing."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import event_cases as E
import event_params_model as M
from sigtk_amd import api, build

F = np.float32


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def cat():
    return E.catalogue()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(api.LIB_PATH):
        build.build_lib()
    return api.load_library()


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI):
        build.build_lib()
        build.build_cli()
    return build.CLI


def test_model_equals_getevents_on_the_presets(oracle, cat):
    """the composition with free parameters is oracle.getevents for both presets, field by field (bit patterns of mean
    and stdv): on every catalogue read and pA array, and on 200 seeded random reads"""
    pas = [(k.name, oracle.pa(k.raw, *E.SCALE)) for k in cat]
    pas += [(k.name, k.pa) for k in E.pa_cases() if np.isfinite(k.pa).all()]
    pas += [("random_%d" % i, oracle.pa(r, *E.SCALE)) for i, r in enumerate(M.random_reads(20240, 200, 3000))]
    n_events = 0
    for name, pa in pas:
        for rna in (0, 1):
            got = M.events_pa(oracle, pa, M.PRESETS[rna])
            if pa.size == 0:
                assert got.start.size == 0
                continue
            want = oracle.getevents(pa, rna)
            assert got.start.size == want.start.size, (name, rna)
            assert np.array_equal(got.start.astype(np.uint64), want.start), (name, rna)
            assert np.array_equal(got.length.astype(F), want.length), (name, rna)
            assert np.array_equal(_bits(got.mean), _bits(want.mean)), (name, rna)
            assert np.array_equal(_bits(got.stdv), _bits(want.stdv)), (name, rna)
            n_events += got.start.size
    assert n_events > 10000


#: beside the grid: the sets next to the corner the domain excludes (a long window of 2 or 3 that differs from the short
#: one: there the long detector emits a peak 2 in front of a short peak that opens at the emitting index)
EDGE_SETS = [M.P(2, 4, 0.5, 0.5, 0.0), M.P(16, 4, 1.0, 0.2, 0.0), M.P(5, 4, 0.0, 0.0, 0.0), M.P(3, 3, 1.0, 0.2, 0.0),
             M.P(2, 2, 2.0, 0.0, 0.0), M.P(3, 5, 3.0, 0.5, float(F(0.1)))]
EXCLUDED = [M.P(5, 2, 1.0, 0.2, 0.0), M.P(5, 3, 1.0, 0.2, 0.0), M.P(2, 3, 0.5, 0.5, 0.0), M.P(3, 2, 0.5, 0.5, 0.0)]


def test_the_excluded_corner_is_where_spacing_fails(oracle):
    """why sgk_event_params_check refuses a long window of 2 or 3 beside another short window: peaks 2 apart"""
    pas = [oracle.pa(r, *E.SCALE) for r in M.random_reads(5, 600, 400)]
    for p in EXCLUDED:
        closest = min((int(np.diff(pk).min()) for pk in (M.peaks_of_pa(oracle, pa, p) for pa in pas) if pk.size > 1))
        assert closest == 2, p


def test_peaks_are_ordered_and_spaced(oracle, cat):
    """What sgk_event_slots_for and the peak bitmap rest on, for every set of the grid: the oracle's peaks are strictly
    increasing, consecutive peaks at least 3 apart, the first at least 1, and a read has at most n / 3 + 2 events."""
    reads = [k.raw for k in cat] + M.random_reads(777, 2000, 600)
    grid = M.GRID + EDGE_SETS
    pas = [oracle.pa(r, *E.SCALE) for r in reads]
    sums = [oracle.prefix_sums(pa) for pa in pas]
    total = {p: 0 for p in grid}
    tcache = {}
    for p in grid:
        for k, (s, q) in enumerate(sums):
            n = s.size - 1
            for w in (p.w1, p.w2):
                if (k, w) not in tcache:
                    tcache[(k, w)] = oracle.tstat(s, q, w)
            pk = M.peaks(oracle, tcache[(k, p.w1)], tcache[(k, p.w2)], p)
            total[p] += pk.size
            if pk.size:
                assert pk[0] >= 1, (p, k)
                assert pk[-1] < n, (p, k)
                d = np.diff(pk)
                assert (d > 0).all(), (p, k, "order")
                assert (d >= 3).all(), (p, k, "spacing", pk[:-1][d < 3][:4])
            assert pk.size + 1 <= n // 3 + 2, (p, k)
    # every set finds something on these reads (a grid set without peaks would check nothing)
    assert all(v > 100 for v in total.values()), total


def _params(w1, w2, t1, t2, ph, flags=0):
    return api.EventParams(w1, w2, t1, t2, ph, flags)


def test_host_abi_presets_and_domain(lib):
    assert C.sizeof(api.EventParams) == 32
    for rna in (0, 1):
        got = api.EventParams.preset(rna)
        want = M.PRESETS[rna]
        assert (got.window_length1, got.window_length2) == (want.w1, want.w2)
        assert _bits([got.threshold1, got.threshold2, got.peak_height]).tolist() == \
            _bits([want.thr1, want.thr2, want.ph]).tolist()
        assert got.flags == 0 and list(got.reserved) == [0, 0]
    assert lib.sgk_event_params_preset(0, None) == api.SGK_ERR_ARG
    for p in M.GRID:
        _params(*p).check()
        _params(*p, flags=api.SGK_EVENT_PARAMS_GENERIC).check()
    assert lib.sgk_event_params_check(None) == api.SGK_ERR_ARG
    ok = M.PRESETS[0]
    for w in (0, 1, api.SGK_EVENT_W_MAX + 1):
        assert lib.sgk_event_params_check(C.byref(_params(w, ok.w2, ok.thr1, ok.thr2, ok.ph))) == api.SGK_ERR_ARG
        assert lib.sgk_event_params_check(C.byref(_params(ok.w1, w, ok.thr1, ok.thr2, ok.ph))) == api.SGK_ERR_ARG
    for p in EDGE_SETS:
        _params(*p).check()
    for p in EXCLUDED:
        assert lib.sgk_event_params_check(C.byref(_params(*p))) == api.SGK_ERR_ARG, p
    for w in (2, api.SGK_EVENT_W_MAX):
        assert lib.sgk_event_params_check(C.byref(_params(w, w, ok.thr1, ok.thr2, ok.ph))) == api.SGK_OK
    for bad in (math.nan, math.inf, -math.inf, -1.0, -1e-30):
        for k in range(3):
            f = [ok.thr1, ok.thr2, ok.ph]
            f[k] = bad
            assert lib.sgk_event_params_check(C.byref(_params(ok.w1, ok.w2, *f))) == api.SGK_ERR_ARG, (bad, k)
    assert lib.sgk_event_params_check(C.byref(_params(3, 6, M.FLT_MAX, 0.0, 0.0))) == api.SGK_OK
    assert lib.sgk_event_params_check(C.byref(_params(3, 6, 1.0, 1.0, 1.0, flags=2))) == api.SGK_ERR_ARG
    # out of domain: no workspace size, and the launch entry points refuse before they look at anything else
    bad = _params(1, 6, 1.0, 1.0, 1.0)
    assert lib.sgk_event_workspace_bytes_param(10, 1000, 100, None, C.byref(bad)) == 0
    assert lib.sgk_event_param(None, C.byref(bad), None, None, None, None, 0, None, None) == api.SGK_ERR_ARG
    assert lib.sgk_event_pa_param(None, None, None, 1, 10, 16, C.byref(bad), None, None, None, None, 0, None, None) == api.SGK_ERR_ARG


def test_workspace_of_the_generic_kernel_ignores_the_batch_total(lib):
    """the rule of the header: bounded by the persistent workgroups and the longest read, not by the samples"""
    p = _params(5, 9, 1.4, 3.0, 0.2)
    a = lib.sgk_event_workspace_bytes_param(100000, 10 ** 9, 20000, None, C.byref(p))
    b = lib.sgk_event_workspace_bytes_param(100000, 2 * 10 ** 9, 20000, None, C.byref(p))
    assert a == b and a > 0
    per = (16 * 20001 + 8 * (20000 // 64 + 2) + 63) // 64 * 64
    assert a == 64 + (4 * 100000 + 512 + 63) // 64 * 64 + 1024 * per
    # ... with the workgroups lowered so that their scratch stays under 2 GiB
    per = (16 * 1000001 + 8 * (1000000 // 64 + 2) + 63) // 64 * 64
    c = lib.sgk_event_workspace_bytes_param(100000, 10 ** 11, 1000000, None, C.byref(p))
    assert c == 64 + (4 * 100000 + 512 + 63) // 64 * 64 + ((2 << 30) // per) * per and c < (2 << 30) + (1 << 20)
    small = lib.sgk_event_workspace_bytes_param(3, 300, 100, None, C.byref(p))
    assert small == 64 + (12 + 512 + 63) // 64 * 64 + 3 * ((16 * 101 + 8 * 3 + 63) // 64 * 64)
    # a preset without the flag is sgk_event_opt's workspace
    d = api.EventParams.preset(0)
    assert lib.sgk_event_workspace_bytes_param(1000, 10 ** 7, 20000, None, C.byref(d)) == \
        lib.sgk_event_workspace_bytes_opt(1000, 10 ** 7, 20000, None)


def test_chunk_constant_mirrors_the_header():
    """api.EVENT_GENERIC_CHUNK_SAMPLES, from which the GPU tests take the lengths around a change of the chunk length, is
    the kernel's GENERIC_CHUNK_SAMPLES"""
    import re
    hdr = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc", "event_generic.h")
    m = re.findall(r"constexpr\s+int\s+GENERIC_CHUNK_SAMPLES\s*=\s*(\d+)\s*;", open(hdr).read())
    assert len(m) == 1 and int(m[0]) == api.EVENT_GENERIC_CHUNK_SAMPLES
    assert "GENERIC_CHUNK_SAMPLES - 1) / GENERIC_CHUNK_SAMPLES" in open(hdr).read()   # chunk_len steps at its multiples


BLOW5 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp1_dna.blow5")


@pytest.mark.parametrize("arg", [
    "3,6,1.4,9",                 # 4 fields
    "3,6,1.4,9,0.2,1",           # 6 fields
    "3,,1.4,9,0.2", ",6,1.4,9,0.2", "3,6,1.4,9,", "",   # empty fields
    "3x,6,1.4,9,0.2", "3,6,1.4abc,9,0.2", "3,6,1.4,9,0.2 ", "3.0,6,1.4,9,0.2",   # text behind a number
    "1,6,1.4,9,0.2", "3,65,1.4,9,0.2", "0,0,1,1,1", "3,6,-1.4,9,0.2", "3,6,1.4,nan,0.2", "3,6,1.4,9,inf",
    "-3,6,1.4,9,0.2", "4294967299,6,1.4,9,0.2", "3,6,1e39,9,0.2", "5,3,1.4,9,0.2",   # out of domain
])
def test_cli_refuses_a_bad_detector(cli, arg):
    """a message and exit 1 before any file or device is opened: the file named here does not exist"""
    p = subprocess.run([cli, "event", "--detector", arg, "/nonexistent/reads.blow5"], capture_output=True, text=True)
    assert p.returncode == 1, (arg, p.stderr)
    assert "--detector" in p.stderr and "cannot open" not in p.stderr and p.stdout == "", (arg, p.stderr)


def test_cli_detector_is_for_event_and_leaves_the_usage_alone(cli):
    p = subprocess.run([cli, "stat", "--detector", "3,6,1.4,9,0.2", "/nonexistent/reads.blow5"], capture_output=True, text=True)
    assert p.returncode == 1 and "--detector" in p.stderr and "cannot open" not in p.stderr
    # a good list gets as far as opening the file
    p = subprocess.run([cli, "event", "--detector", "5,9,1.4,3,0.2", "/nonexistent/reads.blow5"], capture_output=True, text=True)
    assert p.returncode == 1 and "cannot open" in p.stderr
    p = subprocess.run([cli, "event", "-h"], capture_output=True, text=True)
    assert p.returncode == 0 and "--detector" not in p.stdout
