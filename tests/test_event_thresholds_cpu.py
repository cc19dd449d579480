"""CPU: the presets' kernels with run-time thresholds (SGK_EVENT_PARAMS_PRESET_KERNELS).  Before any GPU comparison
means anything the reads of tests/event_threshold_cases.py must be able to tell a run-time threshold from the preset's
constant: threshold2 decides on reads made for it, and every tuned set changes events against its preset.  Then the
host-only part of the feature: the route query, the domain check with the new flag, the workspace rule; and the order and
spacing of the peaks that the arena capacity rests on, for the fast-domain sets."""
import ctypes as C
import os

import numpy as np
import pytest

import event_params_model as M
import event_threshold_cases as TC
from sigtk_amd import api, build

F = np.float32
FLT_MAX = M.FLT_MAX


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(api.LIB_PATH):
        build.build_lib()
    return api.load_library()


class _Model:
    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, rd, p):
        key = (rd.name, p)
        if key not in self.memo:
            self.memo[key] = M.events_raw(self.oracle, rd.raw, *rd.scale, p)
        return self.memo[key]


@pytest.fixture(scope="module")
def model(oracle):
    return _Model(oracle)


# ------------------------------------------------------------------------------------------------ 1. threshold2 decides

@pytest.mark.parametrize("rna", [0, 1])
def test_threshold2_decides(model, rna):
    """with the short detector out of the way (threshold1 = FLT_MAX) the events of threshold2 = 9, 12, 20 and FLT_MAX
    differ pairwise along that chain on at least three of the reads made for it -- the long detector's peak values lie on
    both sides of every tested threshold, which no catalogue read offers"""
    pre = M.PRESETS[rna]
    chain = [M.P(pre.w1, pre.w2, FLT_MAX, t2, pre.ph) for t2 in (9.0, 12.0, 20.0, FLT_MAX)]
    assert all(p in TC.FAST for p in chain[:3])     # the GPU tests run these very sets
    reads = TC.thr2_reads()
    for a, b in zip(chain, chain[1:]):
        changed = [rd.name for rd in reads if TC.differ(model(rd, a), model(rd, b))]
        print("windows %d/%d threshold2 %g -> %g: %d of %d reads change" % (pre.w1, pre.w2, a.thr2, b.thr2, len(changed), len(reads)))
        assert len(changed) >= 3, (a, b, changed)
    # fewer and fewer boundaries, and something left to lose at every step
    for rd in reads:
        n = [model(rd, p).start.size for p in chain]
        assert n[0] >= n[1] >= n[2] >= n[3] == 1, (rd.name, n)


# ------------------------------------------------------------------------------------------------ 2. tuned != preset

@pytest.mark.parametrize("p", TC.FAST, ids=[TC.ident(p) for p in TC.FAST])
def test_every_tuned_set_is_told_apart_from_its_preset(model, p):
    """at least three reads of the set's inputs have other events than with the preset: a kernel that ignored its run-time
    thresholds would fail there"""
    pre = TC.preset_of(p)
    assert p != pre
    changed = [rd.name for rd in TC.reads() if TC.differ(model(rd, p), model(rd, pre))]
    print("%s: %d of %d reads differ from the preset" % (TC.ident(p), len(changed), len(TC.reads())))
    assert len(changed) >= 3, (p, changed)


def test_one_ulp_of_threshold1_decides(oracle, model):
    """the reads made for nextafter(1.4f): a short peak whose value IS that float, above the preset's threshold and not
    above the tuned one -- each loses exactly that boundary"""
    tuned = TC.FAST_DNA[1]
    assert np.float32(tuned.thr1).view(np.uint32) == np.float32(1.4).view(np.uint32) + 1
    reads = TC.ulp_reads()
    assert len(reads) >= 3
    for rd in reads:
        pa = oracle.pa(rd.raw, *rd.scale)
        t1 = oracle.tstat(*oracle.prefix_sums(pa), 3)
        a, b = model(rd, M.PRESETS[0]), model(rd, tuned)
        lost = sorted(set(a.start.tolist()) - set(b.start.tolist()))
        assert len(lost) == 1 and set(b.start.tolist()) < set(a.start.tolist()), (rd.name, a.start, b.start)
        assert np.float32(t1[lost[0]]).view(np.uint32) == np.float32(tuned.thr1).view(np.uint32), (rd.name, t1[lost[0]])


# ------------------------------------------------------------------------------------------------ 3. the route query

def _params(p, flags=0):
    return api.EventParams(p.w1, p.w2, p.thr1, p.thr2, p.ph, flags)


GEN, FAST = api.SGK_EVENT_PARAMS_GENERIC, getattr(api, "SGK_EVENT_PARAMS_PRESET_KERNELS", None)


def test_route_query(lib):
    assert FAST == 4 and (api.SGK_EVENT_ROUTE_PRESET, api.SGK_EVENT_ROUTE_PRESET_WINDOWS, api.SGK_EVENT_ROUTE_GENERIC) == (0, 1, 2)
    route = lambda p, flags: lib.sgk_event_params_route(C.byref(_params(p, flags)))
    for p in TC.FAST:
        for flags in (0, GEN, FAST, GEN | FAST):
            assert lib.sgk_event_params_check(C.byref(_params(p, flags))) == api.SGK_OK, (p, flags)
        assert route(p, 0) == api.SGK_EVENT_ROUTE_GENERIC, p               # opt-in: nothing changes without the flag
        assert route(p, FAST) == api.SGK_EVENT_ROUTE_PRESET_WINDOWS, p
        assert route(p, GEN) == api.SGK_EVENT_ROUTE_GENERIC, p
        assert route(p, GEN | FAST) == api.SGK_EVENT_ROUTE_GENERIC, p      # both flags mean generic
        assert api.event_params_route(_params(p, FAST)) == api.SGK_EVENT_ROUTE_PRESET_WINDOWS
        assert _params(p).preset_kernels().route() == api.SGK_EVENT_ROUTE_PRESET_WINDOWS
    for p in TC.GENERIC_WITH_FLAG + M.GRID_OFF[:5]:
        for flags in (0, GEN, FAST, GEN | FAST):
            assert route(p, flags) == api.SGK_EVENT_ROUTE_GENERIC, (p, flags)
    for rna in (0, 1):
        p = M.PRESETS[rna]
        assert route(p, 0) == route(p, FAST) == api.SGK_EVENT_ROUTE_PRESET          # the constexpr kernels, flag or not
        assert route(p, GEN) == route(p, GEN | FAST) == api.SGK_EVENT_ROUTE_GENERIC
    # threshold2 exactly 9 with another threshold1 is inside, one ulp below 9 is outside
    assert route(M.P(7, 14, 1.0, 9.0, 1.0), FAST) == api.SGK_EVENT_ROUTE_PRESET_WINDOWS
    assert route(M.P(7, 14, 1.0, TC.T9_DOWN, 1.0), FAST) == api.SGK_EVENT_ROUTE_GENERIC
    # out of domain
    assert lib.sgk_event_params_route(None) == api.SGK_ERR_ARG
    assert route(M.P(1, 6, 1.0, 9.0, 1.0), FAST) == api.SGK_ERR_ARG
    assert route(M.P(3, 6, -1.0, 9.0, 1.0), FAST) == api.SGK_ERR_ARG
    # bit 2 stays unassigned (tests/test_event_params_cpu.py has it refused), as does every bit above the flag
    assert route(M.P(3, 6, 1.0, 9.0, 1.0), 2) == api.SGK_ERR_ARG and route(M.P(3, 6, 1.0, 9.0, 1.0), 2 | FAST) == api.SGK_ERR_ARG
    assert route(M.P(3, 6, 1.0, 9.0, 1.0), 8) == api.SGK_ERR_ARG and route(M.P(3, 6, 1.0, 9.0, 1.0), 8 | FAST) == api.SGK_ERR_ARG
    with pytest.raises(Exception):
        api.event_params_route(_params(M.P(1, 6, 1.0, 9.0, 1.0), FAST))


def test_workspace_follows_the_route(lib):
    shapes = [(1000, 10 ** 7, 20000), (3, 300, 100), (10000, 10 ** 9, 100000)]
    opts = [None, api.EventOptions(1024, 1025, 16, 8, 0, 0), api.EventOptions(0, 0, 0, -1, 0, 5)]
    for nr, ns, ml in shapes:
        for o in opts:
            op = C.byref(o) if o is not None else None
            want_fast = lib.sgk_event_workspace_bytes_opt(nr, ns, ml, op)
            for p in TC.FAST:
                generic = lib.sgk_event_workspace_bytes_param(nr, ns, ml, op, C.byref(_params(p)))
                assert generic > 0 and generic == lib.sgk_event_workspace_bytes_param(nr, ns, ml, op, C.byref(_params(p, GEN | FAST)))
                assert lib.sgk_event_workspace_bytes_param(nr, ns, ml, op, C.byref(_params(p, FAST))) == want_fast
                assert generic != want_fast
            for p in TC.GENERIC_WITH_FLAG:
                assert lib.sgk_event_workspace_bytes_param(nr, ns, ml, op, C.byref(_params(p, FAST))) == \
                    lib.sgk_event_workspace_bytes_param(nr, ns, ml, op, C.byref(_params(p))) != want_fast


# ------------------------------------------------------------------------------------------------ 4. peak spacing

def test_peaks_are_ordered_and_spaced(oracle):
    """what sgk_event_slots_for and the peak bitmap rest on, for every fast-domain set on its own inputs and on 600 random
    reads: peaks strictly increasing, at least 3 apart, the first at least 1, at most n / 3 + 2 events"""
    reads = [(rd.raw, rd.scale) for rd in TC.reads()] + [(r, TC.E.SCALE) for r in M.random_reads(778, 600, 600)]
    sums = [oracle.prefix_sums(oracle.pa(raw, *sc)) for raw, sc in reads]
    tc = {}
    for p in TC.FAST:
        total = 0
        for k, (s, q) in enumerate(sums):
            n = s.size - 1
            for w in (p.w1, p.w2):
                if (k, w) not in tc:
                    tc[(k, w)] = oracle.tstat(s, q, w)
            pk = M.peaks(oracle, tc[(k, p.w1)], tc[(k, p.w2)], p)
            total += pk.size
            if pk.size:
                assert pk[0] >= 1 and pk[-1] < n, (p, k)
                d = np.diff(pk)
                assert (d > 0).all() and (d >= 3).all(), (p, k, pk[:-1][d < 3][:4])
            assert pk.size + 1 <= n // 3 + 2, (p, k)
        if p.thr2 != FLT_MAX or p.thr1 != FLT_MAX:
            assert total > 100, (p, total)
