"""CPU: the yardstick and the host side of the caller-supplied segmenter parameters (no GPU needed).

The numpy model of jnnv2 with a window equals the reference's recorded answers (tests/golden/segmenter_params.json) and,
where oracle/_ref is built, the reference itself; the recorded cases cover the edges the GPU test relies on; the new
symbols are declared; every bound of the domain is refused before a device is touched."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import segmenter_params_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("sgk_jnn_param", "sgk_prefix_param", "sgk_prefix_params_preset", "sgk_jnnv2_param", "sgk_find_polya_param",
               "sgk_job_set_jnn_params", "sgk_job_set_prefix_params", "sgk_prefix_route")


@pytest.fixture(scope="module")
def gold():
    return M.load_golden()


def test_the_grid_is_the_issue_s(gold):
    assert M.WINDOWS == (2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1999, 2001, 4096, 13981)
    for w in M.WINDOWS:
        extras = {e for e, _, _ in gold["windows"][str(w)]["reads"]}
        assert extras == {1, 2, 1023, 1024, 1025, 3000}, w
        assert max(w + e for e in extras) <= 60000


def test_model_equals_the_recorded_reference_and_covers_the_edges(gold):
    seen, n_cases, n_real = set(), 0, 0
    for w in M.WINDOWS:
        reads = M.grid_reads(gold, w)
        raws = [M.gen_read(*r) for r in reads]
        fls = [M.flags(raw, w, gold["std_scale"]) for raw in raws]
        for v, row in zip(M.grid_variants(gold, w), gold["windows"][str(w)]["answers"]):
            assert v.lo >= 1 and v.hi >= v.lo and v.seg_dist >= 0
            for r, raw, fl, want in zip(reads, raws, fls, row):
                ans, tags = M.jnnv2_model(raw, v, fl)
                assert list(ans) == want, (w, v, r)
                seen |= tags
                n_cases += 1
                n_real += 0 if M.trivial(ans) else 1
    for goal in ("open_at_0", "close_on_last", "open_at_end", "straddles_tile", "straddles_lane", "end==0",
                 "merge_at_seg_dist-1", "no_merge_at_seg_dist", "len==lo-1", "len==lo", "len==hi", "len==hi+1"):
        assert goal in seen, goal
    assert 2 * n_real >= n_cases, (n_real, n_cases)      # at least half of the cases have an answer
    assert (n_cases, n_real) == (gold["n_cases"], gold["n_with_answer"])


def test_model_equals_the_reference_itself(gold, reflib):
    if reflib is None:
        pytest.skip("oracle/_ref is not built")
    from oracle.oracle import _JnnPair, _Jnnv2Param, _p
    f = reflib.lib.jnnv2
    f.restype = _JnnPair
    f.argtypes = [C.POINTER(C.c_int16), C.c_int64, _Jnnv2Param]
    rng = np.random.default_rng(5)
    for w in (2, 17, 1000, 2000, 4096, M.WINDOW_MAX):
        for k in range(3):
            raw = M.gen_read(w, int(rng.integers(1, 4000)), 100 + k)
            for v in M.variants_for(w, raw, 0.7):
                r = f(_p(raw, C.c_int16), raw.size, _Jnnv2Param(v.std_scale, v.seg_dist, v.window, 0.0, v.hi, v.lo))
                assert (int(r.x), int(r.y)) == M.jnnv2_model(raw, v)[0], (w, k, v)


def _jnn_answers(lib, gold):
    """[set][read] = [xs, ys] of jnn_raw_param (the oracle's, or the reference's) on the seeded reads"""
    assert [list(r) for r in M.JNN_READS] == gold["jnn"]["reads"]
    reads = M.jnn_reads()
    out = []
    for kw in M.JNN_SETS:
        p = lib.jnn_param(**kw)
        out.append([[v.tolist() for v in lib.jnn_raw_param(raw, p)] for raw in reads])
    return out


def _polya_answers(lib, gold):
    """[set][read] = first segment of jnn_pa (the oracle's, or the reference's) at the model's thresholds"""
    cat = M.polya_reads()
    assert [k.name for k in cat] == gold["polya"]["reads"]
    sets = M.polya_sets(cat)
    assert [list(q) for q in sets] == gold["polya"]["sets"]      # (floats written by repr: they come back bit for bit)
    adaptors = [M.jnnv2_model(k.raw, M.POLYA_ADAPTOR)[0] for k in cat]
    out = []
    for q in sets:
        row = []
        for k, ad in zip(cat, adaptors):
            inp = M.polya_inputs(k, q, ad)
            row.append(list(M.polya_first(lib, inp[0], inp[1], inp[2], q)) if inp is not None else [-1, -1])
        out.append(row)
    return out


def test_jnn_sets_oracle_equals_the_recorded_reference(gold, oracle):
    """every jnn set of the GPU tests -- window 32 / error 40 / corrector 17 among them -- on the seeded reads: the
    oracle's segments are those the reference's own jnn_raw returned when the golden was recorded"""
    got = _jnn_answers(oracle, gold)
    assert got == gold["jnn"]["segments"]
    assert all(sum(len(r[0]) for r in row) > 0 for row in got)


def test_polya_sets_model_equals_the_recorded_reference(gold, oracle):
    """every polyA set of the GPU tests (stall_len 0.5, error at the corrector, shift / band one ulp off, bands on a
    sample) on the catalogue's RNA reads: the model's thresholds and the oracle's jnn_pa give the first segments the
    reference's own jnn_pa returned when the golden was recorded"""
    got = _polya_answers(oracle, gold)
    assert got == gold["polya"]["first"]
    assert sum(1 for row in got for a in row if a[1] > 0) >= len(got)
    # the sets are told apart by the reads: one ulp of band on a sample changes an answer, as does each structural set
    assert len({json.dumps(row) for row in got}) >= 8


def test_jnn_and_polya_sets_against_the_reference_itself(gold, reflib):
    if reflib is None:
        pytest.skip("oracle/_ref is not built")
    assert _jnn_answers(reflib, gold) == gold["jnn"]["segments"]
    assert _polya_answers(reflib, gold) == gold["polya"]["first"]


def test_model_with_window_2000_is_the_catalogue_s_model():
    import prefix_cases as P
    for k in P.shim_cases():
        want = P.jnnv2_model(k.raw, k.p)[0]
        assert M.jnnv2_model(k.raw, M.AdaptW(k.p.std_scale, k.p.seg_dist, 2000, k.p.hi, k.p.lo))[0] == want, k.name


def test_prefix_steps_with_the_presets_are_the_oracle_s_prefix(oracle):
    """the composition (adaptor, meanf of the pA region, (m_a + shift) +- band, first segment) with the preset sets is
    oracle.prefix -- the port of cfunc.c:169-216 that tests/test_oracle_vs_ref.py holds to the reference -- on every RNA
    read of the catalogue: the order of the band's two roundings included"""
    n = 0
    for k in M.polya_reads():
        with np.errstate(all="ignore"):
            e = oracle.prefix(k.raw, k.dig, k.off, k.rng, 1, 0)
            wa, wp = M.prefix_model(oracle, k.raw, k.dig, k.off, k.rng, 1, M.POLYA_ADAPTOR, M.POLYA_PRESET)
        assert wa == (e.adapt_x, e.adapt_y) and wp == (e.polya_x, e.polya_y), k.name
        n += 1 if e.polya_y > 0 else 0
    assert n > 10


def test_polya_thresholds_round_once_per_operator():
    q = M.POLYA_PRESET._replace(shift=30.1, band=19.9)
    top, bot = M.polya_thresholds(np.float32(88.123456), q)
    mid = np.float32(np.float32(88.123456) + np.float32(30.1))
    assert top == np.float32(mid + np.float32(19.9)) and bot == np.float32(mid - np.float32(19.9))
    assert top.dtype == np.float32 and bot.dtype == np.float32


# ---------------------------------------------------------------- the public surface
def test_symbols_are_declared_and_listed():
    from sigtk_amd import api
    header = open(os.path.join(ROOT, "include", "sigtk_gpu.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in api.ABI_SYMBOLS, s
    assert "sgk_prefix_params_t" in header and "SGK_PREFIX_PARAMS_GENERIC" in header
    assert C.sizeof(api.PrefixParams) == 72


@pytest.fixture(scope="module")
def lib():
    from sigtk_amd import api
    api.load_library()
    return api._param_lib()


def _jnn(api, **kw):
    d = dict(std_scale=0.75, corrector=50, seg_dist=50, window=150, stall_len=0.25, error=5, top=0.0, bot=0.0)
    d.update(kw)
    return api.JnnParam(d["std_scale"], d["corrector"], d["seg_dist"], d["window"], d["stall_len"], d["error"], d["top"], d["bot"])


def test_jnn_domain(lib):
    from sigtk_amd import api
    chk = lambda **kw: lib.sgk_jnn_params_check(C.byref(_jnn(api, **kw)))
    assert chk() == api.SGK_OK
    assert lib.sgk_jnn_params_check(None) == api.SGK_ERR_ARG
    for ok in (dict(window=32), dict(window=1 << 24), dict(corrector=1), dict(error=0), dict(seg_dist=0), dict(stall_len=0.0),
               dict(std_scale=-1.0, top=math.nan, bot=math.inf), dict(std_scale=0.0), dict(window=32, error=40, corrector=17)):
        assert chk(**ok) == api.SGK_OK, ok
    for bad in (dict(window=31), dict(window=(1 << 24) + 1), dict(window=-5), dict(corrector=0), dict(error=-1), dict(seg_dist=-1),
                dict(stall_len=-0.5), dict(stall_len=math.nan), dict(stall_len=math.inf), dict(std_scale=math.nan),
                dict(std_scale=math.inf)):
        assert chk(**bad) == api.SGK_ERR_ARG, bad
        # ... and by the batch call before it looks at anything else
        assert lib.sgk_jnn_param(None, C.byref(_jnn(api, **bad)), None, None, None, None, None, 0, None, None) == api.SGK_ERR_ARG
        assert lib.sgk_job_set_jnn_params(None, C.byref(_jnn(api, **bad))) == api.SGK_ERR_ARG


def _prefix(api, adaptor=None, polya=None, **kw):
    p = api.PrefixParams.preset(1, 0)
    for k, v in (adaptor or {}).items():
        setattr(p.adaptor, k, v)
    for k, v in (polya or {}).items():
        setattr(p.polya, k, v)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_prefix_presets_and_routes(lib):
    from sigtk_amd import api
    p0, p2 = api.PrefixParams.preset(1, 0), api.PrefixParams.preset(1, 2)
    assert (p0.adaptor.window, p0.adaptor.seg_dist, p0.adaptor.hi_thresh, p0.adaptor.lo_thresh) == (2000, 1500, 200000, 2000)
    assert np.float32(p0.adaptor.std_scale) == np.float32(0.5) and np.float32(p2.adaptor.std_scale) == np.float32(0.7)
    assert p2.adaptor.lo_thresh == 500
    assert (p0.polya.corrector, p0.polya.seg_dist, p0.polya.window, p0.polya.stall_len, p0.polya.error) == (50, 200, 250, 1.0, 30)
    assert (p0.shift, p0.band, p0.flags) == (30.0, 20.0, 0)
    assert lib.sgk_prefix_params_preset(1, 7, C.byref(p0)) == api.SGK_ERR_ARG
    assert lib.sgk_prefix_params_preset(1, 0, None) == api.SGK_ERR_ARG
    assert p0.route() == 0 and p2.route() == 0
    A, PW, PL = api.PREFIX_ROUTE_ADAPTOR_PARAM, api.PREFIX_ROUTE_POLYA_WAVE_PARAM, api.PREFIX_ROUTE_POLYA_LANE_PARAM
    assert _prefix(api, flags=api.PREFIX_PARAMS_GENERIC).route() == A
    assert _prefix(api, adaptor=dict(window=1999)).route() == A
    assert _prefix(api, adaptor=dict(lo_thresh=1999)).route() == A       # any field off the presets
    assert _prefix(api, adaptor=dict(stall_len=0.0)).route() == 0         # ... but the one the reference ignores
    assert _prefix(api, shift=float(np.nextafter(np.float32(30), np.float32(31)))).route() == PW
    assert _prefix(api, polya=dict(error=49)).route() == PW
    assert _prefix(api, polya=dict(error=50)).route() == PL               # error == corrector: the correction can fire
    assert _prefix(api, polya=dict(stall_len=0.5)).route() == PL
    assert _prefix(api, adaptor=dict(window=2), polya=dict(stall_len=0.5)).route() == A | PL
    assert lib.sgk_prefix_route(None) == api.SGK_ERR_ARG


def test_prefix_domain(lib):
    from sigtk_amd import api
    for ok in (dict(adaptor=dict(window=2)), dict(adaptor=dict(window=13981)), dict(adaptor=dict(lo_thresh=1, hi_thresh=1)),
               dict(adaptor=dict(seg_dist=0)), dict(adaptor=dict(stall_len=math.nan)), dict(polya=dict(window=32)),
               dict(polya=dict(top=math.nan, bot=math.nan, std_scale=math.nan)), dict(band=0.0), dict(shift=-3.0e38)):
        assert lib.sgk_prefix_params_check(C.byref(_prefix(api, **ok))) == api.SGK_OK, ok
    bads = [dict(adaptor=dict(window=1)), dict(adaptor=dict(window=0)), dict(adaptor=dict(window=13982)), dict(adaptor=dict(window=-2000)),
            dict(adaptor=dict(lo_thresh=0)), dict(adaptor=dict(lo_thresh=-1)), dict(adaptor=dict(hi_thresh=1999)),
            dict(adaptor=dict(seg_dist=-1)), dict(adaptor=dict(std_scale=math.nan)), dict(adaptor=dict(std_scale=-math.inf)),
            dict(polya=dict(window=31)), dict(polya=dict(window=(1 << 24) + 1)), dict(polya=dict(corrector=0)),
            dict(polya=dict(error=-1)), dict(polya=dict(seg_dist=-1)), dict(polya=dict(stall_len=-1.0)),
            dict(polya=dict(stall_len=math.nan)), dict(shift=math.nan), dict(shift=math.inf), dict(band=math.nan),
            dict(band=math.inf), dict(band=-1.0), dict(flags=2), dict(reserved=1)]
    for bad in bads:
        p = _prefix(api, **bad)
        assert lib.sgk_prefix_params_check(C.byref(p)) == api.SGK_ERR_ARG, bad
        assert lib.sgk_prefix_route(C.byref(p)) == api.SGK_ERR_ARG, bad
        assert lib.sgk_prefix_param(None, 1, C.byref(p), None, None, 0, None, None) == api.SGK_ERR_ARG, bad
        assert lib.sgk_job_set_prefix_params(None, C.byref(p)) == api.SGK_ERR_ARG, bad
    assert lib.sgk_prefix_param(None, 1, None, None, None, 0, None, None) == api.SGK_ERR_ARG


def test_per_read_calls_refuse_before_a_device(lib):
    from sigtk_amd import api
    raw = np.zeros(5000, dtype=np.int16)
    for bad in (dict(window=1), dict(window=13982), dict(lo_thresh=0), dict(hi_thresh=3, lo_thresh=4), dict(seg_dist=-1),
                dict(std_scale=math.nan)):
        d = dict(std_scale=0.5, seg_dist=1500, window=2000, stall_len=1.0, hi_thresh=200000, lo_thresh=2000)
        d.update(bad)
        xy, rc = api.shim_jnnv2_param(raw, api.Jnnv2Param(d["std_scale"], d["seg_dist"], d["window"], d["stall_len"], d["hi_thresh"],
                                                          d["lo_thresh"]))
        assert xy == (-1, -1) and rc == api.SGK_ERR_ARG, bad
    # a read no longer than the window: (-1, -1) and no error, as the reference
    xy, rc = api.shim_jnnv2_param(raw[:100], api.Jnnv2Param(0.5, 10, 100, 0.0, 1000, 1))
    assert xy == (-1, -1) and rc == api.SGK_OK
    L = api._shim_lib()
    p = L.sgk_find_polya_param(None, 0, 1.0, 0.0, _jnn(api, window=31))
    assert (p.x, p.y) == (-1, -1) and L.sgk_shim_status() == api.SGK_ERR_ARG
