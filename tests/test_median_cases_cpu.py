"""CPU: the median catalogue (tests/median_cases.py) covers every decision edge of every GPU form, its fixtures are the
ones recorded from the real reference (tests/golden/median_cases.json, written by tests/golden/make_golden_median_cases.py),
and the oracle the GPU tests lean on elsewhere equals them bit for bit -- the tie class included, where the pA median is
not pA(raw order statistic) but the element the reference's selection leaves at n / 2."""
import json
import os

import numpy as np
import pytest

import median_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

POSITIONS = ["k@lo-1", "k@lo", "k@lo+1", "k@lo+nb-2", "k@lo+nb-1", "k@lo+nb"]
WINDOW = POSITIONS + ["trusted", "fallback", "k_in_k2_out", "k_out_k2_in", "k_k2_other_owner", "k==acc", "k==acc+h-1",
                      "mean_in(-1,0)", "mean_in(-17,-16)", "trunc_decides", "lo_clamped_high", "lo_clamped_low"]
H32 = POSITIONS + ["trusted", "fallback", "k_in_k2_out", "k_out_k2_in", "k_k2_other_bin", "k==acc", "k==acc+h-1",
                   "mean_in(-1,0)", "mean_in(-17,-16)", "trunc_decides", "window_above_int16", "window_below_int16"]
SELECT = ["med%16==0", "med%16==15", "rank2==0", "rank2==last_of_fine_bin", "constant", "distinct>8192",
          "mirror_other_coarse_bin", "median==-32768", "median==32767"]
ANY = ["n=1", "n=2", "n=3", "n=8192", "n=8193", "n=20001", "n=65536", "n=65537", "unit<0,n_odd", "unit<0,n_even",
       "unit<0,n=2", "unit=-0", "tie"]


@pytest.fixture(scope="module")
def cases():
    return mc.cases()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "median_cases.json")))


@pytest.fixture(scope="module")
def models(cases):
    return {c.name: mc.model(c) for c in cases}


def _have(models, cases, form, keep=lambda c, m: True):
    got = set()
    for c in cases:
        m = models[c.name]
        if keep(c, m):
            got |= m[form]
    return got


def test_every_required_tag_is_carried(cases, models):
    """per form on which the tag is meaningful: the wave kernel's window (every read), the same window on the long path
    (reads of 8192 samples and more), k_median's 2048- and 8192-bin windows apart, the 32 bins of k_moments, the
    two-level select (only reads k_median's window does not settle get there), and the lengths and scales"""
    missing = []

    def need(label, want, got):
        missing.extend("%s: %s" % (label, t) for t in want if t not in got)

    need("wave", WINDOW, _have(models, cases, "wave"))
    need("long", WINDOW, _have(models, cases, "wave", lambda c, m: c.raw.size >= 8192))
    need("kmed 2048", WINDOW, _have(models, cases, "kmed", lambda c, m: "nb=2048" in m["kmed"]))
    need("kmed 8192", WINDOW, _have(models, cases, "kmed", lambda c, m: "nb=8192" in m["kmed"]))
    need("h32", H32, _have(models, cases, "h32"))
    need("select", SELECT, _have(models, cases, "select"))
    need("any", ANY, _have(models, cases, "any"))
    assert not missing, missing


def test_alignment_grid_is_complete(cases):
    """every lead 0..7 with every tail 0..7 of visit_keys, and n < head for every head > 1"""
    seen = set()
    short = set()
    for c in cases:
        head = (8 - c.lead) % 8
        n = c.raw.size
        if n < head:
            short.add(c.lead)
        else:
            seen.add((c.lead, (n - head) % 8))
    assert seen >= {(lead, t) for lead in range(8) for t in range(8)}
    assert short >= {lead for lead in range(8) if (8 - lead) % 8 > 1}
    assert max(c.raw.size for c in cases if c.lead) <= 40


def test_tie_class_is_what_the_model_says(cases):
    """a case is in the tie class iff its unit is a zero, not finite, or makes every product underflow (the catalogue's
    offsets are finite) AND raw + offset is positive, negative and exactly 0 inside the read"""
    for c in cases:
        u = mc.unit_of(c.dig, c.rng)
        under = float(abs(u)) * 40.0 < 1e-45    # every product underflows to a zero
        v = c.raw.astype(np.int64) + int(c.off)
        mixed = bool((v > 0).any() and (v < 0).any() and (v == 0).any())
        assert c.tie == (bool(u == 0 or not np.isfinite(u) or under) and mixed), c.name
        if c.tie:
            assert c.raw.size <= 4096


def test_fixtures_are_the_catalogue(cases, golden):
    assert sorted(golden["stat"]) == sorted(c.name for c in cases)
    for c in cases:
        g = golden["stat"][c.name]
        assert (g["n"], g["crc"]) == (c.raw.size, mc.crc(c.raw)), c.name
    fl = mc.float_cases()
    assert sorted(golden["float"]) == sorted(k.name for k in fl)
    for k in fl:
        g = golden["float"][k.name]
        assert (g["n"], g["crc"]) == (k.x.size, mc.crc(k.x)), k.name
    rg = mc.region_cases()
    assert sorted(golden["region"]) == sorted(k.name for k in rg)
    for k in rg:
        g = golden["region"][k.name]
        assert (g["n"], g["crc"]) == (k.raw.size, mc.crc(k.raw)), k.name
        assert g["adapt"][1] > 0, k.name


def same_bits(got, want_bits):
    """bit for bit; two NaNs: the same sign bit"""
    gb = int(np.float32(got).view(np.uint32))
    if gb == want_bits:
        return True
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000  # noqa: E731
    return nan(gb) and nan(want_bits) and (gb >> 31) == (want_bits >> 31)


def test_oracle_equals_the_reference(oracle, cases, golden):
    bad = []
    with np.errstate(all="ignore"):
        for c in cases:
            g = golden["stat"][c.name]
            s = oracle.stat(c.raw, c.dig, c.off, c.rng)
            if int(s[4]) != g["raw_median"] or not all(same_bits(s[i], b) for i, b in zip((0, 1, 2, 3, 5), g["bits"])):
                bad.append(c.name)
        for k in mc.float_cases():
            if not all(same_bits(v, b) for v, b in zip(oracle.statf(k.x), golden["float"][k.name]["bits"])):
                bad.append("f:" + k.name)
        for k in mc.region_cases():
            g = golden["region"][k.name]
            pa = oracle.pa(k.raw, k.dig, k.off, k.rng)
            ax, ay = g["adapt"]
            assert tuple(oracle.find_adaptor(k.raw, mc.REGION_PORE)) == (ax, ay)
            if not all(same_bits(v, b) for v, b in zip(oracle.statf(pa[ax:ay]), g["adapt_bits"])):
                bad.append("r:" + k.name)
            px, py = g["polya"]
            if py > 0 and not all(same_bits(v, b) for v, b in zip(oracle.statf(pa[ay + px:ay + py]), g["polya_bits"])):
                bad.append("r:" + k.name + ":polya")
    assert not bad, bad


def test_plain_sort_agrees_on_the_raw_median(cases, golden):
    for c in cases:
        assert int(np.sort(c.raw)[c.raw.size // 2]) == golden["stat"][c.name]["raw_median"], c.name


def test_pa_median_rule_outside_the_tie_class(cases, golden):
    """pA median = pA(raw order statistic of rank k2): what the windowed kernels rely on"""
    for c in cases:
        if not c.tie:
            assert same_bits(mc.pa_rule(c), golden["stat"][c.name]["bits"][4]), c.name


def test_tie_class_contains_the_bug(cases, golden):
    """the catalogue must not dodge it: on at least a quarter of the tie-class reads the reference's median is NOT
    pA(raw order statistic)"""
    ties = [c for c in cases if c.tie]
    differ = [c.name for c in ties if not same_bits(mc.pa_rule(c), golden["stat"][c.name]["bits"][4])]
    print("%d of %d tie-class reads differ from the rule" % (len(differ), len(ties)))
    assert len(ties) >= 60 and 4 * len(differ) >= len(ties), (len(differ), len(ties))
    # ... under every scale of the class, and in the region fixtures
    for nm, _, _ in mc.TIE_SCALES:
        assert any(d.startswith("tie_%s_" % nm) for d in differ), nm
    rdiff = []
    for k in mc.region_cases():
        ax, ay = golden["region"][k.name]["adapt"]
        if k.tie and not same_bits(mc.pa_rule(k._replace(raw=k.raw[ax:ay])), golden["region"][k.name]["adapt_bits"][2]):
            rdiff.append(k.name)
    assert "region_range+0" in rdiff and len(rdiff) >= 3, rdiff


def test_model_ranks():
    assert mc.ranks(2, np.float32(-1)) == (1, 0, True)
    assert mc.ranks(3, np.float32(-1)) == (1, 1, False)
    assert mc.ranks(4, np.float32(-0.0)) == (2, 2, False)
    assert mc.centre(np.float32(-0.5)) == 0 and mc.centre(np.float32(-16.5)) == -16 and mc.centre(np.float32(4e4)) == 32767
