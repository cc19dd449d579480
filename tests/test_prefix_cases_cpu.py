"""CPU: the catalogue of tests/prefix_cases.py is what it claims to be.  Its branch models give the oracle's answers on
every read (the oracle itself is pinned to the real reference on the same reads: test_oracle_vs_ref.py, group
prefix_catalogue), every branch tag fires where it must, and two builds of the catalogue are the same bytes."""
import os

import numpy as np
import pytest

import prefix_cases as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cat():
    return P.catalogue()


@pytest.fixture(scope="module")
def table(cat):
    return P.tag_table(cat)


def test_models_equal_the_oracle(oracle, cat):
    with np.errstate(all="ignore"):
        for k in cat:
            for pore in (0, 2):
                assert P.jnnv2_model(k.raw, P.adaptor_params(pore))[0] == oracle.find_adaptor(k.raw, pore), (k.name, pore)
                for rna in (0, 1):
                    (ax, ay), (px, py), _ = P.prefix_model(k.raw, k.dig, k.off, k.rng, rna, pore)
                    e = oracle.prefix(k.raw, k.dig, k.off, k.rng, rna, pore)
                    assert (e.adapt_x, e.adapt_y) == (ax, ay), (k.name, pore)
                    want = (e.polya_x + ay, e.polya_y + ay) if e.polya_y > 0 else (-1, -1)
                    assert (px, py) == want, (k.name, pore, rna)
    for k in P.shim_cases():
        assert P.jnnv2_model(k.raw, k.p)[0] == oracle.jnnv2(k.raw, k.p.std_scale, k.p.seg_dist, k.p.hi, k.p.lo), k.name
    for k in P.pa_cases():
        assert P.polya_model(k.pa, k.top, k.bot)[0] == oracle.find_polya(k.pa, k.top, k.bot, 0), k.name


@pytest.mark.parametrize("pore", [0, 2])
def test_every_branch_fires_through_the_subtool(table, pore):
    """every branch of jnnv2 and of the polyA automaton is taken by some read WITH THIS PORE (std_scale and lo_thresh
    differ between the pores, so the tuned reads come in pairs)"""
    for tag in P.A_TAGS_SUBTOOL + P.P_TAGS_SUBTOOL:
        assert any(n.endswith("/pore%d" % pore) for n in table.get(tag, [])), "no read takes %s with pore %d" % (tag, pore)


def test_every_branch_fires_in_the_shim_and_pa_cases(table):
    for tag in P.A_TAGS_SHIM:
        assert table.get("shim " + tag), tag
    for tag in P.P_TAGS:
        assert table.get("pa " + tag), tag


def test_what_the_cases_are_named_after(cat, table):
    """the reads that were tuned for one branch take THAT branch (a retuned constant that lands elsewhere shows up here)"""
    for pore in (0, 2):
        def on(tag, name):
            return "%s/pore%d" % (name, pore) in table[tag]
        assert on(P.A_GAP_DIST_M1, "gap_seg_dist-1_merged_pore%d" % pore) and on(P.A_GAP_DIST, "gap_seg_dist_two_runs_pore%d" % pore)
        assert on(P.A_ONE_SAMPLE, "one_window_run_pore%d" % pore) and on(P.A_ONE_SAMPLE_MERGE, "one_window_run_kills_pore%d" % pore)
        assert on(P.A_EQ_INSIDE, "threshold_on_slope_pore%d" % pore) and on(P.A_EQ_OUTSIDE, "threshold_on_slope_pore%d" % pore)
        assert on(P.A_EQ_OUTSIDE, "const_500x3000") and not on(P.A_EQ_OUTSIDE, "const_333x100000")   # (inexact sum: bot != 333)
        assert on(P.A_EQ_OUTSIDE, "const_below_clamp") and on(P.A_EQ_OUTSIDE, "const_above_clamp")
        assert on(P.A_SKIP_HI, "long_dip_then_adaptor") and on(P.A_ANS_LATER, "long_dip_then_adaptor")
        assert on(P.P_KEPT_AT_WINDOW, "pa_stretch_220") and on(P.P_REJECT_AT_WINDOW_M1, "pa_stretch_219")
        assert on(P.P_MERGE_AT_DIST_M1, "pa_merge_199") and on(P.P_SECOND_AT_DIST, "pa_nomerge_200")
        R = P.GEOMETRY_RESIDUES
        for k, (leader, dip) in enumerate(P.GEOMETRY[pore]):   # run edges on the wave kernel's tile positions
            (a, b), = P.jnnv2_model(P.geometry(leader, dip), P.adaptor_params(pore))[2]
            assert (a % 1024, b % 1024) == (R[k] % 1024, R[(k + 3) % len(R)] % 1024) and b - a > 3 * 1024
        for k, gap in zip(P.TILE_EDGE_K, P.TILE_EDGE[pore]):   # the polyA stretch ends k samples in front of a tail tile
            (ax, ay), (px, py), _ = P.prefix_model(P.tile_edge(gap), P.DIG, P.OFF, P.RNG, 1, pore)
            assert py - px == 600 and (py - (ay & ~7)) % 1024 == -k % 1024, (pore, k)
    # the answer of this read differs between the pores (lo_thresh 2000 against 500)
    k = next(k for k in cat if k.name == "tiny_then_long")
    assert P.jnnv2_model(k.raw, P.adaptor_params(0))[0] != P.jnnv2_model(k.raw, P.adaptor_params(2))[0]
    # a polyA is found on the decreasing branch (negative unit, positive pA)
    k = next(k for k in cat if k.name == "scale_decreasing_polya")
    assert k.rng < 0 and P.prefix_model(k.raw, k.dig, k.off, k.rng, 1, 0)[1][1] > 0
    sizes = [k.raw.size for k in cat]
    assert min(sizes) == 1999 and sorted(sizes)[-2] <= 100000 and max(sizes) == 460000 and sum(sizes) < 2.2e6


def test_catalogue_is_deterministic():
    assert P.catalogue_sha256() == P.catalogue_sha256()


def test_goldens_hold_the_finite_part_of_the_catalogue(cat):
    """tests/golden/prefix_cases_*.prefix_stat.tsv (what the reference CLI printed): one row per read, the adaptor columns
    are the model's"""
    want = [k for k in P.finite_cases(cat)]
    for fname, pore in (("prefix_cases_r9.prefix_stat.tsv", 0), ("prefix_cases_rna004.prefix_stat.tsv", 2)):
        rows = open(os.path.join(GOLDEN, fname)).read().split("\n")[1:-1]
        assert len(rows) == len(want)
        for row, k in zip(rows, want):
            f = row.split("\t")
            (ax, ay), (px, py), _ = P.prefix_model(k.raw, k.dig, k.off, k.rng, 1, pore)
            assert f[0] == k.name and int(f[1]) == k.raw.size
            assert f[2:6] == [str(ax) if ay > 0 else ".", str(ay) if ay > 0 else ".", str(px) if py > 0 else ".",
                              str(py) if py > 0 else "."], row
