"""CPU: the catalogue of tests/jnn_cases.py is what it claims to be.  Its branch model gives the oracle's segments on every
read (the oracle itself is pinned to the real reference on the same reads: test_oracle_vs_ref.py, group jnn_catalogue),
every branch tag of the reference's loop and every geometry tag of the GPU forms fires on some read, the committed
search constants are what the searches find, and the catalogue's bytes are pinned."""
import os

import numpy as np
import pytest

import jnn_cases as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#: sha256 over names, samples and parameters (jnn_cases.catalogue_sha256): a changed read shows up here, and the goldens
#: (tests/golden/jnn_cases_*.jnn.tsv, the group jnn_catalogue of ref_vectors.json) have to be regenerated with it
CATALOGUE_SHA256 = "6371489bc8e4f8f40751336080ea3d3e3509b87b8c122605e35f8e1c8278cb84"


@pytest.fixture(scope="module")
def cat():
    return J.catalogue()


@pytest.fixture(scope="module")
def table(cat):
    return J.tag_table(cat)


def _pairs(x, y):
    return [(int(a), int(b)) for a, b in zip(x, y)]


def test_model_equals_the_oracle(oracle, cat):
    with np.errstate(all="ignore"):
        for k in cat:
            sig = J.clamp_raw(k.raw)
            for label, p in J.case_runs(k):
                want = J.jnn_core_model(sig, p)[0]
                op = oracle.jnn_param(**p._asdict())
                assert _pairs(*oracle.jnn_core(sig, op)) == want, label
                assert _pairs(*oracle.jnn_raw_param(k.raw, op)) == want, label
            if k.params is None:
                for rna in (0, 1):
                    assert _pairs(*oracle.jnn_raw(k.raw, rna)) == J.jnn_core_model(sig, J.PRESET[rna])[0], (k.name, rna)
        for k in J.pa_cases():
            want = J.jnn_core_model(J.clamp_pa(k.pa), k.params)[0]
            assert _pairs(*oracle.jnn_pa(k.pa, oracle.jnn_param(**k.params._asdict()))) == want, k.name


def test_every_tag_fires(table):
    """every branch of the reference's loop and every special place of the GPU forms is reached by some read; the
    message names the tag that no read reaches"""
    for tag in J.J_TAGS + J.G_TAGS:
        assert table.get(tag), "no read takes %s" % tag
    for tag in J.J_TAGS_PA:
        assert table.get("pa " + tag), "no pA array takes %s" % tag


def test_every_branch_fires_through_the_subtool(table):
    """... and what the presets can reach is reached by a preset case with EITHER preset (they go through the subtool and
    the CLI; cases with their own parameters only through the per-read call)"""
    for rna in (0, 1):
        for tag in J.J_TAGS_PRESET + (J.J_TAGS_CDNA if rna == 0 else ()):
            assert any(n.endswith("/rna%d" % rna) for n in table.get(tag, [])), "no preset read takes %s with rna %d" % (tag, rna)
    # the geometry of the wave kernel and of the long-read chains can only be reached with a preset (k_long_chains takes
    # thresholds from the read's own moments; the per-read call never has a long read)
    for tag in J.G_TAGS:
        if tag not in (J.G_ERROR_0, J.G_ERROR_31):
            assert any(n.endswith(("/rna0", "/rna1")) for n in table.get(tag, [])), "no preset read takes %s" % tag


def test_what_the_cases_are_named_after(cat, table):
    """the reads that were tuned for one place take THAT place (a retuned constant that lands elsewhere shows up here)"""
    def on(tag, label):
        return label in table[tag]
    assert on(J.J_C_FIRST_MIN, "first_rule_38/rna0") and on(J.J_C_FIRST_MIN_M1, "first_rule_37/rna0")
    assert on(J.J_C_WINDOW, "window_150/rna0") and on(J.J_C_WINDOW_M1, "window_149/rna0")
    assert on(J.J_C_WINDOW, "window_1000/rna1") and on(J.J_C_WINDOW_M1, "window_999/rna1")
    assert on(J.J_MERGE_DIST_M1, "merge_49/rna0") and on(J.J_NOMERGE_DIST, "nomerge_50/rna0")
    assert on(J.J_MERGE_DIST_M1, "merge_49_rna/rna1") and on(J.J_NOMERGE_DIST, "nomerge_50_rna/rna1")
    assert on(J.J_WEAK_DROPPED, "weak_after_first/rna0") and on(J.J_ABANDONED, "abandoned/rna0")
    assert on(J.J_NO_TRAIL, "scattered_close/rna0") and on(J.J_BUDGET, "scattered_close/rna0") and on(J.J_OPEN_END, "open_end/rna0")
    by_name = {k.name: k for k in cat}
    for what, (tag, _) in J.SYNC_WANT.items():
        assert J.chunk0_end(by_name["sync_" + what].raw) == {tag}, what
        assert on(tag, "sync_%s/rna0" % what)
    assert on(J.G_SEG_SPANS_CHUNK, "span_chunks/rna0") and on(J.G_SEG_SPANS_CHUNK, "span_chunks_rna/rna1")
    assert on(J.G_WEAK_FIRST_LANE, "weak_first_lane2/rna0")
    assert on(J.G_WEAK_NOT_FIRST_DROPPED, "weak_behind_candidate/rna0") and on(J.G_WEAK_NOT_FIRST_DROPPED, "weak_behind_strong/rna0")
    assert on(J.G_MERGE_ACROSS_EMPTY, "merge_across_empty/rna0")
    assert on(J.G_MERGE_ACROSS_DIST_M1, "lanes_49_50/rna0") and on(J.G_NOMERGE_ACROSS_DIST, "lanes_49_50/rna0")
    for name in ("no_sync_16384", "no_sync_40000", "no_sync_all_5000"):
        assert on(J.G_STAGE_OVERFLOW, name + "/rna0")
    assert on(J.L_STAGE_OVERFLOW, "no_sync_16384/rna0") and on(J.L_STAGE_OVERFLOW, "no_sync_40000/rna0")
    assert on(J.L_MERGE_ACROSS_ROUNDS, "rounds_merge_49/rna0") and on(J.J_MERGE_DIST_M1, "rounds_merge_49/rna0")
    assert on(J.L_NOMERGE_ACROSS_ROUNDS, "rounds_nomerge_50/rna0") and on(J.J_NOMERGE_DIST, "rounds_nomerge_50/rna0")
    assert on(J.L_LAST_BY_FLUSH, "rounds_flush/rna0") and on(J.L_WEAK_FIRST_ROUND2, "rounds_weak_first/rna0")
    assert on(J.L_WEAK_NOT_FIRST_ROUND2, "rounds_weak_dropped/rna0")
    for c, n in ((1, 511), (2, 512), (2, 513), (62, 16127), (63, 16128), (63, 16383), (64, 16384)):
        assert J.jnn_chunk_lanes(n) == c and on(J.G_NQ[n], "rich_%d/rna0" % n)
    assert J.jnn_long_chunks(40000) == 78 and J.chunk_len(40000, 78) == 520 and (J.slots(40000)[0] - J.slots(40000)[1]) // 78 == 8
    # the launch rule: the own-parameter sets lie one step either side of each of its terms
    R = J.RULE_PARAMS
    assert [J.wave_ok(R[k]) for k in ("error0", "error-1", "error31", "error32", "window127", "error==corrector",
                                      "error==corrector-1", "polya")] == [True, False, True, False, False, False, True, True]
    assert J.wave_ok(J.fixed(window=128)) and J.wave_ok(J.PRESET[0]) and J.wave_ok(J.PRESET[1])
    # the correction: it fires with error == corrector and with error > corrector, it changes the answer on every
    # correction/ case but the one that is there for NOT firing, and it cannot fire with error < corrector
    for k in cat:
        if k.params is None:
            continue
        sig = J.clamp_raw(k.raw)
        with_c, tags, _ = J.jnn_core_model(sig, k.params)
        without = J.jnn_core_model(sig, k.params, correction=False)[0]
        if k.params.error < k.params.corrector:
            assert J.J_CORRECTION not in tags and with_c == without, k.name
        if k.name.startswith("correction/") and k.name != "correction/below_window":
            assert J.J_CORRECTION in tags and with_c != without, k.name
    assert J.J_CORRECTION not in J.jnn_core_model(J.clamp_raw(by_name["correction/below_window"].raw),
                                                  by_name["correction/below_window"].params)[1]
    assert any(n.startswith("error==corrector/") for n in table[J.J_CORRECTION])
    # ... and the catalogue tells the right loop from two wrong ones: without the err-- (what the wave kernel would give
    # if the launch rule let error == corrector through) and with the `c % w == 0` term of its condition dropped
    def differs(name, mode):
        k = by_name[name]
        return J.jnn_core_model(J.clamp_raw(k.raw), k.params)[0] != J.jnn_core_model(J.clamp_raw(k.raw), k.params, mode)[0]
    assert differs("error==corrector/io", False) and differs("error>corrector/io", False)
    assert differs("correction/c>w", J.NO_MOD) and differs("error==corrector/rich_2048", J.NO_MOD)
    for k in J.pa_cases():
        if k.name.startswith("correction"):
            sig = J.clamp_pa(k.pa)
            assert len({repr(J.jnn_core_model(sig, k.params, m)[0]) for m in (True, False, J.NO_MOD)}) == 3, k.name
    assert on(J.J_CORRECTION_TWICE, "correction/twice") and not on(J.J_CORRECTION_TWICE, "correction/c>w")
    sizes = [k.raw.size for k in cat]
    assert min(sizes) == 1 and max(sizes) == 40000 and 5e5 < sum(sizes) < 2e6


def test_search_constants_are_what_the_searches_find():
    found = J.run_searches()
    assert found["SYNC_LEAD"] == J.SYNC_LEAD and tuple(found["ROUNDS_FIRST"]) == J.ROUNDS_FIRST


def test_catalogue_is_pinned():
    assert J.catalogue_sha256() == J.catalogue_sha256() == CATALOGUE_SHA256


@pytest.mark.parametrize("rna,fname,compact", [(0, "jnn_cases_dna.jnn.tsv", False), (1, "jnn_cases_rna.jnn.tsv", False),
                                               (0, "jnn_cases_dna.jnn_c.tsv", True), (1, "jnn_cases_rna.jnn_c.tsv", True)])
def test_goldens_hold_the_preset_cases(cat, rna, fname, compact):
    """tests/golden/jnn_cases_*.tsv (what the reference CLI printed): one row per preset read, the segments are the model's"""
    rows = open(os.path.join(GOLDEN, fname)).read().split("\n")[1:-1]
    want = J.preset_cases(cat)
    assert len(rows) == len(want)
    for row, k in zip(rows, want):
        f = row.split("\t")
        segs = J.jnn_core_model(J.clamp_raw(k.raw), J.PRESET[rna])[0]
        assert f[0] == k.name and int(f[1]) == k.raw.size and int(f[2]) == len(segs), row
        if not compact:
            assert f[3] == ("".join("%d,%d;" % s for s in segs) or "."), row
