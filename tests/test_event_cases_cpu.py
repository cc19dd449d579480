"""CPU: the catalogue of tests/event_cases.py is what it claims to be.  Its restatement of the t-statistic gives the oracle's
bits and its branch model the oracle's peaks on every read and pA array, with either preset (the oracle itself is pinned to
the real reference on the reads the reference can take: test_oracle_vs_ref.py, group event_catalogue); every branch tag of the
reference's loop and every place of the GPU forms fires on some read, with each preset that can reach it; the reads that
were tuned for a place take it, the committed search constants are what the searches find; the catalogue tells the right
automaton from eight wrong ones; its bytes are pinned, and the CLI goldens hold what the model says."""
import hashlib
import json
import os

import numpy as np
import pytest

import event_cases as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#: sha256 over names, samples and presets (event_cases.catalogue_sha256): a changed read shows up here, and the goldens
#: (tests/golden/event_cases_*.tsv, the group event_catalogue of ref_vectors.json) have to be regenerated with it
CATALOGUE_SHA256 = "6ba92ce9a0d93a27272bbc1db360f0abe90d805d774b24808ec3a8ca7dc0905f"

#: the reads of the CLI goldens
CLI_CASES = ["seed_300_rna", "row_smooth_0", "row_smooth_3", "row_smooth_15", "row_smooth_37", "row_smooth_48", "row_smooth_61",
             "row_smooth_96", "row_smooth_17", "row_ramp_17", "row_ramp_48", "row_ramp_55", "row_mix_0", "row_mix_22", "row_mix_41", "row_mix_76",
             "mask_pair_r", "decline_d_300", "decline_r_300", "decline_d_560_low", "chunk_first_r", "chunk_last_r", "seam-1_d", "seam+0_d",
             "seam+1_d", "seam-1_r", "seam+0_r", "seam+1_r", "two_seams_r", "two_seams_long_r"]


@pytest.fixture(scope="module")
def cat():
    return E.catalogue()


@pytest.fixture(scope="module")
def table(cat):
    return E.tag_table(cat)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_model_equals_the_oracle(oracle, cat):
    """pA, both t-statistics (bit for bit) and the peaks of the model against the oracle's; event_raw starts at the peaks"""
    for k in cat:
        pa = oracle.pa(k.raw, *E.SCALE)
        assert np.array_equal(_bits(pa), _bits(E.pa_of(k.raw))), k.name
        s, q = oracle.prefix_sums(pa)
        for label, rna in E.case_runs(k):
            p = E.PRESET[rna]
            t1, t2 = oracle.tstat(s, q, p.w1), oracle.tstat(s, q, p.w2)
            m1, m2 = E.tstats(k.raw, rna)
            assert np.array_equal(_bits(t1), _bits(m1)) and np.array_equal(_bits(t2), _bits(m2)), label
            want = [x for x, _ in E.peaks_model(t1, t2, rna)[0]]
            assert oracle.peaks(t1, t2, rna).tolist() == want, label
            if k.raw.size:
                assert oracle.event_raw(k.raw, *E.SCALE, rna).start.tolist() == [0] + want, label
    for k in E.pa_cases():
        s, q = oracle.prefix_sums(k.pa)
        p = E.PRESET[k.rna]
        t1, t2 = oracle.tstat(s, q, p.w1), oracle.tstat(s, q, p.w2)
        m1, m2 = E.tstats_pa(k.pa, k.rna)
        assert np.array_equal(_bits(t1), _bits(m1)) and np.array_equal(_bits(t2), _bits(m2)), k.name
        want = [x for x, _ in E.peaks_model(t1, t2, k.rna)[0]]
        assert oracle.peaks(t1, t2, k.rna).tolist() == want, k.name
        assert oracle.getevents(k.pa, k.rna).start.tolist() == [0] + want, k.name


def test_every_tag_fires_with_each_preset(table):
    """every branch of the reference's loop and every special place of the GPU forms is reached by some read with EACH
    preset (but the ones event_cases.E_TAGS_ONE_PRESET names, with its reasons); the message names the tag no read reaches"""
    table, _ = table
    for tag in E.E_TAGS + E.G_TAGS + E.S_TAGS:
        for rna in (0, 1):
            if E.E_TAGS_ONE_PRESET.get(tag, rna) != rna:
                continue
            assert any(n.endswith("/rna%d" % rna) for n in table.get(tag, [])), "no read takes %s with rna %d" % (tag, rna)
    for (rna, n), tag in E.G_LEN_32768.items():
        assert table.get(tag) == ["long_%d/rna%d" % (n, rna)], tag
    for tag in E.E_TAGS_PA + (E.E_NEG_ZERO,):
        got = table.get("pa " + tag, [])
        assert any(n.startswith(("dna_", "neg_zero_d")) for n in got) and any(n.startswith(("rna_", "neg_zero_r")) for n in got), \
            "no pA array takes %s with each preset" % tag


def test_what_the_cases_are_named_after(oracle, cat, table):
    """the reads that were tuned for one place take THAT place (a retuned constant that lands elsewhere shows up here)"""
    table, longs = table

    def on(tag, label):
        return label in table[tag]
    # the issue's seeds, as the oracle has them
    assert longs["dna_seed/rna0"] == [70] and longs["rna_seed/rna1"] == [47, 108]
    assert oracle.event_raw(E.dna_seed().astype(np.int16), *E.SCALE, 0).start.tolist() == [0, 42, 46, 51, 57, 61, 65, 70]
    t2 = E.tstats(E.dna_seed(), 0)[1]
    assert abs(float(t2[65]) - 9.80) < 0.005 and float(t2[70]) > 1e17   # (9.80 is reset away; both windows of 70 are constant)
    for rna, d in ((0, "d"), (1, "r")):
        r = "/rna%d" % rna
        assert on(E.E_EMIT_LAST[1], ("dna_seed_cut", "rna_seed_cut")[rna] + r)
        assert on(E.G_RUN_AT_END_EMITS, "seed_300_%s%s" % (("dna", "rna")[rna], r))
        assert on(E.E_LONG_BETWEEN_CLOSE, "between_%s%s" % (d, r))
        for L, tag in ((120, E.G_DELAY_ERARE), (300, E.G_DELAY_OLDPEAK)):
            assert on(tag, "decline_%s_%d%s" % (d, L, r))
        assert on(E.G_DELAY_SLOW, ("decline_d_560_low", "decline_r_600")[rna] + r)
        assert on(E.G_AT_CHUNK_FIRST, "chunk_first_%s%s" % (d, r)) and on(E.G_AT_CHUNK_LAST, "chunk_last_%s%s" % (d, r))
        for delta in (-1, 0, 1):
            label = "seam%+d_%s%s" % (delta, d, r)
            assert {2048 + delta, 3072 + delta} <= set(longs[label]), label
            for seg, _ in E.SEGMENTS:
                assert on(E.S_AT_SEAM[(seg, delta)], label)
        assert on(E.S_CROSS_PEAK[1024], "seam-1_%s%s" % (d, r)) and on(E.S_CROSS_PEAK[3072], "seam-1_%s%s" % (d, r))
        assert on(E.S_TWO_SEAMS[1024], ("two_seams_d", "const_3000")[rna] + r)
        for seg in (2048, 3072):
            assert on(E.S_TWO_SEAMS[seg], "two_seams_long_%s%s" % (d, r))
        assert on(E.G_NREC_OVER, "nrec_over_%s%s" % (d, r)) and not on(E.G_NREC_8, "nrec_over_%s%s" % (d, r))
        assert on(E.G_NREC_8, "nrec_8_%s%s" % (d, r)) and not on(E.G_NREC_OVER, "nrec_8_%s%s" % (d, r))
        assert on(E.E_N["2w1"], "len_%d%s" % (2 * E.PRESET[rna].w1, r)) and on(E.E_N["2w2+1"], "len_%d%s" % (2 * E.PRESET[rna].w2 + 1, r))
    assert on(E.G_DENSE, "dense_6000/rna0")
    # the kernels' constants, restated: 5 000 samples with a warm-up of 32 are chunks of 80 on 63 lanes (event_device.h)
    assert E.chunk_len_fast(5000, 32) == 80 and len(E.lanes_whole(5000, 0)[1]) == 63 and E.lanes_whole(5000, 0)[1][1] == (112, 192)
    assert E.chunk_len_fast(40000, 64) == 624 and E.chunk_len_lanes(5000, 32, 4) == 1248
    assert [E.lead_of(n, 0) for n in (32767, 32768)] == [32, 64] and [E.lead_of(n, 1) for n in (32768, 32769)] == [128, 256]
    assert E.lanes_segment(2048, 4096, 0) == (32, [(2048 + 32 * c, 2080 + 32 * c) for c in range(64)])
    # the long reads in noise: both seeds' boundaries in chunks of 512 - 640 samples, and no lane near 8 certainly hot runs
    by_name = {k.name: k for k in cat}
    for name in ("long_40000_quiet", "long_32767", "long_32768", "long_32769"):
        for rna in (0, 1):
            assert len(longs["%s/rna%d" % (name, rna)]) >= 20 and on(E.G_IN_RECORDING_LANE, "%s/rna%d" % (name, rna))
            info = E.analyse(by_name[name].raw, rna)[2]
            own = E.lanes_whole(by_name[name].raw.size, rna)[1]
            ends = [E._lane_of(own, min(r.b, info["n"] - 1)) for r in info["runs"] if r.sure_hot]
            assert own[1][1] - own[1][0] >= 512 and max(ends.count(c) for c in set(ends)) <= 4
    sizes = [k.raw.size for k in cat]
    assert min(sizes) == 0 and max(sizes) == 40000 and 2e5 < sum(sizes) < 2e6


#: a wrong automaton -> reads of the catalogue on which it gives other peaks than the right one
TOLD_APART = {"long_never_emits": ("dna_seed/rna0", "rna_seed/rna1"), "long_not_reset": ("dna_seed/rna0", "rna_seed/rna1"),
              "reset_leaves_valid": ("row_smooth_0/rna0", "row_smooth_17/rna1"), "max_update_>=": ("row_smooth_0/rna0", "rna_seed/rna1"),
              "emit_>=": ("rna_seed/rna0", "row_smooth_0/rna1"), "mask_one_short": ("row_ramp_17/rna0", "decline_d_600/rna1"),
              "mask_one_long": ("dna_seed/rna0", "mask_pair_r/rna1"), "run_from_reset_index": ("row_smooth_48/rna0", "row_smooth_15/rna1")}


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_the_catalogue_tells_wrong_automata_apart(cat, variant):
    by_name = {k.name: k for k in cat}
    for label in TOLD_APART[variant]:
        name, rna = label.rsplit("/rna", 1)
        right = E.analyse(by_name[name].raw, int(rna))[0]
        wrong = E.analyse(by_name[name].raw, int(rna), variant)[0]
        assert [x for x, _ in wrong] != [x for x, _ in right], "%s gives the right peaks on %s" % (variant, label)


def test_search_constants_are_what_the_searches_find():
    found = E.run_searches()
    assert found == {"CHUNK_EDGE_FRONT": E.CHUNK_EDGE_FRONT, "SEAM_FRONT": E.SEAM_FRONT, "NREC8_FRONT": E.NREC8_FRONT,
                     "DECLINE_ONSET": E.DECLINE_ONSET, "DECLINE_SLOW_DNA": E.DECLINE_SLOW_DNA, "PA_EQUAL": E.PA_EQUAL}


def test_catalogue_is_pinned():
    assert E.catalogue_sha256() == E.catalogue_sha256() == CATALOGUE_SHA256


@pytest.mark.parametrize("rna,kind", [(0, "dna"), (1, "rna")])
def test_goldens_hold_the_cli_cases(cat, rna, kind):
    """tests/golden/event_cases_*.tsv (what the reference CLI printed): the reads are event_cases.cli_cases(), a row per
    read (-c) or per event, the event starts and lengths are the model's; the files are the ones MANIFEST.json lists"""
    manifest = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    want = E.cli_cases(cat)
    assert [k.name for k in want] == CLI_CASES
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) <= os.path.getsize(os.path.join(GOLDEN, "zstd_frames.npz"))
               for f in os.listdir(GOLDEN))
    raw_c = open(os.path.join(GOLDEN, "event_cases_%s.event_c.tsv" % kind), "rb").read()
    raw_e = open(os.path.join(GOLDEN, "event_cases_%s.event.tsv" % kind), "rb").read()
    assert hashlib.sha256(raw_c).hexdigest() == manifest["event_cases_%s.event_c.tsv" % kind]
    assert hashlib.sha256(raw_e).hexdigest() == manifest["event_cases_%s.event.tsv" % kind]
    rows_c = raw_c.decode().split("\n")[1:-1]
    rows_e = [r.split("\t") for r in raw_e.decode().split("\n")[1:-1] if r]   # (a blank line ends every read)
    assert len(rows_c) == len(want)
    at = 0
    for row, k in zip(rows_c, want):
        f = row.split("\t")
        starts = [0] + [x for x, _ in E.analyse(k.raw, rna)[0]]
        lengths = np.diff(starts + [k.raw.size]).tolist()
        assert f[0] == k.name and int(f[1]) == k.raw.size and (int(f[2]), int(f[3])) == (0, k.raw.size), row[:80]
        assert int(f[4]) == len(starts) and f[5].rstrip(",") == ",".join(map(str, lengths)), row[:80]
        for j, (s0, ln) in enumerate(zip(starts, lengths)):
            r = rows_e[at + j]
            assert r[:4] == [k.name, str(j), str(s0), str(s0 + ln)], r
        at += len(starts)
    assert at == len(rows_e)
