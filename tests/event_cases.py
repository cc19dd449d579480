"""The catalogue of hand-made reads for `event`, a plain branch model of its peak detector, and the places of the GPU forms.

The reference steps two detectors at every index, a short and a long one (orc_peaks in oracle/sigtk_oracle.c).  On the GPU
the long one is lazy (csrc/event_detect.h): proven silent from f32 bounds, its "hot" runs recorded per lane (lz_record, at
most LZ_NREC = 8), replayed exactly after the pass (replay_run) and handed over seams (SegState::cross).  All of that exists
to produce the boundaries the long detector emits -- and, by the ORACLE's count (peaks of orc_peaks that it does not emit
when the long statistic is zeroed), no earlier test input holds one:

    all 100 reads of tests/golden/sp1_dna.blow5                      0 of 92 835 (DNA preset)   0 of 37 852 (RNA preset)
    the five tests/golden/soak*.npz reads                            0 of 5 974                 0 of 1 777
    const, steps, noise, tiny, zeros, dense, flat, ramp (n = 30 000) 0 of 29 450                0 of 5 238
    250 synthetic reads of 1 500 samples (csrc/synth.h), either kind 0                          0

The reads here have 664 (146 with the DNA, 518 with the RNA preset) on 72 of their 146 runs.  The two seeds of the issue that
asked for this catalogue are confirmed by the oracle: DNA_RISE between plateaus gives short boundaries at 42, 46, 51, 57,
61, 65 and a long one at 70 (where both long windows are constant: t2 = 6.4e17; the 9.80 at 65 is reset away), the RNA seed
long ones at 47 and 108.  Both are fragile: the DNA seed 5 raw units higher emits nothing.

`peaks_model` is orc_peaks as a literal loop; it returns the peaks in emission order with the detector that emitted each,
the set of BRANCHES that fired (E_* tags) and the long detector's runs.  `geometry_tags` works out from those, with the
kernels' constants restated below, which special places of the GPU forms a read touches (G_*: one wavefront per read; S_*:
segments of 1024 / 2048 / 3072 samples).  A run is "certainly hot" when it holds a statistic above thr2 or an index at which
both long windows are constant (both_flat: the cold proof cannot succeed there); no model of the f32 estimates is used.
tests/test_event_cases_cpu.py proves model == oracle on every read and requires every tag to fire with each preset.

What could not be reached, and is therefore no tag: a long boundary emitted at i = n - 1 and a VALID long peak pending at n
(the statistic is 0 over the last w2 indices, so a valid peak is always emitted by n - w2/2 + 1: E_EMIT_LAST is the
nearest case); a long boundary between short ones at most 2 * w2 apart (9 000 random shapes gave 17 / 30 as the closest:
the tag asks for 3 * w2); a long peak_value equal to thr2 outside a strong short peak; more than SEG_CROSS_MAX runs into one
segment (runs are disjoint: at most one crosses a seam).  E_TAGS_ONE_PRESET lists what only one preset reaches.

Reads are built from plateaus, integer ramps, smooth (cubic) transitions and steps; where a place needs tuning a search_*
function finds the parameter and what it found is committed next to it.  `python tests/event_cases.py` reruns the searches
and prints the constants and the tag -> read table (86 tags over 146 runs and 8 pA arrays).
"""
import hashlib
from typing import NamedTuple

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(F).max)
FLT_MIN = F(np.finfo(F).tiny)
SCALE = (8192.0, 10.0, 1402.882324)            # digitisation, offset, range of every catalogue read


class EP(NamedTuple):                          # the detector's parameters (the reference's two presets)
    w1: int
    w2: int
    thr1: float
    thr2: float
    ph: float


PRESET = {0: EP(3, 6, float(F(1.4)), 9.0, float(F(0.2))), 1: EP(7, 14, float(F(2.5)), 9.0, float(F(1.0)))}

# ---------------------------------------------------------------- numbers: pA, prefix sums, t-statistic (orc_pa, orc_tstat)


def pa_of(raw, dig=SCALE[0], off=SCALE[1], rng=SCALE[2]):
    unit = F(rng) / F(dig)
    return (np.asarray(raw, dtype=np.int16).astype(F) + F(off)) * unit


def prefix_sums(x):
    x = np.asarray(x, dtype=F)
    s = np.zeros(x.size + 1, dtype=np.float64)
    q = np.zeros(x.size + 1, dtype=np.float64)
    np.cumsum(x.astype(np.float64), out=s[1:])             # np.cumsum adds strictly in order
    np.cumsum((x * x).astype(np.float64), out=q[1:])       # the square is rounded to float first
    return s, q


def tstat(s, q, w):
    """orc_tstat, rounding step by rounding step"""
    n = s.size - 1
    t = np.zeros(n, dtype=F)
    if n < 2 * w or w < 2:
        return t
    i = np.arange(w, n - w + 1)
    wf = F(w)
    with np.errstate(all="ignore"):
        sum1, sumsq1 = s[i] - s[i - w], q[i] - q[i - w]
        sum2, sumsq2 = (s[i + w] - s[i]).astype(F), (q[i + w] - q[i]).astype(F)
        mean1 = (sum1 / np.float64(wf)).astype(F)
        mean2 = sum2 / wf
        acc = sumsq1 / np.float64(wf)
        acc = acc - (mean1 * mean1).astype(np.float64)
        acc = acc + (sumsq2 / wf).astype(np.float64)
        acc = acc - (mean2 * mean2).astype(np.float64)
        cv = np.maximum(acc.astype(F), FLT_MIN)
        delta = mean2 - mean1
        t[i] = (np.abs(delta.astype(np.float64)) / np.sqrt((cv / wf).astype(np.float64))).astype(F)
    return t


def tstats_pa(pa, rna):
    s, q = prefix_sums(pa)
    p = PRESET[rna]
    return tstat(s, q, p.w1), tstat(s, q, p.w2)


def both_flat(x, w2):
    """the indices i in [w2, n - w2] at which x[i - w2 .. i) and x[i .. i + w2) are both constant.  There the kernel's cold
    proof (sgk_long_cold: 81 (V - 2^-19 (qA + qB)) > ...) must fail: V, the sum of two differences of equal numbers
    rounded to float, is at most a few 2^-23 of q, so the right-hand side is negative"""
    x = np.asarray(x)
    n = x.size
    out = np.zeros(n, dtype=bool)
    if n >= 2 * w2:
        ch = np.concatenate([[0], np.cumsum(x[1:] != x[:-1])])          # ch[j] - ch[i]: changes inside x[i .. j]
        i = np.arange(w2, n - w2 + 1)
        out[i] = (ch[i - 1] == ch[i - w2]) & (ch[i + w2 - 1] == ch[i])
    return out


def tstats(raw, rna):
    return tstats_pa(pa_of(raw), rna)


# ---------------------------------------------------------------- branch tags: orc_peaks
def _both(name):
    return {0: "e:short:" + name, 1: "e:long:" + name}


E_NEW_MIN = _both("before_peak_new_minimum")
E_RISE_SMALL = _both("before_peak_rise<=peak_height")
E_RISE_EQ = _both("before_peak_v==peak_value")
E_OPEN = _both("peak_opens")
E_NEW_MAX = _both("in_peak_new_maximum")
E_PLATEAU = _both("in_peak_v==peak_value_position_stays")
E_VALID_NEXT = _both("valid_at_pos+1")
E_VALID_LATE = _both("valid_later_than_pos+window/2")
E_WAIT = _both("valid_but_i-pos<=window/2")
E_EMIT_EXACT = _both("emitted_at_pos+window/2+1")
E_HUGE_THEN_ORDINARY = _both("peak_value>=1e17_then_ordinary")
E_STRONG_RESET = "e:short:strong_peak_resets_long"
E_WEAK_NO_RESET = "e:short:peak_value<=thr1_no_reset"
E_SHORT_PENDING_AT_N = "e:short:peak_pending_at_n_dropped"
E_LONG_MASKED = "e:long:index_masked"
E_LONG_FIRST_UNMASKED = "e:long:first_index_behind_mask"
E_LONG_RESET_BEFORE = "e:long:reset_before_peak"
E_LONG_RESET_IN = "e:long:reset_in_peak"
E_LONG_RESET_VALID = "e:long:reset_while_valid_and_waiting_not_emitted"
E_LONG_LE_THR2 = "e:long:peak_above_peak_height_but<=thr2_never_valid"
E_LONG_EMIT = "e:long:boundary_emitted"
E_LONG_TWO = "e:long:two_boundaries_in_one_run"
E_LONG_BETWEEN_CLOSE = "e:long:boundary_between_short_boundaries<=3*w2_apart"
E_LONG_OPEN_AT_N = "e:long:run_open_at_n_peak_pending_dropped"
E_EMIT_LAST = _both("emitted_peak_at_n-window_the_last_index_with_a_statistic")
E_PV_EQ_THR = _both("peak_value==threshold_not_above_it")
E_RISE_EQ_PH = _both("before_peak_v-peak_value==peak_height_no_peak")
E_INDEX0 = "e:index_0_skipped"
E_T_ZERO = "t:both_windows_constant_and_equal_t==0"
E_T_HUGE = "t:both_windows_constant_and_different_t>=1e17"
E_N = {k: "n:" + k for k in ("0", "1", "2w1-1", "2w1", "2w1+1", "2w2-1", "2w2", "2w2+1")}
E_TAGS = tuple(t[k] for t in (E_NEW_MIN, E_RISE_SMALL, E_RISE_EQ, E_OPEN, E_NEW_MAX, E_PLATEAU, E_VALID_NEXT, E_VALID_LATE, E_WAIT,
                              E_EMIT_EXACT) for k in (0, 1)) + (
    E_HUGE_THEN_ORDINARY[0], E_HUGE_THEN_ORDINARY[1], E_EMIT_LAST[0], E_EMIT_LAST[1], E_STRONG_RESET, E_WEAK_NO_RESET, E_SHORT_PENDING_AT_N, E_LONG_MASKED, E_LONG_FIRST_UNMASKED,
    E_LONG_RESET_BEFORE, E_LONG_RESET_IN, E_LONG_RESET_VALID, E_LONG_LE_THR2, E_LONG_EMIT, E_LONG_TWO, E_LONG_BETWEEN_CLOSE,
    E_LONG_OPEN_AT_N, E_INDEX0, E_T_ZERO, E_T_HUGE) + tuple(E_N.values())

#: what only pA arrays can hold
E_TAGS_PA = (E_PV_EQ_THR[0], E_RISE_EQ_PH[0])
E_NEG_ZERO = "pa:-0.0_sample"
#: reached with one preset only: no read of the searches (6 000 random rises, 3 000 pairs of smooth transitions, 360 seeded
#: rows per preset) made the RNA preset's long detector turn valid later than 7 indices behind its peak
#: (... and short RNA peaks lie at least 5 apart: at most 410 in 2 048 samples)
E_TAGS_ONE_PRESET = {E_VALID_LATE[1]: 0, "g:more_than_512_boundaries_in_2048_samples": 0}

#: deliberately WRONG automata (peaks_model's `variant`): the CPU test shows that the catalogue tells each from the right one
VARIANTS = ("long_never_emits", "long_not_reset", "reset_leaves_valid", "max_update_>=", "emit_>=", "mask_one_short",
            "mask_one_long", "run_from_reset_index")
HUGE = 1e17


def _diff_gt(a, b, ph, tags=None, eq_tag=None):
    """(float)a - (float)b > ph in float arithmetic, for a, b, ph that are floats held as Python numbers"""
    d = a - b
    if d > ph * 1.001:
        return True
    if d < ph * 0.999:
        return False
    with np.errstate(all="ignore"):
        df = F(a) - F(b)
    if tags is not None and df == F(ph):
        tags.add(eq_tag)
    return bool(df > F(ph))


class Run(NamedTuple):             # a stretch the long detector walks between two resets
    a: int                         # first index it processes (not masked)
    b: int                         # the index of the reset that ends it, or n
    sure_hot: bool                 # some t2 in it exceeds thr2: the kernel's cold proof (a bound) must fail
    peaks: tuple                   # the boundaries it emits


def peaks_model(t1, t2, rna, variant=None, flat2=None):
    """orc_peaks as a literal loop -> (peaks [(position, detector)] in emission order, tags, info).  flat2 (both_flat): the
    indices at which both long windows are constant; they and the indices with t2 > thr2 make a run certainly hot"""
    assert variant is None or variant in VARIANTS
    p = PRESET[rna]
    n = len(t1)
    sig = (np.asarray(t1, dtype=F).astype(np.float64).tolist(), np.asarray(t2, dtype=F).astype(np.float64).tolist())
    thr, win, ph = (p.thr1, p.thr2), (p.w1, p.w2), p.ph
    masked_to, pos, val, valid = [0, 0], [-1, -1], [FLT_MAX, FLT_MAX], [False, False]
    ge_max, ge_emit = variant == "max_update_>=", variant == "emit_>="
    tags, peaks = set(), []
    runs, run_a, run_peaks, run_hot = [], 1, [], False
    short_emits = []                                  # (position, index of the emission)
    masked_seen = False

    last_reset = -2

    def close_run(b):
        # (a strong short peak resets at every index until it is emitted: what lies between two of ITS resets is no run)
        if run_a < b and last_reset != b - 1:
            runs.append(Run(run_a, b, run_hot, tuple(run_peaks)))
            if len(run_peaks) >= 2:
                tags.add(E_LONG_TWO)
    if n > 0:
        tags.add(E_INDEX0)
    for i in range(n):
        for k in (0, 1):
            if masked_to[k] >= i:
                if k == 1 and i > 0:
                    tags.add(E_LONG_MASKED)
                    masked_seen = True
                continue
            if k == 1:
                if masked_seen:
                    tags.add(E_LONG_FIRST_UNMASKED)
                    masked_seen = False
                if sig[1][i] > p.thr2 or (flat2 is not None and flat2[i]):
                    run_hot = True
            v = sig[k][i]
            if pos[k] < 0:
                if v < val[k]:
                    val[k] = v
                    tags.add(E_NEW_MIN[k])
                elif _diff_gt(v, val[k], ph, tags, E_RISE_EQ_PH[k]):
                    val[k] = v
                    pos[k] = i
                    tags.add(E_OPEN[k])
                else:
                    tags.add(E_RISE_EQ[k] if v == val[k] else E_RISE_SMALL[k])
            else:
                if v > val[k] or (ge_max and v == val[k]):
                    val[k] = v
                    pos[k] = i
                    tags.add(E_NEW_MAX[k])
                elif v == val[k]:
                    tags.add(E_PLATEAU[k])
                if k == 0:
                    if val[0] > thr[0]:
                        tags.add(E_STRONG_RESET)
                        if variant != "long_not_reset":
                            tags.add(E_LONG_RESET_BEFORE if pos[1] < 0 else E_LONG_RESET_VALID if valid[1] else E_LONG_RESET_IN)
                            close_run(i)
                            masked_to[1] = pos[0] + win[0] + {"mask_one_short": -1, "mask_one_long": 1}.get(variant, 0)
                            if variant == "run_from_reset_index":
                                masked_to[1] = i - 1
                            pos[1], val[1] = -1, FLT_MAX
                            if variant != "reset_leaves_valid":
                                valid[1] = False
                            run_a, run_peaks, run_hot, last_reset = max(i, masked_to[1] + 1), [], False, i
                            masked_seen = False
                    else:
                        tags.add(E_WEAK_NO_RESET)
                if val[k] == thr[k]:
                    tags.add(E_PV_EQ_THR[k])
                if _diff_gt(val[k], v, ph):
                    if val[k] > thr[k]:
                        if not valid[k]:
                            if i == pos[k] + 1:
                                tags.add(E_VALID_NEXT[k])
                            if i - pos[k] > win[k] // 2:
                                tags.add(E_VALID_LATE[k])
                            if val[k] >= HUGE and v < 1e6:
                                tags.add(E_HUGE_THEN_ORDINARY[k])
                        valid[k] = True
                    elif k == 1:
                        tags.add(E_LONG_LE_THR2)
                if valid[k]:
                    d = i - pos[k]
                    if d > win[k] // 2 or (ge_emit and d == win[k] // 2):
                        if d == win[k] // 2 + 1:
                            tags.add(E_EMIT_EXACT[k])
                        if not (k == 1 and variant == "long_never_emits"):
                            assert variant is not None or not peaks or pos[k] > peaks[-1][0], "emission order is not increasing in position"
                            peaks.append((pos[k], k))
                            if pos[k] == n - win[k]:
                                tags.add(E_EMIT_LAST[k])
                            if k == 1:
                                run_peaks.append(pos[1])
                                tags.add(E_LONG_EMIT)
                            else:
                                short_emits.append((pos[0], i))
                        pos[k], val[k], valid[k] = -1, v, False
                    else:
                        tags.add(E_WAIT[k])
    last_reset = -2
    close_run(n)
    if pos[0] >= 0:
        tags.add(E_SHORT_PENDING_AT_N)
    if pos[1] >= 0:
        tags.add(E_LONG_OPEN_AT_N)
    # a long boundary between two short ones that lie close together
    shorts = [x for x, k in peaks if k == 0]
    for x, k in peaks:
        if k == 1:
            lo = max([s for s in shorts if s < x], default=None)
            hi = min([s for s in shorts if s > x], default=None)
            if lo is not None and hi is not None and hi - lo <= 3 * p.w2:
                tags.add(E_LONG_BETWEEN_CLOSE)
    # the statistic and the lengths
    for w, t in ((p.w1, sig[0]), (p.w2, sig[1])):
        if n >= 2 * w:
            body = np.asarray(t[w:n - w + 1])
            if (body == 0).any():
                tags.add(E_T_ZERO)
            if (body >= HUGE).any():
                tags.add(E_T_HUGE)
    for name, m in (("0", 0), ("1", 1), ("2w1-1", 2 * p.w1 - 1), ("2w1", 2 * p.w1), ("2w1+1", 2 * p.w1 + 1),
                    ("2w2-1", 2 * p.w2 - 1), ("2w2", 2 * p.w2), ("2w2+1", 2 * p.w2 + 1)):
        if n == m:
            tags.add(E_N[name])
    return peaks, tags, {"n": n, "runs": runs, "short_emits": short_emits, "long": [x for x, k in peaks if k == 1]}


# ---------------------------------------------------------------- the kernels' geometry, restated (event_device.h, event_detect.h)
LEAD = {0: (32, 64), 1: (128, 256)}     # LEAD_DNA_SHORT, LEAD_DNA / LEAD_RNA_SHORT, LEAD_RNA
UNROLL = 16
LZ_NREC, RING = 8, 512
SEG_CROSS_MAX, SEG_PRE_MAX = 23, 15
BUILD_MAX_BOUNDARIES, BUILD_TILE = 512, 2048
REP_MAX_EVENTS = 32
SEGMENTS = ((1024, 1025), (2048, 2049), (3072, 3073))


def lead_of(length, rna):
    """the 32 768-sample rule of detect_span"""
    if rna:
        return LEAD[1][0] if length <= 32768 else LEAD[1][1]
    return LEAD[0][0] if length < 32768 else LEAD[0][1]


def chunk_len_fast(n, lead):
    return 16 * max((max(n - lead, 1) + 1023) // 1024, 1)


def chunk_len_lanes(n, lead, lanes):
    return 16 * max((max(n - lead, 1) + 16 * lanes - 1) // (16 * lanes), 1)


def lanes_whole(n, rna, lanes=64):
    """-> (lead, [(s, e)]): what every lane of a read's wavefront owns (lane 0 from 0; lane c warms up over [s - lead, s))"""
    lead = lead_of(n * (64 // lanes), rna)
    K = chunk_len_fast(n, lead) if lanes == 64 else chunk_len_lanes(n, lead, lanes)
    own = []
    for c in range(lanes):
        s = 0 if c == 0 else c * K + lead
        e = min(lead + K if c == 0 else s + K, n)
        if s < n:
            own.append((s, e))
    return lead, own


def lanes_segment(a, b, rna):
    """a segment [a, b) of a cut read: every lane warms up"""
    K = 16 * ((b - a + 1023) // 1024)
    return lead_of(b - a, rna), [(a + c * K, min(a + (c + 1) * K, b)) for c in range(64) if a + c * K < b]


def _lane_of(own, x):
    for c, (s, e) in enumerate(own):
        if s <= x < e:
            return c
    raise AssertionError(x)


G_IN_RECORDING_LANE = "g:long_boundary_in_the_chunk_that_records_its_run"
G_IN_EARLIER_LANE = "g:long_boundary_in_an_earlier_lane's_chunk"
G_RUN_SPANS_CHUNKS = "g:hot_run_spans_two_whole_chunks"
G_RUN_AT_END_EMITS = "g:run_recorded_at_the_read's_end_emits"
G_AT_CHUNK_FIRST = "g:long_boundary_at_first_index_of_a_chunk"
G_AT_CHUNK_LAST = "g:long_boundary_at_last_index_of_a_chunk"
G_IN_WARMUP = "g:long_boundary_and_its_run's_end_inside_a_lane's_warm-up"
G_NREC_OVER = "g:more_than_8_hot_runs_end_in_one_chunk"
G_NREC_8 = "g:exactly_8_runs_end_in_one_chunk_none_more"
G_DELAY_ERARE = "g:short_peak_emitted_17..224_behind_its_position"
G_DELAY_OLDPEAK = "g:short_peak_emitted_225..511_behind_its_position"
G_DELAY_SLOW = "g:short_peak_emitted_more_than_512_behind_its_position"
G_SHORT_PRE = "g:short_peak_pending_at_a_chunk_end_emitted_by_the_lane_behind"
G_DENSE = "g:more_than_512_boundaries_in_2048_samples"
G_LEN_32768 = {(r, m): "g:rna%d_n==%d" % (r, m) for r in (0, 1) for m in (32767, 32768, 32769)}
G_TAGS = (G_IN_RECORDING_LANE, G_IN_EARLIER_LANE, G_RUN_SPANS_CHUNKS, G_RUN_AT_END_EMITS, G_AT_CHUNK_FIRST, G_AT_CHUNK_LAST,
          G_IN_WARMUP, G_NREC_OVER, G_NREC_8, G_DELAY_ERARE, G_DELAY_OLDPEAK, G_DELAY_SLOW, G_SHORT_PRE, G_DENSE)
S_CROSS_PEAK = {s: "s%d:long_boundary_in_front_of_a_seam_its_run_ends_behind" % s for s, _ in SEGMENTS}
S_AT_SEAM = {(s, d): "s%d:long_boundary_at_seam%+d" % (s, d) for s, _ in SEGMENTS for d in (-1, 0, 1)}
S_TWO_SEAMS = {s: "s%d:run_crosses_two_seams" % s for s, _ in SEGMENTS}
S_TAGS = tuple(S_CROSS_PEAK.values()) + tuple(S_AT_SEAM.values()) + tuple(S_TWO_SEAMS.values())


def geometry_tags(info, peaks, rna):
    """the G_* / S_* tags of a read, from the model's peaks and runs"""
    tags = set()
    n = info["n"]
    if n == 0:
        return tags
    lead, own = lanes_whole(n, rna)
    ends = {}
    for r in info["runs"]:
        cb = _lane_of(own, min(r.b, n - 1))
        if r.sure_hot:
            ends[cb] = ends.get(cb, 0) + 1
            if cb - _lane_of(own, r.a) >= 3:
                tags.add(G_RUN_SPANS_CHUNKS)
        for x in r.peaks:
            cx = _lane_of(own, x)
            tags.add(G_IN_RECORDING_LANE if cx == cb else G_IN_EARLIER_LANE)
            if r.b == n:
                tags.add(G_RUN_AT_END_EMITS)
            if cx > 0 and x == own[cx][0]:
                tags.add(G_AT_CHUNK_FIRST)
            if cx < len(own) - 1 and x == own[cx][1] - 1:
                tags.add(G_AT_CHUNK_LAST)
            for s, _ in own[1:]:
                if s - lead <= x < s and r.b < s:
                    tags.add(G_IN_WARMUP)
        for seg, lmin in SEGMENTS:
            if n >= lmin:
                if r.sure_hot and min(r.b, n - 1) // seg - r.a // seg >= 2:
                    tags.add(S_TWO_SEAMS[seg])
                for x in r.peaks:
                    if x // seg < min(r.b, n - 1) // seg:
                        tags.add(S_CROSS_PEAK[seg])
                    for d in (-1, 0, 1):
                        if x - d >= seg and (x - d) % seg == 0:
                            tags.add(S_AT_SEAM[(seg, d)])
    all_runs = {}
    for r in info["runs"]:
        cb = _lane_of(own, min(r.b, n - 1))
        all_runs[cb] = all_runs.get(cb, 0) + 1
    if ends and max(ends.values()) > LZ_NREC:
        tags.add(G_NREC_OVER)
    if ends and max(ends.values()) == LZ_NREC and max(all_runs.values()) == LZ_NREC:
        tags.add(G_NREC_8)
    for x, i in info["short_emits"]:
        d = i - x
        tags |= {G_DELAY_ERARE} if 17 <= d <= 224 else {G_DELAY_OLDPEAK} if 225 <= d <= 511 else {G_DELAY_SLOW} if d > 512 else set()
        if _lane_of(own, x) < _lane_of(own, i):
            tags.add(G_SHORT_PRE)
    pk = np.sort(np.asarray([x for x, _ in peaks], dtype=np.int64))
    if pk.size > BUILD_MAX_BOUNDARIES and (pk[BUILD_MAX_BOUNDARIES:] - pk[:-BUILD_MAX_BOUNDARIES] < BUILD_TILE).any():
        tags.add(G_DENSE)
    if (rna, n) in G_LEN_32768:
        tags.add(G_LEN_32768[(rna, n)])
    return tags


# ---------------------------------------------------------------- building blocks
#: the issue's DNA seed without its plateaus: 876 -> 931 in 23 samples
DNA_RISE = (877, 877, 878, 879, 881, 883, 885, 889, 895, 903, 911, 917, 921, 923, 925, 927, 928, 929, 929, 930, 930, 930, 930)


class Case(NamedTuple):
    name: str
    raw: np.ndarray
    rna: tuple                     # the presets it is run with
    note: str = ""


class PaCase(NamedTuple):
    name: str
    pa: np.ndarray
    rna: int
    note: str = ""


def cat_(*parts):
    parts = [np.asarray(x, dtype=np.int64) for x in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def flat(n, v):
    return np.full(int(n), int(v), dtype=np.int64)


def sig(*parts):
    """plateaus (length, level) in a row"""
    return cat_(*[flat(n, v) for n, v in parts])


def ramp(a, b, n):
    """n samples on the integer line from a towards b (b itself is the first sample behind it)"""
    k = np.arange(n, dtype=np.int64)
    return a + ((b - a) * k + (n // 2 if b >= a else -(n // 2))) // n if b >= a else a - ((a - b) * k + n // 2) // n


def smooth(a, b, n):
    """n samples of a smooth (cubic, 3u^2 - 2u^3) transition from a to b, in integer arithmetic"""
    k = np.arange(1, n + 1, dtype=np.int64)
    num = (3 * k * k * (n + 1) - 2 * k * k * k)
    den = (n + 1) ** 3
    d = abs(b - a)
    step = (d * num + den // 2) // den
    return a + step if b >= a else a - step


def dna_seed(front=42, back=75, base=0):
    return cat_(flat(front, 876 + base), np.asarray(DNA_RISE) + base, flat(back, 931 + base))


def rna_seed(front=60, back=80):
    """the issue's RNA seed: a plateau, a 20-sample smooth rise, a 40-sample plateau, a smooth fall"""
    return cat_(flat(front, 1143), smooth(1143, 1283, 20), flat(40, 1283), smooth(1283, 1226, 20), flat(back, 1226))


def train(seed, n, kinds=("smooth", "ramp", "step"), plateau=(8, 90), width=(4, 40), noise=0):
    """a seeded row of plateaus joined by smooth transitions, integer ramps and single steps"""
    rs = np.random.RandomState(seed)
    out, level, have = [], int(rs.randint(500, 1100)), 0
    while have < n:
        L = int(rs.randint(*plateau))
        nxt = int(np.clip(level + rs.choice((-1, 1)) * rs.randint(4, 160), 200, 1500))
        kind = kinds[int(rs.randint(len(kinds)))]
        w = int(rs.randint(*width))
        tr = smooth(level, nxt, w) if kind == "smooth" else ramp(level, nxt, w) if kind == "ramp" else np.zeros(0, dtype=np.int64)
        out += [flat(L, level), tr]
        have += L + tr.size
        level = nxt
    x = cat_(*out)[:n]
    if noise:
        x = x + rs.randint(-noise, noise + 1, size=n)
    return x


def steps(seed, n, every):
    """noise-free steps every `every` samples: every plateau is a hot run of the long detector"""
    rs = np.random.RandomState(seed)
    lv = rs.randint(300, 700, size=n // every + 1)
    lv[1:][lv[1:] == lv[:-1]] += 37
    return np.repeat(lv, every)[:n]


def decline(length, rna, onset=(), base=300):
    """a plateau, a linear rise of `length` samples (slope 8 per sample; `onset`: its first increments) that rolls off with
    a linearly falling slope, a plateau.  On a line the statistic is constant (4.5 with a window of 3, 6.55 with 7): the
    short peak that opened at the onset stays in decline, but by less than peak_height, until the rise ends
    -- or until the rounding of the float squares, which grows with the level, lifts a statistic above the peak's: with the
    DNA preset's peak_height of 0.2 that takes a rise from raw 0 to stay in decline for more than 512 indices"""
    inc = np.full(length, 8, dtype=np.int64)
    inc[:len(onset)] = onset
    rise = base + np.cumsum(np.concatenate([inc, np.arange(7, 0, -1)]))
    return cat_(flat(60, base), rise, flat(60, int(rise[-1])))


def analyse(raw, rna, variant=None):
    """-> (peaks, tags (E_*, G_*, S_*), info) of a raw read under a preset"""
    raw = np.asarray(raw, dtype=np.int16)
    t1, t2 = tstats(raw, rna)
    peaks, tags, info = peaks_model(t1, t2, rna, variant, both_flat(raw, PRESET[rna].w2))
    return peaks, tags | geometry_tags(info, peaks, rna), info


# ---------------------------------------------------------------- searched constants
def seed_read(rna, front, n, base=0):
    """a read of n samples that holds the preset's seed, `base` higher, behind a plateau of `front` samples"""
    if rna:
        return rna_seed(front, n - front - 80) + base
    return dna_seed(front, n - front - len(DNA_RISE), base)


def search_chunk_edge(rna, last):
    """`front` of seed_read(rna, front, 600) that puts a long boundary on the first (last) index of a lane's chunk"""
    want = G_AT_CHUNK_LAST if last else G_AT_CHUNK_FIRST
    for front in range(200, 232):
        if want in analyse(seed_read(rna, front, 600), rna)[1]:
            return front
    return None


#: `front` of seed_read(rna, front, 600): [rna] -> (first index of a chunk, last index)
CHUNK_EDGE_FRONT = {0: (212, 211), 1: (205, 204)}


def seam_read(rna, front2048, front3072):
    """3 500 samples with the preset's seed near sample 2048 and, behind a step back to its first level, near 3072"""
    return cat_(seed_read(rna, front2048, 2560), seed_read(rna, front3072 - 2560, 940))


def search_seam(rna, d):
    """(front2048, front3072) of seam_read that put long boundaries at 2048 + d and at 3072 + d"""
    out = []
    for seam in (2048, 3072):
        found = None
        for front in range(seam - 80, seam + 20):
            x = seam_read(rna, front, 3000) if seam == 2048 else seam_read(rna, 1900, front)
            if seam + d in analyse(x, rna)[2]["long"]:
                found = front
                break
        out.append(found)
    return tuple(out)


#: [rna][d] -> (front2048, front3072) of seam_read
SEAM_FRONT = {0: {-1: (2019, 3043), 0: (2020, 3044), 1: (2021, 3045)}, 1: {-1: (1999, 3023), 0: (2000, 3024), 1: (2001, 3025)}}


def nrec_read(rna, front, over):
    """noise-free plateaus, long enough for both long windows to be constant inside each (a certainly hot run per
    plateau), behind a first plateau of `front` samples: 13 / 8 per 160-sample chunk with the DNA preset at 10 000 samples,
    11 / 8 per 320-sample chunk with the RNA preset at 20 000"""
    n, every = ((20000, 28 if over else 40) if rna else (10000, 12 if over else 20))
    return cat_(flat(front, 480), steps(7 + rna, n - front, every))


def search_nrec8(rna):
    for front in range(0, 200, 4):
        t = analyse(nrec_read(rna, front, False), rna)[1]
        if G_NREC_8 in t and G_NREC_OVER not in t:
            return front
    return None


#: `front` of nrec_read(rna, front, over=False)
NREC8_FRONT = {0: 36, 1: 132}


def search_decline_onset(rna):
    """the first increments of decline(120, rna, onset) with which the short peak of the onset is emitted >= 100 behind"""
    import itertools
    for on in itertools.product(range(0, 17, 2), repeat=3):
        info = analyse(decline(120, rna, on), rna)[2]
        if max([i - x for x, i in info["short_emits"]], default=0) >= 100:
            return on
    return None


DECLINE_ONSET = {0: (0, 6, 6), 1: (0, 0, 0)}


def search_decline_slow():
    """the first increments of decline(560, 0, onset, base=0) whose short peak is emitted more than 512 behind (DNA preset)"""
    import itertools
    for on in itertools.product(range(0, 17, 2), repeat=3):
        info = analyse(decline(560, 0, on, 0), 0)[2]
        if max([i - x for x, i in info["short_emits"]], default=0) > RING:
            return on
    return None


DECLINE_SLOW_DNA = (0, 8, 6)


def run_searches():
    return {"CHUNK_EDGE_FRONT": {r: (search_chunk_edge(r, False), search_chunk_edge(r, True)) for r in (0, 1)},
            "SEAM_FRONT": {r: {d: search_seam(r, d) for d in (-1, 0, 1)} for r in (0, 1)},
            "NREC8_FRONT": {r: search_nrec8(r) for r in (0, 1)},
            "DECLINE_ONSET": {r: search_decline_onset(r) for r in (0, 1)}, "DECLINE_SLOW_DNA": search_decline_slow(),
            "PA_EQUAL": {k: search_pa_equal(w, t, at, j, rna, tag) for k, (w, t, at, j, rna, tag) in PA_EQUAL_WANT.items()}}


def pa_equal(w, d_bits, e_bits, at=20):
    """a pA array whose statistic of window w at index `at` is decided by two floats (given as their bits): a step from 10
    to D at sample `at`, the two samples behind it D + e and D - e.  (at == w: the first index that has a statistic; the
    detector comes to it with peak_value 0)"""
    D, e = np.array([d_bits, e_bits], dtype=np.uint32).view(F)
    x = np.full(at + 20 + w, 10.0, dtype=F)
    x[at:] = D
    x[at + 1], x[at + 2] = D + e, D - e
    return x


def search_pa_equal(w, target, at=20, j=None, rna=0, tag=None, max_d=20000):
    """-> (bits of D, bits of e) for which the statistic of pa_equal at index j (default: at) equals `target` as a float
    and the model takes branch `tag`: for D = 11 and the floats above it, the e at which the (falling) statistic crosses
    the target is bisected and its neighbours tried"""
    target = F(target)
    D = F(11.0)
    j = at if j is None else j

    def x_of(D, e):
        return pa_equal(w, int(D.view(np.uint32)), int(F(e).view(np.uint32)), at)

    def t_at(D, e):
        s, q = prefix_sums(x_of(D, e))
        return tstat(s, q, w)[j]
    for _ in range(max_d):
        lo, hi = F(0.05), F(60.0)
        for _ in range(60):
            mid = F((np.float64(lo) + np.float64(hi)) / 2)
            if mid == lo or mid == hi:
                break
            if t_at(D, mid) > target:
                lo = mid
            else:
                hi = mid
        for v in (np.nextafter(lo, F(0)), lo, hi, np.nextafter(hi, F(100))):
            if t_at(D, v) == target and (tag is None or tag in peaks_model(*tstats_pa(x_of(D, v), rna), rna)[1]):
                return int(D.view(np.uint32)), int(v.view(np.uint32))
        D = np.nextafter(D, F(200))
    return None


#: name -> (window, target, at, j, preset, the branch it must take): thr1 as a peak's value and peak_height as the first
#: statistic of a read (the detector comes to it with peak_value 0), with both presets; a long statistic equal to thr2
PA_EQUAL_WANT = {"dna_t1==thr1": (3, PRESET[0].thr1, 20, 19, 0, E_PV_EQ_THR[0]), "rna_t1==thr1": (7, PRESET[1].thr1, 20, 20, 1, E_PV_EQ_THR[0]),
                 "dna_t1==peak_height": (3, PRESET[0].ph, 3, 3, 0, E_RISE_EQ_PH[0]), "rna_t1==peak_height": (7, PRESET[1].ph, 7, 7, 1, E_RISE_EQ_PH[0]),
                 "dna_t2==thr2": (6, 9.0, 20, 20, 0, None), "rna_t2==thr2": (14, 9.0, 20, 20, 1, None)}
#: name -> (bits of D, bits of e) of pa_equal
PA_EQUAL = {"dna_t1==thr1": (1093664771, 1092290196), "rna_t1==thr1": (1093664804, 1073573941),
            "dna_t1==peak_height": (1093664768, 1093252259), "rna_t1==peak_height": (1093664768, 1084122194),
            "dna_t2==thr2": (1093664820, 1056005585), "rna_t2==thr2": (1093664874, 1066192405)}


# ---------------------------------------------------------------- the catalogue
BOTH = (0, 1)
#: seeds of train(seed, 1500, kinds) that the mining run kept: between them they take every branch of the long detector
TRAIN_SEEDS = ((0, ("smooth",)), (3, ("smooth",)), (15, ("smooth",)), (37, ("smooth",)), (48, ("smooth",)), (61, ("smooth",)),
               (96, ("smooth",)), (17, ("smooth",)), (17, ("ramp",)), (48, ("ramp",)), (55, ("ramp",)), (0, ("smooth", "ramp", "step")),
               (22, ("smooth", "ramp", "step")), (41, ("smooth", "ramp", "step")), (76, ("smooth", "ramp", "step")))
#: two smooth transitions (width, width, plateau between, height, height) with a long boundary between two short ones that
#: lie 17 (DNA) / 30 (RNA) apart: the closest 3 000 random pairs gave
BETWEEN = {0: (25, 4, 11, 131, 49), 1: (34, 14, 28, 154, 47)}
LENGTH_EDGES = (0, 1, 2, 5, 6, 7, 11, 12, 13, 14, 15, 27, 28, 29)


#: ... and one on which a mask that is one index too long changes the RNA preset's peaks
MASK_PAIR_RNA = (26, 57, 22, 71, 20)


def pair(w1, w2, gap, h1, h2):
    return cat_(flat(50, 800), smooth(800, 800 + h1, w1), flat(gap, 800 + h1), smooth(800 + h1, 800 + h1 + h2, w2), flat(60, 800 + h1 + h2))


def long_read(n, kinds):
    """n samples of seeded rows, 1 500 each"""
    return cat_(*[train(100 + k, 1500, kinds) for k in range((n + 1499) // 1500)])[:n]


def quiet_long(n, seed):
    """n samples of flat signal with noise of +-8, in which the long detector has nothing to do -- but for a seed (noise-
    free, with its plateaus) in every slot of 700 samples, DNA and RNA seed in turn: a long read's lanes have chunks of 512
    to 640 samples, so no lane meets more than 8 hot runs and the read stays on the fast path.  (The noise must not be
    too small for the level: the cold proof, sgk_long_cold, gives away 2^-19 of the windows' sums of squares, which at
    150 pA is 3/4 of the variance of a noise of +-3 raw units -- statistics from 4.7 on would count as hot -- and 1/8 of
    that of +-8: from 8.4 on, which pure noise reaches about once in 10^5 indices)"""
    rs = np.random.RandomState(seed)

    def noisy(length, level):
        return level + rs.randint(-8, 9, size=length)
    out = []
    for k in range(n // 1400 + 1):
        out += [noisy(280, 876), dna_seed(), noisy(280, 931), noisy(280, 1143), rna_seed(), noisy(200, 1226)]
    x = cat_(*out)
    assert x.size >= n
    return x[:n]


def catalogue():
    """-> list of Case, deterministic"""
    c = []

    def add(name, raw, note, rna=BOTH):
        raw = np.asarray(raw)
        assert raw.size == 0 or (raw.min() >= -32768 and raw.max() <= 32767)
        c.append(Case(name, np.ascontiguousarray(raw, dtype=np.int16), tuple(rna), note))
    # ---- the two seeds of the issue, and cut behind their long boundary's window
    add("dna_seed", dna_seed(), "a long boundary at 70 (t2 = 6.4e17: both long windows constant) behind short ones at 42 .. 65; the run is open at n")
    add("rna_seed", rna_seed(), "long boundaries at 47 (the long window leaves the plateau) and at 108")
    add("dna_seed_cut", dna_seed()[:76], "n = 70 + w2: the boundary's statistic is the last one the read has")
    add("rna_seed_cut", rna_seed()[:122], "n = 108 + w2")
    add("seed_300_dna", seed_read(0, 100, 300), "300 samples, the run of the long boundary is open at n")
    add("seed_300_rna", cat_(flat(178, 1143), rna_seed()[:122]), "the same with the RNA seed, cut 14 samples behind its second boundary")
    # ---- lengths around 2 w1 and 2 w2 of both presets: a step in the middle
    for n in LENGTH_EDGES:
        add("len_%d" % n, sig((n // 2, 500), (n - n // 2, 700)), "")
    add("const_3000", flat(3000, 500), "constant: every statistic 0, one run from 1 to n that is hot all the way")
    add("zeros_700", flat(700, 0), "raw 0")
    # ---- seeded rows of plateaus, smooth transitions, ramps and steps without noise
    for seed, kinds in TRAIN_SEEDS:
        add("row_%s_%d" % ("mix" if len(kinds) > 1 else kinds[0], seed), train(seed, 1500, kinds), "")
    for seed in (1, 2):
        add("row_noise_%d" % seed, train(seed, 3000, noise=2), "the same with noise of +-2: what the old inputs look like")
    for rna in BOTH:
        add("between_%s" % "dr"[rna], pair(*BETWEEN[rna]), "a long boundary between two short ones %d apart" % (30 if rna else 17))
    add("mask_pair_r", pair(*MASK_PAIR_RNA), "the first index behind the mask decides (RNA preset)")
    # ---- a short peak that stays in decline by less than peak_height for 120 / 300 / 600 indices
    for rna in BOTH:
        for L in (120, 300, 600):
            add("decline_%s_%d" % ("dr"[rna], L), decline(L, rna, DECLINE_ONSET[rna]), "emitted %d behind its position" % L)
    add("decline_d_560_low", decline(560, 0, DECLINE_SLOW_DNA, 0), "from raw 0: emitted 526 behind its position with the DNA preset")
    # ---- a long boundary on the first / last index of a lane's chunk (16 samples at this length)
    for rna in BOTH:
        for j, what in enumerate(("first", "last")):
            add("chunk_%s_%s" % (what, "dr"[rna]), seed_read(rna, CHUNK_EDGE_FRONT[rna][j], 600), "")
    # ---- ... at, in front of and behind the seams of segments of 1024 / 2048 / 3072 samples
    for rna in BOTH:
        for d in (-1, 0, 1):
            add("seam%+d_%s" % (d, "dr"[rna]), seam_read(rna, *SEAM_FRONT[rna][d]), "long boundaries at 2048%+d and 3072%+d" % (d, d))
        add("two_seams_%s" % "dr"[rna], cat_(seed_read(rna, 900, 3300), flat(200, 700)),
            "the run of the boundary near 930 ends at 3300: over the seams at 1024, 2048 and 3072")
    add("two_seams_long_d", cat_(seed_read(0, 1900, 6400), flat(200, 700)), "... near 1930 to 6400: over 2048 and 4096, 3072 and 6144")
    add("two_seams_long_r", seed_read(1, 6300, 6600), "the read's first run, hot all the way, ends behind its boundary at 6287 (RNA preset; "
        "behind the RNA seed a short peak stays in decline for as long as the plateau lasts)")
    # ---- more hot runs in a chunk than a lane records (8)
    for rna in BOTH:
        add("nrec_over_%s" % "dr"[rna], nrec_read(rna, 0, True), "13 (DNA) / 11 (RNA) certainly hot runs per chunk: the exact fallback")
        add("nrec_8_%s" % "dr"[rna], nrec_read(rna, NREC8_FRONT[rna], False), "8 runs in a chunk and in none more: stays on the fast path")
    add("dense_6000", np.repeat(np.tile([420, 610], 1001), 3)[:6000], "a step every 3 samples: more than 512 boundaries in 2048 samples")
    # ---- chunks of 512 - 640 samples, warm-ups of 64 / 256, the 32 768-sample rule
    add("long_40000_smooth", long_read(40000, ("smooth",)), "noise-free: dozens of hot runs per chunk, fast only in segments")
    add("long_40000_quiet", quiet_long(40000, 1), "both seeds 31 times in noise: the fast path of a read with chunks of 624 samples")
    for n in (32767, 32768, 32769):
        add("long_%d" % n, quiet_long(n, n), "either side of the length at which the warm-up doubles")
    names = [k.name for k in c]
    assert len(set(names)) == len(names)
    return c


def pa_sig(*parts):
    return np.concatenate([np.full(int(n), v, dtype=F) for n, v in parts])


def pa_cases():
    """pA arrays straight into sgk_event_pa: what raw reads cannot hold"""
    out = []
    for name, (w, target, at, j, rna, tag) in PA_EQUAL_WANT.items():
        out.append(PaCase(name, pa_equal(w, *PA_EQUAL[name], at), rna, "the statistic of window %d at index %d is %r" % (w, j, target)))
    for rna in BOTH:
        out.append(PaCase("neg_zero_%s" % "dr"[rna], pa_sig((40, -0.0), (30, 3.5), (40, -0.0), (30, 0.0), (40, -0.0), (25, -7.25), (40, -0.0)),
                          rna, "-0.0 plateaus between levels and +0.0"))
    return out


def catalogue_sha256() -> str:
    h = hashlib.sha256()
    for k in catalogue():
        h.update(k.name.encode() + b"\0" + k.raw.tobytes() + repr(k.rna).encode())
    for k in pa_cases():
        h.update(k.name.encode() + b"\0" + k.pa.tobytes() + repr(k.rna).encode())
    return h.hexdigest()


def case_runs(k):
    """the (label, preset) a case is run with"""
    return [("%s/rna%d" % (k.name, rna), rna) for rna in k.rna]


def tag_table(cat=None):
    """-> ({tag: [labels of the runs it fires on]}, {label: the long detector's boundaries}) over the catalogue, and
    ("pa " + tag) over the pA arrays"""
    table, longs = {}, {}
    for k in cat or catalogue():
        for label, rna in case_runs(k):
            peaks, tags, info = analyse(k.raw, rna)
            longs[label] = info["long"]
            for t in tags:
                table.setdefault(t, []).append(label)
    for k in pa_cases():
        tags = peaks_model(*tstats_pa(k.pa, k.rna), k.rna)[1]
        if ((k.pa == 0) & np.signbit(k.pa)).any():
            tags = tags | {E_NEG_ZERO}
        for t in tags:
            table.setdefault("pa " + t, []).append(k.name)
    return table, longs


if __name__ == "__main__":
    for name, v in run_searches().items():
        print("%s = %r" % (name, v))
    cat = catalogue()
    table, longs = tag_table(cat)
    for t in E_TAGS + G_TAGS + tuple(G_LEN_32768.values()) + S_TAGS + tuple("pa " + t for t in E_TAGS_PA + (E_NEG_ZERO,)):
        names = table.get(t, [])
        print("%-78s %3d  %s" % (t, len(names), ", ".join(names[:3])))
    print("%d reads, %d samples, longest %d; %d runs with a long-detector boundary, %d such boundaries" % (
        len(cat), sum(k.raw.size for k in cat), max(k.raw.size for k in cat), sum(1 for v in longs.values() if v),
        sum(len(v) for v in longs.values())))
    print(catalogue_sha256())


def ref_cli_prints(raw):
    """the reference's command line tool ends in a failed assertion of its trimming pass (which `event` then discards) unless
    some 100-sample chunk of the read has a median absolute deviation above the smallest one: never below 200 samples"""
    raw = np.asarray(raw, dtype=np.float64)
    nchunk = raw.size // 100
    if nchunk < 2:
        return False
    ch = raw[:nchunk * 100].reshape(nchunk, 100)
    mad = np.sort(np.abs(ch - np.sort(ch, axis=1)[:, 50:51]), axis=1)[:, 50]
    return bool(mad.max() > mad.min())


def cli_cases(cat=None):
    """the reads of the CLI goldens (tests/golden/event_cases_*.tsv; `event` prints a row per event): every read of up to
    7 000 samples on which the long detector emits a boundary with either preset and that the reference's tool prints (not
    the two bare seeds and their cuts, nor the length edges: those are pinned through its library, ref_vectors.json)"""
    out = []
    for k in cat or catalogue():
        if k.raw.size <= 7000 and ref_cli_prints(k.raw) and any(analyse(k.raw, rna)[2]["long"] for rna in k.rna):
            out.append(k)
    return out
