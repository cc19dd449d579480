"""The catalogue of hand-made reads for `jnn` and a plain branch model of its segmenter.

jnn_core (the reference's src/jnn.c:190-278) is an error-tolerant run finder over the clamped signal: a segment opens at
an in-range sample, tolerates `error` out-of-range samples, is kept when it ends after `window` samples (or, while
nothing has been kept, after window * stall_len), and is merged into the previous kept one when it starts less than
seg_dist behind its end.  `jnn_core_model` restates it as a literal loop and returns, besides the segments, the SET OF
BRANCHES that fired (the J_* tags).  The GPU has the loop four times, two of them in a very different form (chunks
between data-determined sync points, a flag-scan merge, rounds of 64 chunks with a carry): `geometry_tags` works out from
the model's segment and streak positions, with the kernels' constants restated below, which of THEIR special places a
read touches (the G_* tags).  test_jnn_cases_cpu.py proves the model equal to the oracle on every read and requires
every tag to fire somewhere: that is what keeps this catalogue from going soft.

The reads are built from plateaus, dips and single outliers (`io`: in-range runs at one level, out-of-range samples
alternately below and above it, so that mean +- 0.75 sd separates them whatever the mix).  Where a branch needs tuning
-- the first sync sample exactly at a chunk's end, a merge across two merge rounds -- a small search function
(`search_*`) finds the parameter, and what it found is committed next to it as a constant: building the catalogue runs
no search.  `python tests/jnn_cases.py` reruns the searches and prints the constants and the tag -> read table.

Numbers: the two sequential float sums (meanf, stdvf) are np.cumsum in float32, which adds strictly in order.
"""
import hashlib
from typing import NamedTuple, Optional

import numpy as np

from prefix_cases import F, meanf, stdvf

# ---- branch tags: the reference's loop
J_OPEN_AT_0 = "j:open_at_0"
J_OPEN_LATER = "j:open_later"
J_TOLERATED = "j:tolerated_error"
J_KEPT_WINDOW = "j:kept_c>=window"
J_KEPT_FIRST = "j:kept_by_first_segment_rule"
J_WEAK_DROPPED = "j:weak_after_first_dropped"
J_C_FIRST_MIN = "j:c==first_min_kept"
J_C_FIRST_MIN_M1 = "j:c==first_min-1_rejected"
J_C_WINDOW = "j:c==window_kept_after_first"
J_C_WINDOW_M1 = "j:c==window-1_dropped_after_first"
J_MERGE = "j:merged"
J_MERGE_DIST_M1 = "j:merge_at_seg_dist-1"
J_NOMERGE_DIST = "j:no_merge_at_seg_dist"
J_ABANDONED = "j:abandoned"
J_TRAIL = "j:trailing_errors_cut"
J_NO_TRAIL = "j:no_trailing_errors"
J_BUDGET = "j:budget_exhausted_scattered"
J_OPEN_END = "j:open_at_end_dropped"
J_EQ_TOP = "j:sample==top"
J_EQ_BOT = "j:sample==bot"
J_HI_1200 = "j:top==1200_clamped_sample_out"
J_HI_1201 = "j:top_in_(1200,1201]_clamped_sample_in"
J_LO_0 = "j:bot==0_clamped_sample_out"
J_LO_M1 = "j:bot_in_[-1,0)_clamped_sample_in"
J_TOP_LE_0 = "j:top<=0"
J_BOT_GE_1200 = "j:bot>=1200"
J_NAN_THR = "j:nan_threshold"
J_N1 = "j:n==1"
J_CONST = "j:sd==0"
J_CORRECTION = "j:err--"
J_CORRECTION_TWICE = "j:err--_twice_in_one_segment"
J_NONE = "j:nothing_found"
J_TAGS = (J_OPEN_AT_0, J_OPEN_LATER, J_TOLERATED, J_KEPT_WINDOW, J_KEPT_FIRST, J_WEAK_DROPPED, J_C_FIRST_MIN,
          J_C_FIRST_MIN_M1, J_C_WINDOW, J_C_WINDOW_M1, J_MERGE, J_MERGE_DIST_M1, J_NOMERGE_DIST, J_ABANDONED, J_TRAIL,
          J_NO_TRAIL, J_BUDGET, J_OPEN_END, J_EQ_TOP, J_EQ_BOT, J_HI_1200, J_HI_1201, J_LO_0, J_LO_M1, J_TOP_LE_0,
          J_BOT_GE_1200, J_NAN_THR, J_N1, J_CONST, J_CORRECTION, J_CORRECTION_TWICE, J_NONE)
#: what the two presets must reach through the subtool (fixed thresholds and error >= corrector need own parameters)
J_TAGS_PRESET = (J_OPEN_AT_0, J_OPEN_LATER, J_TOLERATED, J_KEPT_WINDOW, J_MERGE, J_MERGE_DIST_M1, J_NOMERGE_DIST,
                 J_ABANDONED, J_TRAIL, J_NO_TRAIL, J_BUDGET, J_OPEN_END, J_N1, J_CONST, J_NONE, J_C_WINDOW, J_C_WINDOW_M1)
#: ... and what only the cDNA preset can (with stall_len 1 the first-segment rule is the window rule)
J_TAGS_CDNA = (J_KEPT_FIRST, J_WEAK_DROPPED, J_C_FIRST_MIN, J_C_FIRST_MIN_M1)
#: only pA arrays can hold these
J_NAN_SAMPLE = "j:nan_sample"
J_INF_SAMPLE = "j:inf_sample"
J_NEG_ZERO = "j:-0.0_sample"
J_TAGS_PA = (J_NAN_SAMPLE, J_INF_SAMPLE, J_NEG_ZERO, J_EQ_TOP, J_EQ_BOT, J_NAN_THR, J_CORRECTION, J_CORRECTION_TWICE)

# ---- geometry tags: places of the wave-per-read kernel (one wave, C <= 64 chunks) ...
CHUNK_COUNTS = (1, 2, 63, 64)
CHUNK_NQ = (511, 512, 513, 16127, 16128, 16383, 16384)
G_C = {c: "g:chunks==%d" % c for c in CHUNK_COUNTS}
G_NQ = {n: "g:nq==%d" % n for n in CHUNK_NQ}
G_SYNC_CE_M2 = "g:streak's_first_sync_at_ce-2_run_ends_on_its_second"
G_SYNC_CE_M1 = "g:streak's_first_sync_at_ce-1"
G_SYNC_CE = "g:streak's_first_sync_at_ce"
G_OPEN_CE_M1 = "g:sync_at_ce-2_segment_opens_at_ce-1"
G_SYNC_BLOCK_FIRST = "g:run_ends_on_first_sample_of_block"
G_SYNC_BLOCK_LAST = "g:run_ends_on_last_sample_of_block"
G_STREAK_E1_STRADDLE = "g:streak_of_error+1_straddles_chunk_end"
G_STREAK_E_STRADDLE = "g:streak_of_error_straddles_chunk_end"
G_SEG_SPANS_CHUNK = "g:segment_spans_whole_chunk"
G_END_NO_SYNC = "g:segment_ended_by_scattered_errors_no_sync"
G_WEAK_FIRST_LANE = "g:weak_first_candidate_in_lane>0"
G_WEAK_NOT_FIRST_DROPPED = "g:weak_first_of_lane_behind_other_lane's_candidate"
G_MERGE_IN_LANE = "g:merge_within_lane"
G_MERGE_ACROSS = "g:merge_across_lanes"
G_MERGE_ACROSS_EMPTY = "g:merge_across_empty_lanes"
G_MERGE_ACROSS_DIST_M1 = "g:merge_across_lanes_at_seg_dist-1"
G_NOMERGE_ACROSS_DIST = "g:no_merge_across_lanes_at_seg_dist"
G_STAGE_OVERFLOW = "g:lane_stages_more_than_capL"
G_ERROR_0 = "g:error==0_every_out_sample_syncs"
G_ERROR_31 = "g:error==31_streak_of_a_block"
# ... and of the long-read chains (C up to 4096 chunks, merged in rounds of 64 with a carry)
L_TWO_ROUNDS = "l:two_merge_rounds"
L_WEAK_FIRST_ROUND2 = "l:weak_first_candidate_in_round>=2"
L_WEAK_NOT_FIRST_ROUND2 = "l:weak_first_of_lane_in_round>=2_dropped"
L_MERGE_ACROSS_ROUNDS = "l:merge_across_rounds"
L_NOMERGE_ACROSS_ROUNDS = "l:no_merge_across_rounds"
L_LAST_BY_NEXT = "l:round's_last_segment_decided_by_next_round"
L_LAST_BY_FLUSH = "l:round's_last_segment_decided_by_flush"
L_STAGE_OVERFLOW = "l:chunk_stages_more_than_capL-2"
G_TAGS = tuple(G_C.values()) + tuple(G_NQ.values()) + (
    G_SYNC_CE_M2, G_SYNC_CE_M1, G_SYNC_CE, G_OPEN_CE_M1, G_SYNC_BLOCK_FIRST, G_SYNC_BLOCK_LAST, G_STREAK_E1_STRADDLE, G_STREAK_E_STRADDLE,
    G_SEG_SPANS_CHUNK, G_END_NO_SYNC, G_WEAK_FIRST_LANE, G_WEAK_NOT_FIRST_DROPPED, G_MERGE_IN_LANE, G_MERGE_ACROSS,
    G_MERGE_ACROSS_EMPTY, G_MERGE_ACROSS_DIST_M1, G_NOMERGE_ACROSS_DIST, G_STAGE_OVERFLOW, G_ERROR_0, G_ERROR_31,
    L_TWO_ROUNDS, L_WEAK_FIRST_ROUND2, L_WEAK_NOT_FIRST_ROUND2, L_MERGE_ACROSS_ROUNDS, L_NOMERGE_ACROSS_ROUNDS,
    L_LAST_BY_NEXT, L_LAST_BY_FLUSH, L_STAGE_OVERFLOW)


class JP(NamedTuple):              # jnn_param_t
    std_scale: float
    corrector: int
    seg_dist: int
    window: int
    stall_len: float
    error: int
    top: float
    bot: float


PRESET = {0: JP(0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0), 1: JP(0.75, 50, 50, 1000, 1.0, 5, 0.0, 0.0)}
POLYA = JP(-1.0, 50, 200, 250, 1.0, 30, 600.0, 400.0)    # the polyA preset with fixed thresholds


def wave_ok(p: JP) -> bool:
    """the launch rule: these parameters may take the wave-per-read kernel (no err-- can fire, E1 fits a block)"""
    return p.error >= 0 and p.error < p.corrector and p.error <= 31 and p.window >= 128


def clamp_raw(raw):
    return np.clip(np.asarray(raw, dtype=np.int64), 0, 1200).astype(F)


def clamp_pa(pa):
    with np.errstate(invalid="ignore"):
        s = np.asarray(pa, dtype=F).copy()
        s[s > 1200] = 1200
        s[s < 0] = 0
    return s


class Closed(NamedTuple):          # a segment the loop ended with c >= min(window, first_min): a kernel's "candidate"
    start: int
    i: int                         # the sample that ended it
    end: int                       # i - the trailing errors
    c: int
    kept: bool


NO_MOD = "no c % w"


def jnn_core_model(sig, p: JP, correction=True):
    """-> (segments [(x, y)], tags, info): jnn_core on the clamped float signal.  info: the in-range flags and the ended
    segments a chunk of the wave kernel would report.  Two deliberately WRONG loops, for the tests that show that the
    catalogue tells them from the right one: correction=False leaves the err-- out (what the wave kernel runs: right
    only while error < corrector), correction=NO_MOD drops the `c % w == 0` term of its condition"""
    tags = set()
    sig = np.asarray(sig, dtype=F)
    n = sig.size
    if n == 1:
        tags.add(J_N1)
    with np.errstate(all="ignore"):
        if p.std_scale > 0:
            mn, sd = meanf(sig), stdvf(sig)
            band = sd * F(p.std_scale)
            top, bot = mn + band, mn - band
            if sd == 0:
                tags.add(J_CONST)
        else:
            top, bot = F(p.top), F(p.bot)
        inr_a = (sig < top) & (sig > bot)
        if (sig == top).any():
            tags.add(J_EQ_TOP)
        if (sig == bot).any():
            tags.add(J_EQ_BOT)
        if np.isnan(top) or np.isnan(bot):
            tags.add(J_NAN_THR)
        if top <= 0:
            tags.add(J_TOP_LE_0)
        if bot >= 1200:
            tags.add(J_BOT_GE_1200)
        if (sig == 1200).any():
            if top == 1200:
                tags.add(J_HI_1200)
            if 1200 < top <= 1201 and bot < 1200:
                tags.add(J_HI_1201)
        if (sig == 0).any() and not np.signbit(sig[sig == 0]).all():
            if bot == 0:
                tags.add(J_LO_0)
            if -1 <= bot < 0 and top > 0:
                tags.add(J_LO_M1)
        first_min = float(F(p.window) * F(p.stall_len))
    first_min_i = int(np.ceil(first_min)) if np.isfinite(first_min) else 1 << 30
    inr = inr_a.tolist()
    prev, err, prev_err, c, w = False, 0, 0, 0, p.corrector
    window, error, seg_dist = p.window, p.error, p.seg_dist
    start, fired = 0, 0
    segs, closed = [], []
    for i in range(n):
        if inr[i]:
            if not prev:
                start, prev, fired = i, True, 0
                tags.add(J_OPEN_AT_0 if i == 0 else J_OPEN_LATER)
            c += 1
            w += 1
            prev_err = 0
            if correction and c >= window and c >= w and (c % w == 0 or correction == NO_MOD):
                err -= 1
                fired += 1
                tags.add(J_CORRECTION_TWICE if fired > 1 else J_CORRECTION)
        elif prev and err < error:
            c += 1
            err += 1
            prev_err += 1
            tags.add(J_TOLERATED)
            if correction and c >= window and c >= w and (c % w == 0 or correction == NO_MOD):
                err -= 1
                fired += 1
                tags.add(J_CORRECTION_TWICE if fired > 1 else J_CORRECTION)
        elif prev and (c >= window or (not segs and float(c) >= first_min)):
            end = i - prev_err
            prev = False
            if c >= window:
                tags.add(J_KEPT_WINDOW)
                if segs and c == window:
                    tags.add(J_C_WINDOW)
            else:
                tags.add(J_KEPT_FIRST)
                if c == first_min_i:
                    tags.add(J_C_FIRST_MIN)
            tags.add(J_TRAIL if prev_err > 0 else J_NO_TRAIL)
            if prev_err < error:
                tags.add(J_BUDGET)
            closed.append(Closed(start, i, end, c, True))
            if segs and start - segs[-1][1] < seg_dist:
                tags.add(J_MERGE)
                if start - segs[-1][1] == seg_dist - 1:
                    tags.add(J_MERGE_DIST_M1)
                segs[-1][1] = end
            else:
                if segs and start - segs[-1][1] == seg_dist:
                    tags.add(J_NOMERGE_DIST)
                segs.append([start, end])
            c = err = prev_err = 0
        elif prev:
            if segs and c == window - 1:
                tags.add(J_C_WINDOW_M1)
            if float(c) >= first_min:
                tags.add(J_WEAK_DROPPED)
                closed.append(Closed(start, i, i - prev_err, c, False))
            else:
                tags.add(J_ABANDONED)
                if not segs and c == first_min_i - 1:
                    tags.add(J_C_FIRST_MIN_M1)
            prev = False
            c = err = prev_err = 0
    if prev:
        tags.add(J_OPEN_END)
    if not segs:
        tags.add(J_NONE)
    return [tuple(s) for s in segs], tags, {"inr": inr_a, "closed": closed}


# ---------------------------------------------------------------- the kernels' geometry, restated
BLOCK, LINE = 32, 64               # samples a lane takes per step; per 128-byte line
LONG_MIN = 8192                    # the long-read threshold the tests configure
LC_WAVES = 64


def jnn_chunk_lanes(nq):
    return (64 if nq // 256 >= 64 else nq // 256) if nq >= 512 else 1


def jnn_long_chunks(nq):
    c, lanes = nq // 512, jnn_chunk_lanes(nq)
    return 64 * LC_WAVES if c > 64 * LC_WAVES else (c if c > lanes else lanes)


def chunk_len(nq, C):
    return ((nq + C - 1) // C + 7) & ~7


def slots(n):
    """-> (cap, half): the slots a read of n samples gets, and the part of them the merged segments go to"""
    cap = n // 32 + 2
    return cap, cap // 2


def lane_runs(inr, error, C):
    """-> (K, sync flags, [(b, e)] per chunk): chunk gc runs the automaton over the samples in (b, e] -- from behind the
    first sync sample at cs - 1 or later to the first sync sample at ce - 1 or later -- or nothing ((0, -1)).  A sync sample
    ends a streak of error + 1 out-of-range samples: behind it the automaton is closed whatever came before"""
    n = inr.size
    K = chunk_len(n, C)
    idx = np.arange(n)
    streak = idx - np.maximum.accumulate(np.where(inr, idx, -1))
    sync = streak >= error + 1
    spos = np.flatnonzero(sync)

    def S(p):
        k = int(np.searchsorted(spos, p))
        return int(spos[k]) if k < spos.size else n
    runs = []
    for gc in range(C):
        cs, ce = gc * K, (gc + 1) * K
        b = -1 if gc == 0 else S(cs - 1)
        if b >= n or b >= ce - 1:
            runs.append((0, -1))
        else:
            runs.append((b, S(ce - 1)))
    return K, sync, streak, runs


def _lane_of(runs, x):
    for gc, (b, e) in enumerate(runs):
        if b < x <= e:
            return gc
    raise AssertionError("sample %d lies in no chunk's run" % x)


def _boundary_tags(inr, sync, streak, runs, K, gc, error):
    """what the end of chunk gc (ce = its first sample behind) meets"""
    tags = set()
    n = inr.size
    ce = (gc + 1) * K
    if ce >= n or ce < 3:
        return tags
    b, e = runs[gc]
    if e >= b:
        if sync[ce - 2] and not sync[ce - 3] and e == ce - 1:
            tags.add(G_SYNC_CE_M2)
        if sync[ce - 1] and not sync[ce - 2]:
            tags.add(G_SYNC_CE_M1)
        if sync[ce] and not sync[ce - 1]:
            tags.add(G_SYNC_CE)
        if sync[ce - 2] and not sync[ce - 1]:
            tags.add(G_OPEN_CE_M1)
        if e < n and e % BLOCK == 0:
            tags.add(G_SYNC_BLOCK_FIRST)
        if e < n and e % BLOCK == BLOCK - 1:
            tags.add(G_SYNC_BLOCK_LAST)
    if not inr[ce - 1] and not inr[ce]:
        j = ce
        while j + 1 < n and not inr[j + 1]:
            j += 1
        L = int(streak[j])
        if j - L + 1 > 0:      # (a streak that starts the read is no streak inside a segment)
            if L == error + 1:
                tags.add(G_STREAK_E1_STRADDLE)
            if L == error and error > 0:
                tags.add(G_STREAK_E_STRADDLE)
    return tags


def _layout_tags(info, p, C, cap_l, long):
    tags = set()
    inr, closed = info["inr"], info["closed"]
    n = inr.size
    K, sync, streak, runs = lane_runs(inr, p.error, C)
    if not long:
        if C in G_C:
            tags.add(G_C[C])
        if n in G_NQ:
            tags.add(G_NQ[n])
        if p.error == 0:
            tags.add(G_ERROR_0)
        if p.error == 31 and (streak >= 32).any():
            tags.add(G_ERROR_31)
        for gc in range(C - 1):
            tags |= _boundary_tags(inr, sync, streak, runs, K, gc, p.error)
    lanes = [_lane_of(runs, k.start) for k in closed]
    for k in closed:
        if k.i // K - k.start // K >= 2:
            tags.add(G_SEG_SPANS_CHUNK)
        if k.kept and not sync[k.i] and not long:
            tags.add(G_END_NO_SYNC)
    seen_lanes = set()
    staged = {}
    for j, (k, la) in enumerate(zip(closed, lanes)):
        first_of_lane = la not in seen_lanes
        seen_lanes.add(la)
        weak = k.c < p.window
        if j == 0 and weak and la > 0:
            tags.add(L_WEAK_FIRST_ROUND2 if long and la >= 64 else G_WEAK_FIRST_LANE)
        if j > 0 and weak and first_of_lane:
            tags.add(L_WEAK_NOT_FIRST_ROUND2 if long and la >= 64 else G_WEAK_NOT_FIRST_DROPPED)
        if not first_of_lane and not weak:
            staged[la] = staged.get(la, 0) + 1
    if staged and max(staged.values()) > cap_l:
        tags.add(L_STAGE_OVERFLOW if long else G_STAGE_OVERFLOW)
    kept = [(k, la) for k, la in zip(closed, lanes) if k.kept]
    for (a, la), (b, lb) in zip(kept, kept[1:]):
        d = b.start - a.end
        merged = d < p.seg_dist
        if long:
            if la // 64 != lb // 64:
                tags.add(L_MERGE_ACROSS_ROUNDS if merged else L_NOMERGE_ACROSS_ROUNDS)
                tags.add(L_LAST_BY_NEXT)
            continue
        if merged:
            tags.add(G_MERGE_IN_LANE if la == lb else G_MERGE_ACROSS)
            if lb - la >= 2:
                tags.add(G_MERGE_ACROSS_EMPTY)
        if la != lb and d == p.seg_dist - 1:
            tags.add(G_MERGE_ACROSS_DIST_M1)
        if la != lb and d == p.seg_dist:
            tags.add(G_NOMERGE_ACROSS_DIST)
    if long and C > 64:
        tags.add(L_TWO_ROUNDS)
        if kept and kept[-1][1] // 64 < (C - 1) // 64:
            tags.add(L_LAST_BY_FLUSH)
    return tags


def geometry_tags(info, p: JP):
    """the G_* / L_* tags of a read that starts on a multiple of 8 samples, from the model's `info`"""
    if not wave_ok(p):
        return set()
    n = info["inr"].size
    cap, half = slots(n)
    C = jnn_chunk_lanes(n)
    tags = _layout_tags(info, p, C, (cap - half) // C, False)
    if p.std_scale > 0 and n >= LONG_MIN:
        C = jnn_long_chunks(n)
        cap_l = (cap - half) // C
        if cap_l >= 4:
            tags |= _layout_tags(info, p, C, cap_l - 2, True)
    return tags


# ---------------------------------------------------------------- building blocks
IN, LO, HI = 500, 300, 700


class Case(NamedTuple):
    name: str
    raw: np.ndarray
    params: Optional[JP]           # None: a preset case, run with both presets through the subtool
    note: str = ""


class PaCase(NamedTuple):
    name: str
    pa: np.ndarray
    params: JP
    note: str = ""


def sig(*parts):
    """plateaus (length, level) in a row"""
    return np.concatenate([np.full(int(n), int(v), dtype=np.int16) for n, v in parts])


def io(*runs, pad_to=0):
    """runs of in-range samples (n > 0: n samples at IN) and of outliers (n < 0: -n samples, alternately LO and HI over
    the whole read: mean +- 0.75 sd lies between IN and either); pad_to: outliers up to that length"""
    out = []
    k = 0
    runs = list(runs)
    have = sum(abs(r) for r in runs)
    if pad_to > have:
        runs.append(-(pad_to - have))
    for r in runs:
        if r > 0:
            out.append(np.full(r, IN, dtype=np.int16))
        elif r < 0:
            v = np.where((np.arange(-r) + k) % 2 == 0, LO, HI).astype(np.int16)
            k += -r
            out.append(v)
    return np.concatenate(out)


def rich(n, seed, error=5, window=150):
    """a seeded mix of in-range runs around the first-segment length and the window, and of outlier streaks around
    error, error + 1 and seg_dist; single outliers inside the runs"""
    rs = np.random.RandomState(seed)
    ins = [3, 20, 32, 33, 60, window - 6, window - 5, window, window + 40, 2 * window, 3 * window]
    outs = [1, 2, max(error - 1, 1), max(error, 1), error + 1, error + 2, 20, 44, 45, 49, 50, 51, 120]
    runs, have = [], 0
    while have < n:
        a, b = int(rs.choice(ins)), int(rs.choice(outs))
        runs += [a, -b]
        have += a + b
    x = io(*runs)[:n].copy()
    hits = np.flatnonzero(rs.rand(n) < 0.004)
    x[hits] = np.where(hits % 2 == 0, LO, HI)
    return x


def no_sync(k, body=150):
    """k segments in a row with no sync sample between them: `body` in-range samples, then outliers one by one (each
    followed by one in-range sample) until the sixth ends the segment; the next segment opens on the sample behind it"""
    one = [body] + [-1, 1] * 5 + [-1]
    return one * k


# ---------------------------------------------------------------- searched constants
def sync_read(lead, streak):
    """2048 samples, 8 chunks of 256: a strong segment from sample 10 to `lead`, `streak` outliers behind it, then
    segments that keep every later chunk end away from a sync sample's edge"""
    return io(-10, lead - 10, -streak, 230, -20, 300, -40, 200, -30, pad_to=2048)


SYNC_WANT = {"ce-2": (G_SYNC_CE_M2, 10), "ce-1": (G_SYNC_CE_M1, 10), "ce": (G_SYNC_CE, 10),
             "e1_straddle": (G_STREAK_E1_STRADDLE, 6), "e_straddle": (G_STREAK_E_STRADDLE, 5)}


def search_sync(what):
    """`lead` of sync_read for which the streak behind the first segment does what `what` names at the end of chunk 0"""
    tag, streak = SYNC_WANT[what]
    for lead in range(230, 270):
        if chunk0_end(sync_read(lead, streak)) == {tag}:
            return lead
    return None


def chunk0_end(raw, p=PRESET[0]):
    """which of SYNC_WANT's tags the end of chunk 0 of a 2048-sample read fires (8 chunks of 256)"""
    _, _, info = jnn_core_model(clamp_raw(raw), p)
    K, sync, streak, runs = lane_runs(info["inr"], p.error, 8)
    return _boundary_tags(info["inr"], sync, streak, runs, K, 0, p.error) & {t for t, _ in SYNC_WANT.values()}


#: `lead` of sync_read, per entry of SYNC_WANT
SYNC_LEAD = {"ce-2": 249, "ce-1": 250, "ce": 251, "e1_straddle": 252, "e_straddle": 252}


def rounds_read(gap, first=250):
    """40 000 samples, 78 chunks of 520 on the long path (merge rounds of 64: the second starts at sample 33 280):
    segments every 400 samples up to 30 000, then one that ends `gap` samples in front of one in the second round"""
    return io(*([250, -150] * 75), -2990, first, -gap, 300, -200, 400, pad_to=40000)


def search_rounds(want_merge):
    """`gap` of rounds_read at seg_dist - 1 (merged) / seg_dist for which the two segments lie in different rounds"""
    gap = PRESET[0].seg_dist - (1 if want_merge else 0)
    for first in range(200, 320):
        _, _, info = jnn_core_model(clamp_raw(rounds_read(gap, first)), PRESET[0])
        t = geometry_tags(info, PRESET[0])
        if (L_MERGE_ACROSS_ROUNDS if want_merge else L_NOMERGE_ACROSS_ROUNDS) in t:
            return first
    return None


#: `first` of rounds_read: (merged at seg_dist - 1, not merged at seg_dist)
ROUNDS_FIRST = (241, 200)


def run_searches():
    return {"SYNC_LEAD": {k: search_sync(k) for k in SYNC_WANT},
            "ROUNDS_FIRST": (search_rounds(True), search_rounds(False))}


# ---------------------------------------------------------------- the catalogue
def fixed(**kw):
    """own parameters with fixed thresholds 400 / 600 around IN; window 128, seg_dist 50, no first-segment rule"""
    d = dict(std_scale=-1.0, corrector=50, seg_dist=50, window=128, stall_len=1.0, error=5, top=600.0, bot=400.0)
    d.update(kw)
    return JP(**d)


#: one step either side of every term of the launch rule (wave: True)
RULE_PARAMS = {"error0": fixed(error=0), "error31": fixed(error=31), "error32": fixed(error=32),
               "window127": fixed(window=127), "error-1": fixed(error=-1),
               "error==corrector": fixed(corrector=8, error=8), "error==corrector-1": fixed(corrector=8, error=7),
               "polya": POLYA, "error0_std": fixed(error=0, std_scale=0.75), "error31_std": fixed(error=31, std_scale=0.6),
               "stall0.3": fixed(stall_len=0.3), "error>corrector": fixed(corrector=3, error=6, window=20, seg_dist=10)}


def catalogue():
    """-> list of Case, deterministic"""
    c = []

    def add(name, raw, note, params=None):
        c.append(Case(name, np.ascontiguousarray(raw, dtype=np.int16), params, note))
    # ---- sizes and constant reads
    add("n1", sig((1, 500)), "one sample: sd = 0, nothing in range")
    add("n2", sig((1, 400), (1, 600)), "two samples")
    add("const_500x3000", sig((3000, 500)), "constant: sd = 0, top == bot == every sample")
    add("const_above_clamp", sig((700, 2000)), "constant above 1200: clamped")
    add("const_below_clamp", sig((700, -50)), "constant below 0: clamped to 0")
    add("all_in_but_one", io(900, -1, 900), "one outlier: a tolerated error, the segment is open at the end")
    # ---- the automaton's branches (cDNA: window 150, first segment from 38, error 5; a segment that ends in a streak
    # has c = its in-range samples + 5)
    add("open_at_0", io(200, -20, 300, -30), "the first segment opens at sample 0")
    add("first_rule_38", io(-100, 33, -20, 200, -20), "c == 38 >= 37.5: kept as the first segment")
    add("first_rule_37", io(-100, 32, -20, 200, -20), "c == 37: not kept, the next one is the first")
    add("window_150", io(-50, 200, -60, 145, -60, 300, -10), "a later segment with c == window: kept")
    add("window_149", io(-50, 200, -60, 144, -60, 300, -10), "a later segment with c == window - 1: dropped")
    add("window_1000", io(-50, 1100, -60, 995, -60, 1300, -10), "the same for the dRNA preset's window")
    add("window_999", io(-50, 1100, -60, 994, -60, 1300, -10), "the same for the dRNA preset's window")
    add("weak_after_first", io(-50, 200, -100, 60, -100, 200, -20), "a segment of 65 behind the first: dropped")
    add("merge_49", io(-20, 200, -49, 200, -100), "gap seg_dist - 1: merged")
    add("nomerge_50", io(-20, 200, -50, 200, -100), "gap seg_dist: two segments")
    add("merge_49_rna", io(-20, 1200, -49, 1200, -100), "the same with segments the dRNA preset keeps")
    add("nomerge_50_rna", io(-20, 1200, -50, 1200, -100), "the same with segments the dRNA preset keeps")
    add("abandoned", io(-20, 10, -20, 200, -20), "a segment of 15: abandoned")
    add("scattered_close", io(-20, *no_sync(1), 100, -20), "the sixth scattered outlier ends the segment: nothing trailing")
    add("scattered_close_rna", io(-20, *no_sync(1, 1100), 100, -20), "the same, long enough for the dRNA preset")
    add("five_scattered", io(-20, 160, *[-1, 9] * 5, 100, -20), "five tolerated outliers, a clean edge")
    add("open_end", io(-20, 200, -20, 500), "the second segment is open at the end: dropped")
    add("open_end_rna", io(-20, 1200, -20, 1500), "the same for the dRNA preset")
    add("only_open", io(-20, 2000), "nothing closes")
    add("chain_of_merges", io(-30, 200, -10, 200, -49, 200, -6, 200, -50, 200, -20), "four merged, a fifth apart")
    # ---- chunk counts: 1 / 2 / 63 / 64 chunks and the lengths where the count changes
    for n in CHUNK_NQ:
        add("rich_%d" % n, rich(n, n), "%d chunks" % jnn_chunk_lanes(n))
    for n, seed in ((700, 1), (2048, 2), (2049, 3), (5000, 4), (5000, 5), (12000, 6), (40000, 7), (40000, 8), (39999, 9)):
        add("rich_%d_seed%d" % (n, seed), rich(n, seed), "a mix of everything")
    add("rich_rna_40000", rich(40000, 10, window=1000), "the same around the dRNA preset's window")
    add("rich_rna_16384", rich(16384, 11, window=1000), "the same around the dRNA preset's window")
    # ---- the end of chunk 0 (sample 255 / 256 of 2048) against the first sync sample
    for what, lead in SYNC_LEAD.items():
        add("sync_" + what, sync_read(lead, SYNC_WANT[what][1]), "the streak behind the first segment: " + what)
    add("span_chunks", io(-100, 800, -20, 300, pad_to=2048), "a segment over chunks 0 .. 3: lanes 1 and 2 run nothing")
    add("span_chunks_rna", io(-100, 3000, -20, 1300, pad_to=8000), "the same for the dRNA preset")
    add("weak_first_lane2", io(-600, 60, -10, 200, -20, 300, pad_to=2048), "the first candidate is weak and lies in lane 2")
    add("weak_behind_candidate", io(-100, 140, -270, 60, -30, 200, -20, 300, pad_to=2048),
        "a weak first candidate (145), then lane 1's first candidate is weak (65): dropped")
    add("weak_behind_strong", io(-100, 200, -300, 60, -30, 200, -20, 300, pad_to=2048), "the same behind a strong first")
    add("merge_across_empty", io(-100, 300, -6, 700, -49, 300, -50, 200, pad_to=2048),
        "merges at 6 and at 49 with whole chunks of one segment between")
    add("lanes_49_50", io(-30, 200, -49, 200, -50, 200, -49, 200, -50, 200, -49, 200, -50, 200, pad_to=2048),
        "gaps of 49 and 50 over the chunk ends")
    # ---- no sync point: a lane runs on through its neighbours' chunks and stages more than its slots hold
    add("no_sync_16384", io(-300, *no_sync(30), -100, 300, -200, 200, pad_to=16384), "30 strong segments in lane 1: capL is 4")
    add("no_sync_40000", io(-700, *no_sync(40), -100, 300, -200, 200, pad_to=40000), "40 in one lane: capL 9 (wave), 6 (long)")
    add("no_sync_all_5000", io(*no_sync(31)), "no sync sample in the whole read: lane 0 does everything")
    # ---- two merge rounds on the long path
    add("rounds_merge_49", rounds_read(49, ROUNDS_FIRST[0]), "merged across the rounds at seg_dist - 1")
    add("rounds_nomerge_50", rounds_read(50, ROUNDS_FIRST[1]), "not merged across the rounds at seg_dist")
    add("rounds_flush", io(*([250, -150] * 70), pad_to=40000), "nothing kept in the second round: the flush ends the last")
    add("rounds_weak_first", io(*([20, -100] * 280), -500, 60, -100, 300, -60, 200, pad_to=40000),
        "the first candidate is weak and lies in the second round")
    add("rounds_weak_dropped", io(-100, 200, -33500, 60, -100, 300, -60, 200, pad_to=40000),
        "a weak first-of-chunk in the second round behind a candidate of the first: dropped")
    # ---- own parameters: one step either side of every term of the launch rule, on the same reads
    for pname, p in RULE_PARAMS.items():
        e, w = max(p.error, 0), p.window
        add("%s/rich_2048" % pname, rich(2048, 21, e, w), "", p)
        add("%s/rich_5000" % pname, rich(5000, 22, e, w), "", p)
        add("%s/rich_16384" % pname, rich(16384, 23, e, w), "", p)
        add("%s/io" % pname, io(-20, w + 50, -(e + 1), w - e - 1, -(e + 1), w - e, -49, w, -50, w, *[-1, 3] * (e + 2), w, -(e + 1),
                                pad_to=4096), "streaks of error + 1, c == window - 1 / window, gaps of 49 / 50", p)
    for k, s in enumerate((30, 31, 32, 33)):
        add("error31/streak_%d" % s, io(-40, 226 - k, -s, 300, -32, 200, pad_to=2048),
            "a streak of %d from sample %d: over the end of chunk 0" % (s, 266 - k), RULE_PARAMS["error31"])
    add("error0/alternating", io(*[1, -1] * 600, 300, -1, 200, -1, 127, -1, 128, -1), "every outlier closes", RULE_PARAMS["error0"])
    # ---- the err-- correction (error >= corrector: once c has caught up with w it fires on every in-range sample)
    pc = fixed(corrector=4, error=4, window=20, seg_dist=1)
    add("correction/once", io(30, -4, 8, -1, 8, -1, 8, -1, 8, -1, 8, -1, 8, -30, 40, -20),
        "opens at 0; the fourth error makes c == w", pc)
    add("correction/twice", io(30, -4, *[8, -1] * 12, -30, 40, -20), "c == w on every in-range sample: errors never add up", pc)
    add("correction/later", io(-3, 2, -9, 30, -6, *[8, -1] * 12, -30, 40, -20),
        "two in-range samples in front of the segment: it takes corrector + 2 errors", fixed(corrector=4, error=6, window=20, seg_dist=1))
    add("correction/c>w", io(30, -5, *[3, -1] * 12, -30, 40, -20),
        "c == w + 1: c % w != 0 for ever, the budget runs out", fixed(corrector=4, error=5, window=20, seg_dist=1))
    add("correction/below_window", io(10, -4, *[3, -1] * 12, -30, 40, -20), "c == w below the window: no correction",
        fixed(corrector=4, error=4, window=40, seg_dist=10))
    add("correction/std", io(30, -4, *[8, -1] * 12, -30, 40, -20), "the same with thresholds from the read",
        pc._replace(std_scale=0.75))
    # ---- thresholds against the clamp
    hi = sig((50, 100), (300, 5000), (20, 1200), (50, 100))
    lo = sig((50, 600), (300, -7), (20, 0), (50, 600))
    for name, raw, top, bot in (("top_1200", hi, 1200.0, 1000.0), ("top_1200.5", hi, 1200.5, 1000.0), ("top_1201", hi, 1201.0, 1000.0),
                                ("top_5000", hi, 5000.0, 1199.5), ("bot_0", lo, 100.0, 0.0), ("bot_-0.5", lo, 100.0, -0.5),
                                ("bot_-1", lo, 100.0, -1.0), ("bot_-7", lo, 0.5, -7.0), ("top_0", lo, 0.0, -5.0), ("top_-3", lo, -3.0, -9.0),
                                ("bot_1200", hi, 1300.0, 1200.0), ("bot_1250", hi, 1300.0, 1250.0),
                                ("top_nan", hi, float("nan"), 1000.0), ("bot_nan", lo, 100.0, float("nan")),
                                ("top_inf", hi, float("inf"), 1000.0), ("bot_-inf", lo, 100.0, float("-inf")),
                                ("top<bot", hi, 1000.0, 1300.0)):
        add("thr/" + name, raw, "", fixed(top=top, bot=bot))
    eq = sig((20, 700), (200, 499), (50, 500), (200, 499), (30, 700), (200, 501), (30, 700))
    add("thr/sample==top", eq, "a stretch AT top is out of range", fixed(top=500.0, bot=400.0))
    add("thr/sample==bot", eq, "a stretch AT bot is out of range", fixed(top=600.0, bot=500.0))
    add("thr/fraction", eq, "499 < 499.5 < 500", fixed(top=499.5, bot=400.0))
    names = [k.name for k in c]
    assert len(set(names)) == len(names)
    return c


def preset_cases(cat):
    return [k for k in cat if k.params is None]


def pa_sig(*parts):
    return np.concatenate([np.full(int(n), v, dtype=F) for n, v in parts])


def pa_cases():
    """pA arrays straight into jnn_pa: what raw reads cannot hold"""
    nan, inf = float("nan"), float("inf")
    I, O = 100.0, 150.0
    p = fixed(top=120.0, bot=80.0)
    out = []

    def add(name, pa, params, note=""):
        out.append(PaCase(name, np.ascontiguousarray(pa, dtype=F), params, note))
    add("plain", pa_sig((20, O), (200, I), (49, O), (200, I), (50, O), (200, I), (30, O)), p, "merge at 49, none at 50")
    x = pa_sig((20, O), (400, I), (100, O)); x[30:400:80] = nan
    add("nan_errors", x, p, "NaN samples are tolerated errors")
    add("all_nan", pa_sig((500, nan)), p, "nothing in range")
    x = pa_sig((20, O), (400, I), (100, O)); x[200] = nan
    add("nan_inside_std", x, p._replace(std_scale=0.75), "a NaN sample with std_scale > 0: thresholds NaN, no segment")
    add("inf", pa_sig((10, O), (300, I), (3, inf), (300, I), (100, -inf), (200, I), (10, O)), p, "+-inf are clamped: out of range")
    add("inf_in_range", pa_sig((10, 0.0), (300, inf), (20, 0.0)), fixed(top=1200.5, bot=1000.0), "inf is clamped to 1200: in range")
    add("neg_zero_bot_neg_zero", pa_sig((10, O), (300, -0.0), (20, O)), fixed(top=50.0, bot=-0.0), "-0.0 > -0.0 is false")
    add("neg_zero_bot_below", pa_sig((10, O), (300, -0.0), (20, O)), fixed(top=50.0, bot=-0.5), "-0.0 is in range, so is -3 (clamped)")
    add("level==top", pa_sig((10, O), (300, 100.25), (20, O), (300, 100.125), (20, O)), fixed(top=100.25, bot=80.0), "AT the float top")
    add("level==bot", pa_sig((10, O), (300, 80.5), (20, O), (300, 80.625), (20, O)), fixed(top=120.0, bot=80.5), "AT the float bot")
    add("std", pa_sig((30, 140.5), (400, 100.25), (30, 60.0), (300, 100.25), (40, 140.5)), p._replace(std_scale=0.75), "thresholds from floats")
    add("n1", pa_sig((1, I)), p, "one sample in range, open at the end")
    pc = fixed(corrector=4, error=4, window=20, seg_dist=1, top=120.0, bot=80.0)
    add("correction_once", pa_sig((30, I), (4, O), *[(8, I), (1, O)] * 6, (30, O), (40, I), (20, O)), pc)
    add("correction_twice", pa_sig((30, I), (4, O), *[(8, I), (1, nan)] * 12, (30, O), (40, I), (20, O)), pc)
    add("correction_c>w", pa_sig((30, I), (5, O), *[(3, I), (1, O)] * 12, (30, O), (40, I), (20, O)), pc._replace(error=5))
    return out


def catalogue_sha256() -> str:
    h = hashlib.sha256()
    for k in catalogue():
        h.update(k.name.encode() + b"\0" + k.raw.tobytes() + repr(k.params).encode())
    for k in pa_cases():
        h.update(k.name.encode() + b"\0" + k.pa.tobytes() + repr(k.params).encode())
    return h.hexdigest()


def case_runs(k):
    """the (label, parameters) a case is run with: both presets, or its own"""
    return [("%s/rna%d" % (k.name, rna), PRESET[rna]) for rna in (0, 1)] if k.params is None else [(k.name, k.params)]


def tag_table(cat=None):
    """-> {tag: [labels of the runs it fires on]} over the catalogue and ("pa " + tag) over the pA arrays"""
    table = {}
    for k in cat or catalogue():
        s = clamp_raw(k.raw)
        for label, p in case_runs(k):
            _, tags, info = jnn_core_model(s, p)
            for t in tags | geometry_tags(info, p):
                table.setdefault(t, []).append(label)
    for k in pa_cases():
        s = clamp_pa(k.pa)
        _, tags, _ = jnn_core_model(s, k.params)
        with np.errstate(invalid="ignore"):
            if np.isnan(k.pa).any():
                tags.add(J_NAN_SAMPLE)
            if np.isinf(k.pa).any():
                tags.add(J_INF_SAMPLE)
            if ((k.pa == 0) & np.signbit(k.pa)).any():
                tags.add(J_NEG_ZERO)
        for t in tags:
            table.setdefault("pa " + t, []).append(k.name)
    return table


if __name__ == "__main__":
    for name, v in run_searches().items():
        print("%s = %r" % (name, v))
    cat = catalogue()
    table = tag_table(cat)
    for t in J_TAGS + G_TAGS + tuple("pa " + t for t in J_TAGS_PA):
        names = table.get(t, [])
        print("%-60s %3d  %s" % (t, len(names), ", ".join(names[:3])))
    print("%d reads, %d samples, longest %d" % (len(cat), sum(k.raw.size for k in cat), max(k.raw.size for k in cat)))
    print(catalogue_sha256())
