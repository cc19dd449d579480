"""The catalogue of hand-made reads for `prefix` and a plain branch model of its two finders.

find_adaptor is jnnv2 (the reference's src/jnn.c:99-188): a run finder over the 2000-sample rolling means of the clamped
raw signal.  find_polya (src/jnn.c:352-374) is the error-tolerant jnn_core automaton (src/jnn.c:190-278) on clamped pA,
cut down to its first merged segment.  `jnnv2_model` and `polya_model` restate both as literal loops and return, besides
the answer, the SET OF BRANCHES that fired (the A_* / P_* tags below).  test_prefix_cases_cpu.py proves the models equal
to the oracle on every read and requires every tag to fire somewhere: that is what keeps this catalogue from going soft.

The reads are built from plateaus and dips (`sig`), with an optional seeded noise term.  Where a branch needs tuning --
a run of exactly one window, a gap between two runs of exactly seg_dist - 1 / seg_dist, a rolling mean that EQUALS the
threshold, run edges at chosen window indices modulo the wave kernel's 1024-window tile -- a small search function
(`search_*`) finds the parameter, and what it found is committed next to it as a constant: building the catalogue runs
no search.  `python tests/prefix_cases.py` reruns the searches and prints the constants and the tag -> read table.

Numbers: rolling totals are integers below 2^24, so forming them as integers is what the reference's float running
total gives; the two sequential float sums (meanf, stdvf) are np.cumsum in float32, which adds strictly in order.
"""
import hashlib
from typing import NamedTuple

import numpy as np

F = np.float32
WINDOW = 2000

# ---- branch tags: jnnv2
A_TOO_SHORT = "a:too_short"            # n <= window: (-1, -1)
A_M1 = "a:m==1"                        # a single rolling mean
A_OPEN_AT_0 = "a:open_at_window_0"
A_EXTEND = "a:extend"
A_CLOSE_NEW = "a:close_new"
A_CLOSE_MERGE = "a:close_merge"
A_ONE_SAMPLE = "a:one_sample_run"      # closed with end == 0: the run was never extended
A_ONE_SAMPLE_MERGE = "a:one_sample_run_merged"   # ... and merged: the previous run's end becomes 0
A_EQ_OUTSIDE = "a:t==bot_outside_run"
A_EQ_INSIDE = "a:t==bot_inside_run"
A_SKIP_LO = "a:skip_lt_lo"
A_SKIP_HI = "a:skip_gt_hi"
A_ANS_RUN0 = "a:answer_run_0"
A_ANS_LATER = "a:answer_run_ge_1"
A_NONE = "a:no_run_qualifies"
A_OPEN_END = "a:open_at_end_dropped"
A_BOT_NEG = "a:bot<0"
A_GAP_DIST_M1 = "a:merge_at_seg_dist-1"
A_GAP_DIST = "a:no_merge_at_seg_dist"
A_LEN_EQ_LO = "a:len==lo"
A_LEN_EQ_LO_M1 = "a:len==lo-1"
A_LEN_EQ_HI = "a:len==hi"
A_LEN_EQ_HI_P1 = "a:len==hi+1"
A_TAGS_SUBTOOL = (A_TOO_SHORT, A_M1, A_OPEN_AT_0, A_EXTEND, A_CLOSE_NEW, A_CLOSE_MERGE, A_ONE_SAMPLE, A_EQ_OUTSIDE,
                  A_EQ_INSIDE, A_SKIP_LO, A_SKIP_HI, A_ANS_RUN0, A_ANS_LATER, A_NONE, A_OPEN_END, A_BOT_NEG,
                  A_GAP_DIST_M1, A_GAP_DIST)
A_TAGS_SHIM = (A_LEN_EQ_LO, A_LEN_EQ_LO_M1, A_LEN_EQ_HI, A_LEN_EQ_HI_P1, A_GAP_DIST_M1, A_GAP_DIST)

# ---- branch tags: the polyA automaton
P_OPEN_AT_0 = "p:open_at_0"
P_KEPT = "p:closed_kept"
P_KEPT_AT_WINDOW = "p:closed_kept_c==window"
P_REJECT = "p:closed_rejected"
P_REJECT_AT_WINDOW_M1 = "p:closed_rejected_c==window-1"
P_MERGED_FIRST = "p:merged_into_first"
P_MERGE_AT_DIST_M1 = "p:merge_at_seg_dist-1"
P_SECOND = "p:second_segment"
P_SECOND_AT_DIST = "p:second_segment_at_seg_dist"
P_OPEN_END = "p:open_at_end"
P_BUDGET = "p:error_budget_exhausted_scattered"   # the (error + 1)-th error closes, the earlier ones not all trailing
P_TRAIL = "p:trailing_errors_cut"                 # end = i - run_err with run_err > 0
P_NO_TRAIL = "p:no_trailing_errors"
P_EQ_TOP = "p:sample==top"
P_EQ_BOT = "p:sample==bot"
P_NAN = "p:nan_sample"
P_NONE = "p:nothing_found"
P_TAGS = (P_OPEN_AT_0, P_KEPT, P_KEPT_AT_WINDOW, P_REJECT, P_REJECT_AT_WINDOW_M1, P_MERGED_FIRST, P_MERGE_AT_DIST_M1,
          P_SECOND, P_SECOND_AT_DIST, P_OPEN_END, P_BUDGET, P_TRAIL, P_NO_TRAIL, P_EQ_TOP, P_EQ_BOT, P_NAN, P_NONE)
# what must be reached through the subtool (raw reads): equality with a float threshold and NaN samples need pA arrays
P_TAGS_SUBTOOL = (P_OPEN_AT_0, P_KEPT, P_KEPT_AT_WINDOW, P_REJECT, P_REJECT_AT_WINDOW_M1, P_MERGED_FIRST,
                  P_MERGE_AT_DIST_M1, P_SECOND, P_SECOND_AT_DIST, P_OPEN_END, P_BUDGET, P_TRAIL, P_NO_TRAIL, P_NONE)


class AdaptP(NamedTuple):          # jnnv2_param_t
    std_scale: float
    seg_dist: int
    hi: int
    lo: int


def adaptor_params(pore: int) -> AdaptP:
    return AdaptP(0.7, 1500, 200000, 500) if pore == 2 else AdaptP(0.5, 1500, 200000, 2000)


def seqsum(x) -> np.float32:
    """float sum = 0; for (...) sum += x[i];"""
    x = np.asarray(x, dtype=F)
    return F(0) if x.size == 0 else np.cumsum(x, dtype=F)[-1]


def meanf(x):
    return seqsum(x) / F(len(x))


def stdvf(x):
    x = np.asarray(x, dtype=F)
    d = x - meanf(x)
    return np.sqrt(seqsum(d * d) / F(len(x)))


def rolling_means(raw):
    c = np.clip(np.asarray(raw, dtype=np.int64), 0, 1200)
    cs = np.concatenate([[0], np.cumsum(c)])
    m = c.size - WINDOW
    return (cs[WINDOW:WINDOW + m] - cs[:m]).astype(F) / F(WINDOW)


def adaptor_bot(raw, std_scale):
    t = rolling_means(raw)
    with np.errstate(all="ignore"):
        return t, meanf(t) - stdvf(t) * F(std_scale)


def jnnv2_model(raw, p: AdaptP):
    """-> ((x, y), tags, runs): jnnv2 with window 2000; runs = the (start, end) list before the length filter"""
    tags = set()
    n = len(raw)
    if not n > WINDOW:
        return (-1, -1), {A_TOO_SHORT}, []
    t, bot = adaptor_bot(raw, p.std_scale)
    if t.size == 1:
        tags.add(A_M1)
    if bot < 0:
        tags.add(A_BOT_NEG)
    lt = (t < bot).tolist()
    gt = (t > bot).tolist()
    begin, start, end = False, 0, 0
    segs = []
    for j in range(t.size):
        if lt[j] and not begin:
            start, begin = j, True
            if j == 0:
                tags.add(A_OPEN_AT_0)
        elif lt[j]:
            end = j
            tags.add(A_EXTEND)
        elif gt[j] and begin:
            if end == 0:
                tags.add(A_ONE_SAMPLE)
            if segs and start - segs[-1][1] < p.seg_dist:
                if start - segs[-1][1] == p.seg_dist - 1:
                    tags.add(A_GAP_DIST_M1)
                if end == 0:
                    tags.add(A_ONE_SAMPLE_MERGE)
                segs[-1][1] = end
                tags.add(A_CLOSE_MERGE)
            else:
                if segs and start - segs[-1][1] == p.seg_dist:
                    tags.add(A_GAP_DIST)
                segs.append([start, end])
                tags.add(A_CLOSE_NEW)
            start, end, begin = 0, 0, False
        elif not lt[j] and not gt[j]:
            tags.add(A_EQ_INSIDE if begin else A_EQ_OUTSIDE)
    if begin:
        tags.add(A_OPEN_END)
    ans = (0, 0)
    for i, (a, b) in enumerate(segs):
        if b - a > p.hi:
            tags.add(A_SKIP_HI)
            if b - a == p.hi + 1:
                tags.add(A_LEN_EQ_HI_P1)
            continue
        if b - a < p.lo:
            tags.add(A_SKIP_LO)
            if b - a == p.lo - 1:
                tags.add(A_LEN_EQ_LO_M1)
            continue
        if b - a == p.lo:
            tags.add(A_LEN_EQ_LO)
        if b - a == p.hi:
            tags.add(A_LEN_EQ_HI)
        ans = (a + WINDOW // 2 - 1, b + WINDOW // 2 - 1)
        tags.add(A_ANS_RUN0 if i == 0 else A_ANS_LATER)
        break
    else:
        tags.add(A_NONE)
    return ans, tags, [tuple(s) for s in segs]


POLYA = dict(corrector=50, seg_dist=200, window=250, stall_len=1.0, error=30)


def polya_model(pa, top, bot):
    """-> ((x, y), tags): find_polya = segs[0] of jnn_core on rm_outlierf(pa) with the polyA preset, (-1, -1) if none"""
    tags = set()
    top, bot = F(top), F(bot)
    with np.errstate(invalid="ignore"):
        sig = np.asarray(pa, dtype=F).copy()
        sig[sig > 1200] = 1200
        sig[sig < 0] = 0
        inr = ((sig < top) & (sig > bot)).tolist()
        if np.isnan(sig).any():
            tags.add(P_NAN)
        if (sig == top).any():
            tags.add(P_EQ_TOP)
        if (sig == bot).any():
            tags.add(P_EQ_BOT)
    prev, err, prev_err, c, w = False, 0, 0, 0, POLYA["corrector"]
    window, error, seg_dist, stall = POLYA["window"], POLYA["error"], POLYA["seg_dist"], POLYA["stall_len"]
    start = 0
    segs = []
    for i in range(len(inr)):
        if inr[i]:
            if not prev:
                start, prev = i, True
                if i == 0:
                    tags.add(P_OPEN_AT_0)
            c += 1
            w += 1
            prev_err = 0
            if c >= window and c >= w and c % w == 0:
                err -= 1
        elif prev and err < error:
            c += 1
            err += 1
            prev_err += 1
            if c >= window and c >= w and c % w == 0:
                err -= 1
        elif prev and (c >= window or (not segs and c >= window * stall)):
            end = i - prev_err
            prev = False
            tags.add(P_KEPT)
            if c == window:
                tags.add(P_KEPT_AT_WINDOW)
            tags.add(P_TRAIL if prev_err > 0 else P_NO_TRAIL)
            if prev_err < error:
                tags.add(P_BUDGET)
            if segs and start - segs[-1][1] < seg_dist:
                if len(segs) == 1:
                    tags.add(P_MERGED_FIRST)
                    if start - segs[-1][1] == seg_dist - 1:
                        tags.add(P_MERGE_AT_DIST_M1)
                segs[-1][1] = end
            else:
                if len(segs) == 1:
                    tags.add(P_SECOND)
                    if start - segs[-1][1] == seg_dist:
                        tags.add(P_SECOND_AT_DIST)
                segs.append([start, end])
            c = err = prev_err = 0
        elif prev:
            tags.add(P_REJECT)
            if c == window - 1:
                tags.add(P_REJECT_AT_WINDOW_M1)
            prev = False
            c = err = prev_err = 0
    if prev:
        tags.add(P_OPEN_END)
    if not segs:
        tags.add(P_NONE)
        return (-1, -1), tags
    return (segs[0][0], segs[0][1]), tags


def to_pa(raw, dig, off, rng):
    """signal_in_picoamps: float unit = range / digitisation; pA = (raw + (float)offset) * unit"""
    with np.errstate(all="ignore"):
        unit = F(np.float64(rng) / np.float64(dig))
        return (np.asarray(raw, dtype=F) + F(off)) * unit


def prefix_model(raw, dig, off, rng, rna, pore):
    """-> (adaptor (x, y), polyA (x, y) relative to the read, tags of both stages)"""
    (ax, ay), tags, _ = jnnv2_model(raw, adaptor_params(pore))
    if ay <= 0 or not rna:
        return (ax, ay), (-1, -1), tags
    pa = to_pa(raw, dig, off, rng)
    with np.errstate(all="ignore"):
        m_a = meanf(pa[ax:ay])
        mid = m_a + F(30)
        (px, py), ptags = polya_model(pa[ay:], mid + F(20), mid - F(20))
    return (ax, ay), ((px + ay, py + ay) if py > 0 else (-1, -1)), tags | ptags


# ---------------------------------------------------------------- building blocks
DIG, OFF, RNG = 8192.0, 10.0, 1402.882324      # unit 0.17125: 30 pA are 175 raw codes
BODY, ADAPT, POLY = 900, 500, 675              # raw levels: body, adaptor dip, polyA (adaptor + 30 pA)


class Case(NamedTuple):
    name: str
    raw: np.ndarray
    dig: float
    off: float
    rng: float
    rna: int
    note: str


def sig(*parts, noise=0, seed=0):
    """plateaus (length, level) in a row; noise: uniform integers in [-noise, noise] from a seeded generator"""
    x = np.concatenate([np.full(int(n), int(v), dtype=np.int64) for n, v in parts])
    if noise:
        x = x + np.random.RandomState(seed).randint(-noise, noise + 1, size=x.size)
    return np.clip(x, -32768, 32767).astype(np.int16)


def case(name, raw, note, rna=1, dig=DIG, off=OFF, rng=RNG):
    return Case(name, raw, float(dig), float(off), float(rng), rna, note)


# ---------------------------------------------------------------- searched constants
GAP_TAIL = {0: 8000, 2: 40000}   # (std_scale 0.7 needs a higher threshold for runs that close together: more body)


def two_dips(gap, pore):
    return sig((3000, BODY), (4500, ADAPT), (gap, BODY), (4500, ADAPT), (GAP_TAIL[pore], BODY))


def search_gap(pore, want):
    """the stretch between two dips for which the second run starts exactly `want` windows behind the first's end"""
    p = adaptor_params(pore)
    for gap in range(200, 4000):
        t, bot = adaptor_bot(two_dips(gap, pore), p.std_scale)
        below = np.flatnonzero(t < bot)
        cut = np.flatnonzero(np.diff(below) > 1)
        if cut.size == 1 and below[cut[0] + 1] - below[cut[0]] == want:
            return gap
    return None


#: samples between the dips of `two_dips`, per pore: (run gap seg_dist - 1 -> merged, run gap seg_dist -> two runs)
GAPS = {0: (707, 708), 2: (1843, 1844)}


def vee(tail, after=False, level=700):
    """a real adaptor dip and a dip of exactly one window at `level` (its rolling mean has a single lowest index), in
    front of it or 600 samples behind it; the length of the body at the end moves the threshold"""
    v, a = [(WINDOW, level)], [(5000, ADAPT)]
    mid = [(600, BODY)] if after else [(5000, BODY)]
    return sig((4000, BODY), *((a + mid + v) if after else (v + mid + a)), (tail, BODY))


def search_one_sample(pore, after):
    """tail for which exactly one rolling mean of the one-window dip lies below the threshold: a run that opens and is
    never extended (it closes with end == 0)"""
    p = adaptor_params(pore)
    for tail in range(2500, 40000, 3):
        t, bot = adaptor_bot(vee(tail, after), p.std_scale)
        lo = 4000 + (5600 if after else 0)
        if np.count_nonzero(t[lo - 300:lo + 300] < bot) == 1:
            return tail
    return None


#: tail of `vee`, per pore: (one-window dip in front of the adaptor, behind it)
ONE_SAMPLE = {0: (5380, 9997), 2: (10327, 15082)}


def shallow(bump_len, bump_level):
    """a dip two codes deep: its slopes are rolling means 0.001 apart, so the float threshold can land ON one"""
    return sig((4000, 500), (5000, 498), (5000, 500), (bump_len, bump_level), (3000, 500))


def search_eq(pore, limit=4000):
    """bump for which one rolling mean on the falling slope (outside a run) and one on the rising slope (inside a
    run) EQUAL the threshold"""
    p = adaptor_params(pore)
    k = 0
    for blen in range(2500, 4000, 7):
        for level in (501, 502, 503, 504, 499, 497):
            k += 1
            if k > limit:
                return None
            t, bot = adaptor_bot(shallow(blen, level), p.std_scale)
            if np.count_nonzero(t == bot) < 2:
                continue
            _, tags, _ = jnnv2_model(shallow(blen, level), p)
            if A_EQ_INSIDE in tags and A_EQ_OUTSIDE in tags:
                return blen, level
    return None


#: (bump length, bump level) of `shallow`, per pore
EQ_SLOPES = {0: (2528, 499), 2: (2549, 497)}


def geometry(leader, dip):
    return sig((leader, BODY), (dip, ADAPT), (9000, BODY), noise=3, seed=5)


#: the run's first / last window index modulo the wave kernel's tile of 1024 windows (read k: start R[k], end R[k + 3])
GEOMETRY_RESIDUES = (0, 1, 15, 16, 1023, 1024, 1025)


def search_geometry(pore, r_start, r_end):
    """leader and dip lengths that put the run's first window at r_start and its last at r_end (mod 1024)"""
    p = adaptor_params(pore)
    leader, dip = 3000 + r_start, 5200
    for _ in range(40):
        _, _, runs = jnnv2_model(geometry(leader, dip), p)
        if len(runs) != 1:
            return None
        a, b = runs[0]
        da, db = (r_start - a) % 1024, (r_end - b) % 1024
        if da == 0 and db == 0:
            return leader, dip
        if da:
            leader += da if da < 512 else da - 1024
            if leader < 2500:
                leader += 1024
        else:
            dip += db if db < 512 else db - 1024
            if dip < 4200:
                dip += 1024
    return None


#: (leader, dip) of `geometry`, per pore, one per entry of GEOMETRY_RESIDUES
GEOMETRY = {0: [(2912, 5409), (2915, 5386), (2932, 5367), (2933, 5367), (4002, 5259), (4003, 5259), (4002, 5276)],
            2: [(2842, 4525), (2682, 5852), (2699, 5834), (2700, 5834), (3773, 5717), (3775, 5716), (3774, 5733)]}

def tile_edge(gap):
    """an adaptor and two polyA stretches; `gap` places the end of the first stretch relative to the tiles of 1024 samples
    in which the wave kernel walks the tail (they start at adapt_y rounded down to 8 samples)"""
    return sig((3000, BODY), (5000, ADAPT), (gap, BODY), (600, POLY), (300, BODY), (600, POLY), (6000, BODY))


#: the first stretch ends k samples in front of a tile boundary of the tail: its 31 errors (the last one closes the segment)
#: lie in the next tile (0), straddle the boundary (1, 15, 16, 29), end on the tile's last sample (31) or first (30)
TILE_EDGE_K = (0, 1, 15, 16, 29, 30, 31, 32)


def search_tile_edge(pore, k):
    gap = 1500
    for _ in range(20):
        (ax, ay), _, _ = jnnv2_model(tile_edge(gap), adaptor_params(pore))
        end = 8000 + gap + 600
        d = (-k - (end - (ay & ~7))) % 1024
        if d == 0:
            return gap
        gap += d
        if gap > 3000:
            gap -= 1024
    return None


#: `gap` of `tile_edge`, per pore, one per entry of TILE_EDGE_K
TILE_EDGE = {0: [2360, 2359, 2337, 2336, 2323, 2322, 2321, 2320], 2: [2192, 2191, 2177, 2176, 2163, 2162, 2161, 2160]}

#: jnnv2 shim: the run of `shim_dip()` has this length (last - first window) at std_scale 0.5 / 0.7, and the two runs of
#: `two_dips(1200, 0)` lie this far apart
SHIM_RUN_LEN = {0.5: 6382, 0.7: 6078}
SHIM_RUN_GAP = {0.5: 1928, 0.7: 2270}


def shim_dip():
    return sig((8000, BODY), (6000, ADAPT), (16000, BODY), noise=2, seed=9)


def run_searches():
    out = {"GAPS": {}, "ONE_SAMPLE": {}, "EQ_SLOPES": {}, "GEOMETRY": {}, "SHIM_RUN_LEN": {}, "SHIM_RUN_GAP": {}}
    R = GEOMETRY_RESIDUES
    for pore in (0, 2):
        out["GAPS"][pore] = (search_gap(pore, 1499), search_gap(pore, 1500))
        out["ONE_SAMPLE"][pore] = (search_one_sample(pore, False), search_one_sample(pore, True))
        out["EQ_SLOPES"][pore] = search_eq(pore)
        out["GEOMETRY"][pore] = [search_geometry(pore, r, R[(k + 3) % len(R)]) for k, r in enumerate(R)]
        p = adaptor_params(pore)
        runs = jnnv2_model(shim_dip(), p)[2]
        out.setdefault("TILE_EDGE", {})[pore] = [search_tile_edge(pore, k) for k in TILE_EDGE_K]
        out["SHIM_RUN_LEN"][p.std_scale] = runs[0][1] - runs[0][0]
        runs = jnnv2_model(two_dips(1200, 0), p._replace(seg_dist=1))[2]
        out["SHIM_RUN_GAP"][p.std_scale] = runs[1][0] - runs[0][1]
    return out


# ---------------------------------------------------------------- the catalogue
def rna_read(*tail, noise=0, seed=0, body=6000):
    """leader, adaptor dip, 1500 samples of body (out of the polyA band), the given tail, body"""
    return sig((3000, BODY), (5000, ADAPT), (1500, BODY), *tail, (body, BODY), noise=noise, seed=seed)


def bursts(n, every):
    """n samples at the polyA level, every `every`-th one at the body level (a tolerated error each)"""
    x = np.full(n, POLY, dtype=np.int16)
    x[every - 1::every] = BODY
    return x


def catalogue():
    """-> list of Case, deterministic"""
    c = []
    rs = np.random.RandomState(20250)
    # ---- lengths around the window, constant reads (sd = 0, bot = mean: every rolling mean EQUALS the threshold)
    c.append(case("short_1999", sig((1999, 500), noise=5, seed=1), "n < window: (-1, -1)"))
    c.append(case("short_2000", sig((2000, 500), noise=5, seed=2), "n == window: (-1, -1)"))
    c.append(case("one_mean_2001", sig((2001, 500), noise=5, seed=3), "a single rolling mean: t == bot"))
    c.append(case("two_means_2002", sig((2001, 500), (1, 100)), "two rolling means, the second lower"))
    c.append(case("const_500x3000", sig((3000, 500)), "constant, float sums exact"))
    c.append(case("const_333x100000", sig((100000, 333)), "constant, the float sum of 98 000 means is not exact"))
    c.append(case("const_below_clamp", sig((5000, -50)), "constant below 0: clamped to 0"))
    c.append(case("const_above_clamp", sig((5000, 2000)), "constant above 1200: clamped"))
    c.append(case("bot_negative", sig((9000, -20), (1000, 1200), (9000, 0)), "mean 60, sd large: bot < 0, nothing below"))
    # ---- the run finder
    c.append(case("typical", sig((3000, BODY), (5000, ADAPT), (3000, POLY), (15000, BODY), noise=40, seed=4),
                  "leader, adaptor, polyA straight behind it, body"))
    c.append(case("typical_flat", sig((3000, BODY), (5000, ADAPT), (3000, POLY), (15000, BODY)), "the same without noise"))
    c.append(case("merge_pair", sig((3000, BODY), (4000, ADAPT), (2600, BODY), (4000, ADAPT), (9000, BODY), noise=10, seed=5),
                  "two dips whose runs lie less than seg_dist apart: one merged run"))
    for pore in (0, 2):
        for k, what in enumerate(("seg_dist-1_merged", "seg_dist_two_runs")):
            c.append(case("gap_%s_pore%d" % (what, pore), two_dips(GAPS[pore][k], pore),
                          "second run starts exactly %d windows behind the first's end with pore %d" % (1499 + k, pore)))
    c.append(case("short_then_long", sig((3000, BODY), (2600, ADAPT), (6000, BODY), (6000, ADAPT), (9000, BODY), noise=10, seed=6),
                  "first run under 2000 windows but over 500: the answer differs between the pores"))
    c.append(case("tiny_then_long", sig((3000, BODY), (1700, ADAPT), (6000, BODY), (6000, ADAPT), (9000, BODY), noise=10, seed=7),
                  "first run under 500 windows: skipped with either pore"))
    c.append(case("only_short", sig((5000, BODY), (1800, ADAPT), (9000, BODY)), "one run, too short: (0, 0)"))
    c.append(case("dip_at_start", sig((5000, ADAPT), (12000, BODY), noise=10, seed=8), "the run opens at window 0"))
    c.append(case("dip_at_end", sig((12000, BODY), (5000, ADAPT), noise=10, seed=9), "the only run is still open at the end"))
    c.append(case("dip_then_open_end", sig((3000, BODY), (5000, ADAPT), (8000, BODY), (4000, ADAPT)),
                  "a closed run, then one open at the end"))
    for pore in (0, 2):
        c.append(case("one_window_run_pore%d" % pore, vee(ONE_SAMPLE[pore][0]),
                      "with pore %d one rolling mean is below bot: run (start, 0), skipped; the adaptor follows" % pore))
        c.append(case("one_window_run_kills_pore%d" % pore, vee(ONE_SAMPLE[pore][1], True),
                      "with pore %d the one-window run is merged into the adaptor run, whose end becomes 0" % pore))
        c.append(case("threshold_on_slope_pore%d" % pore, shallow(*EQ_SLOPES[pore]),
                      "with pore %d a rolling mean equals bot on the way down and on the way up" % pore))
    c.append(case("spikes", sig((4000, BODY), (5000, ADAPT), (9000, BODY), noise=3, seed=10) +
                  (rs.rand(18000) < 0.002).astype(np.int16) * rs.randint(-30000, 30000, size=18000).astype(np.int16),
                  "isolated spikes of either sign on a dip read"))
    c.append(case("full_range_noise", rs.randint(-32768, 32768, size=30000).astype(np.int16), "white noise over all of int16"))
    c.append(case("noisy_edges", sig((6000, 700), (6000, 400), (8000, 700), noise=600, seed=11),
                  "noise wider than the slope: the below-threshold flag flickers at both run edges"))
    c.append(case("long_dip_then_adaptor", sig((20000, BODY), (230000, ADAPT), (100000, BODY), (6000, ADAPT), (104000, BODY),
                                               noise=20, seed=12),
                  "460 000 samples: a run over hi_thresh, then the qualifying one"))
    # ---- run edges on the wave kernel's tile boundaries
    for pore in (0, 2):
        for k, (leader, dip) in enumerate(GEOMETRY[pore]):
            R = GEOMETRY_RESIDUES
            c.append(case("edges_pore%d_%d_%d" % (pore, R[k], R[(k + 3) % len(R)]), geometry(leader, dip),
                          "with pore %d the run starts at window = %d and ends at %d (mod 1024)" % (pore, R[k], R[(k + 3) % len(R)])))
    # ---- the polyA stage through the subtool
    P, B = POLY, BODY
    c.append(case("pa_stretch_220", rna_read((220, P), (300, B), (600, P)), "220 in range + 30 errors: c == 250, kept"))
    c.append(case("pa_stretch_219", rna_read((219, P), (300, B), (600, P)), "c == 249: rejected, the later stretch is the answer"))
    c.append(case("pa_stretch_249", rna_read((249, P), (300, B), (600, P)), "kept"))
    c.append(case("pa_stretch_250", rna_read((250, P), (300, B), (600, P)), "kept"))
    c.append(case("pa_merge_199", rna_read((400, P), (199, B), (400, P), (300, B), (400, P)), "gap 199: merged; the third is a second segment"))
    c.append(case("pa_nomerge_200", rna_read((400, P), (200, B), (400, P)), "gap 200 == seg_dist: not merged"))
    c.append(case("pa_chain_of_merges", rna_read((300, P), (150, B), (300, P), (40, B), (300, P), (199, B), (300, P), (900, B), (300, P)),
                  "four stretches merged into the first segment, a fifth apart"))
    c.append(case("pa_open_tail", rna_read((400, P), (300, B), (700, P), body=0), "the second stretch is open at the end of the read"))
    c.append(case("pa_only_open", rna_read((900, P), body=0), "the only stretch is open at the end: nothing found"))
    x = rna_read((700, P))
    x[9500:10200] = bursts(700, 15)
    c.append(case("pa_scattered_errors", x, "an error every 15 samples: the 31st closes the segment, nothing trailing"))
    x = rna_read((1200, P))
    x[9500:10700] = bursts(1200, 41)
    c.append(case("pa_29_errors", x, "29 scattered errors are tolerated, the stretch ends on a clean edge"))
    c.append(case("pa_rejects_then_kept", rna_read((100, P), (60, B), (200, P), (60, B), (500, P)), "two short stretches rejected"))
    c.append(case("pa_noisy", rna_read((2500, P), noise=90, seed=13), "noise as wide as the polyA band"))
    c.append(case("pa_late", rna_read((30000, B), (800, P), noise=8, seed=14), "polyA 30 000 samples behind the adaptor: 30 tiles of nothing"))
    for pore in (0, 2):
        for k, gap in zip(TILE_EDGE_K, TILE_EDGE[pore]):
            c.append(case("pa_tile_edge_pore%d_%d" % (pore, k), tile_edge(gap),
                          "with pore %d the first polyA stretch ends %d samples in front of a tile boundary of the tail" % (pore, k)))
    # ---- hostile scalings of a read whose adaptor is found
    base = rna_read((400, P), (199, B), (400, P), (300, B), (400, P), noise=6, seed=15)
    for name, kw, note in (("dig_zero", dict(dig=0.0), "unit = inf"), ("range_zero", dict(rng=0.0), "every pA is 0"),
                           ("range_1e38", dict(rng=1e38), "the pA sums overflow"), ("range_1e-30", dict(rng=1e-30), "tiny pA"),
                           ("offset_fraction", dict(off=10.37), "fractional offset"),
                           ("offset_nan", dict(off=float("nan")), "every pA is NaN"),
                           ("offset_negative", dict(off=-600.0), "pA changes sign inside the read"),
                           ("range_negative", dict(rng=-RNG), "negative unit, negative pA: clamped to 0")):
        c.append(case("scale_" + name, base, note, **kw))
    c.append(case("scale_decreasing_polya", sig((2000, B), (19300, ADAPT), (700, ADAPT - 18), (8000, B)),
                  "negative range and raw + offset < 0: pA positive and DEcreasing in raw, a polyA is found below the adaptor",
                  dig=820.0, off=-800.0, rng=-RNG))
    c.append(case("scale_decreasing_noisy", sig((2000, B), (19300, ADAPT), (700, ADAPT - 18), (8000, B), noise=4, seed=16),
                  "the same with noise", dig=820.0, off=-800.0, rng=-RNG))
    names = [k.name for k in c]
    assert len(set(names)) == len(names)
    return c


def finite_cases(cat):
    """the part of the catalogue a BLOW5 file can hold and whose pA are finite"""
    return [k for k in cat if np.isfinite(k.off) and k.dig != 0.0]


class ShimCase(NamedTuple):
    name: str
    raw: np.ndarray
    p: AdaptP
    note: str


def shim_cases():
    """30 000-sample reads for the jnnv2 shim with hi / lo / seg_dist set around the read's own run length and run gap"""
    out = []
    for scale in (0.5, 0.7):
        L, G = SHIM_RUN_LEN[scale], SHIM_RUN_GAP[scale]
        for name, hi, lo in (("len==hi", L, 100), ("len==hi+1", L - 1, 100), ("len==lo", 200000, L), ("len==lo-1", 200000, L + 1)):
            out.append(ShimCase("%s_scale%g" % (name, scale), shim_dip(), AdaptP(scale, 1500, hi, lo), name))
        out.append(ShimCase("gap==seg_dist_scale%g" % scale, two_dips(1200, 0), AdaptP(scale, G, 200000, 100), "two runs"))
        out.append(ShimCase("gap==seg_dist-1_scale%g" % scale, two_dips(1200, 0), AdaptP(scale, G + 1, 200000, 100), "merged"))
    return out


class PaCase(NamedTuple):
    name: str
    pa: np.ndarray
    top: float
    bot: float
    note: str


def pa_sig(*parts):
    return np.concatenate([np.full(int(n), v, dtype=F) for n, v in parts])


def pa_cases():
    """pA arrays straight into find_polya: what raw reads cannot reach (NaN samples, equality with a threshold, the clamp)"""
    I, O, T, B = 100.0, 150.0, 120.0, 80.0
    nan = float("nan")
    out = []
    for n in (219, 220, 249, 250):
        out.append(PaCase("stretch_%d" % n, pa_sig((500, O), (n, I), (100, O), (600, I), (300, O)), T, B, "c = %d at the close" % (n + 30)))
    out.append(PaCase("merge_199", pa_sig((50, O), (400, I), (199, O), (400, I), (300, O), (400, I), (100, O)), T, B, "merged, then a second segment"))
    out.append(PaCase("nomerge_200", pa_sig((50, O), (400, I), (200, O), (400, I), (100, O)), T, B, "two segments"))
    out.append(PaCase("open_at_0", pa_sig((400, I), (100, O)), T, B, "opens at sample 0"))
    out.append(PaCase("open_tail", pa_sig((10, O), (400, I), (300, O), (700, I)), T, B, "second stretch open at the end"))
    out.append(PaCase("only_open", pa_sig((10, O), (900, I)), T, B, "nothing closes"))
    x = pa_sig((20, O), (700, I), (100, O)); x[20 + 14:720:15] = O
    out.append(PaCase("scattered_errors", x, T, B, "31st scattered error closes"))
    x = pa_sig((20, O), (700, I), (100, O)); x[20 + 9:720:23] = nan
    out.append(PaCase("nan_errors", x, T, B, "NaN samples count as errors"))
    out.append(PaCase("all_nan", pa_sig((3000, nan)), T, B, "nothing in range"))
    out.append(PaCase("nan_thresholds", pa_sig((10, O), (900, I), (100, O)), nan, B, "top is NaN: nothing in range"))
    out.append(PaCase("level==top", pa_sig((10, O), (400, T), (100, O), (400, I), (100, O)), T, B, "a stretch AT top is out of range"))
    out.append(PaCase("level==bot", pa_sig((10, O), (400, B), (100, O), (400, I), (100, O)), T, B, "a stretch AT bot is out of range"))
    out.append(PaCase("clamp_high_in_range", pa_sig((10, 0.0), (400, 5000.0), (100, 0.0)), 1250.0, 1150.0, "5000 pA is clamped to 1200: in range"))
    out.append(PaCase("clamp_low_in_range", pa_sig((10, 50.0), (400, -300.0), (100, 50.0)), 5.0, -5.0, "negative pA is clamped to 0: in range"))
    out.append(PaCase("inf_samples", pa_sig((10, O), (300, I), (20, float("inf")), (300, I), (100, float("-inf"))), T, B, "+-inf are clamped, out of range"))
    out.append(PaCase("late", pa_sig((70000, O), (400, I), (100, O)), T, B, "a segment 68 tiles in"))
    out.append(PaCase("short_10", pa_sig((10, I)), T, B, "shorter than anything"))
    return out


def catalogue_sha256() -> str:
    h = hashlib.sha256()
    for k in catalogue():
        h.update(k.name.encode() + b"\0" + k.raw.tobytes() + np.array([k.dig, k.off, k.rng], dtype="<f8").tobytes() + bytes([k.rna]))
    for k in shim_cases():
        h.update(k.name.encode() + b"\0" + k.raw.tobytes() + repr(tuple(k.p)).encode())
    for k in pa_cases():
        h.update(k.name.encode() + b"\0" + k.pa.tobytes() + np.array([k.top, k.bot], dtype="<f4").tobytes())
    return h.hexdigest()


def tag_table(cat=None):
    """-> {tag: [names of the reads (with the pore) it fires on]} over the catalogue, the shim cases and the pA arrays"""
    table = {}
    for k in cat or catalogue():
        for pore in (0, 2):
            for t in prefix_model(k.raw, k.dig, k.off, k.rng, 1, pore)[2]:
                table.setdefault(t, []).append("%s/pore%d" % (k.name, pore))
    for k in shim_cases():
        for t in jnnv2_model(k.raw, k.p)[1]:
            table.setdefault("shim " + t, []).append(k.name)
    for k in pa_cases():
        for t in polya_model(k.pa, k.top, k.bot)[1]:
            table.setdefault("pa " + t, []).append(k.name)
    return table


if __name__ == "__main__":
    for name, v in run_searches().items():
        print("%s = %r" % (name, v))
    for t, names in sorted(tag_table().items()):
        print("%-48s %3d  %s" % (t, len(names), ", ".join(names[:3])))
    print(catalogue_sha256())
