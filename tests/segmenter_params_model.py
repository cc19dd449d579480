"""Yardstick of the segmenters with caller-supplied parameters (sgk_prefix_param, sgk_jnnv2_param, sgk_jnn_param).

A serial numpy model of jnnv2 (src/jnn.c:99-179) with ANY window: integer prefix sums for the rolling totals,
float32(tot) / float32(W), the sequential float32 mean and std of the m = n - W means, then the run finder of
jnn.c:125-167.  tests/prefix_cases.py holds the same model for the window 2000.  The prefix steps are composed here as
src/cfunc.c:169-216 composes them: adaptor, meanf of the pA region, the band, jnn_pa with the polyA set, first segment.

The reads of the window grid are made from seeds (gen_read); tests/golden/segmenter_params.json keeps the seeds and the
reference's own answers, recorded by tests/golden/make_golden_segmenter_params.py."""
from __future__ import annotations

import json
import os
from typing import NamedTuple

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "segmenter_params.json")

WINDOWS = (2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1999, 2001, 4096, 13981)
EXTRA = (1, 2, 1023, 1024, 1025, 3000)      # read lengths W + extra: extra = number of rolling means
WINDOW_MAX = 13981
BIG = 1 << 30


class AdaptW(NamedTuple):          # jnnv2_param_t
    std_scale: float
    seg_dist: int
    window: int
    hi: int
    lo: int


def seqsum(x) -> np.float32:
    x = np.asarray(x, dtype=F)
    return F(0) if x.size == 0 else np.cumsum(x, dtype=F)[-1]


def meanf(x):
    with np.errstate(all="ignore"):
        return seqsum(x) / F(len(x))


def rolling_means(raw, w: int):
    c = np.clip(np.asarray(raw, dtype=np.int64), 0, 1200)
    cs = np.concatenate([[0], np.cumsum(c)])
    m = c.size - w
    return (cs[w:w + m] - cs[:m]).astype(F) / F(w)


class Flags(NamedTuple):           # what of a read the run finder looks at: independent of seg_dist / hi / lo
    lt: list
    gt: list


def flags(raw, w: int, std_scale: float) -> Flags:
    t = rolling_means(raw, w)
    with np.errstate(all="ignore"):
        mn = seqsum(t) / F(t.size)
        d = t - mn
        sd = np.sqrt(seqsum(d * d) / F(t.size))
        bot = mn - sd * F(std_scale)
        return Flags((t < bot).tolist(), (t > bot).tolist())


def runs_of(fl: Flags, seg_dist: int):
    """-> (merged runs [[start, end], ...], tags) of jnn.c:125-158"""
    tags = set()
    begin, start, end = False, 0, 0
    segs = []
    m = len(fl.lt)
    for j in range(m):
        if fl.lt[j]:
            if not begin:
                start, begin = j, True
                if j == 0:
                    tags.add("open_at_0")
            else:
                end = j
        elif begin and fl.gt[j]:
            if j == m - 1:
                tags.add("close_on_last")
            if end == 0:
                tags.add("end==0")
            if start // 1024 != j // 1024:
                tags.add("straddles_tile")
            if start // 16 != j // 16:
                tags.add("straddles_lane")
            if segs and start - segs[-1][1] < seg_dist:
                if start - segs[-1][1] == seg_dist - 1:
                    tags.add("merge_at_seg_dist-1")
                segs[-1][1] = end
            else:
                if segs and start - segs[-1][1] == seg_dist:
                    tags.add("no_merge_at_seg_dist")
                segs.append([start, end])
            start, end, begin = 0, 0, False
        elif begin and not fl.gt[j]:
            tags.add("t==bot_inside")
    if begin:
        tags.add("open_at_end")
    return segs, tags


def pick(segs, w: int, hi: int, lo: int):
    tags = set()
    for a, b in segs:
        for v, name in ((lo - 1, "len==lo-1"), (lo, "len==lo"), (hi, "len==hi"), (hi + 1, "len==hi+1")):
            if b - a == v:
                tags.add(name)
        if b - a > hi or b - a < lo:
            continue
        return (a + w // 2 - 1, b + w // 2 - 1), tags
    return (0, 0), tags


def jnnv2_model(raw, p: AdaptW, fl: Flags = None):
    """-> ((x, y), tags)"""
    if not len(raw) > p.window:
        return (-1, -1), {"too_short"}
    fl = fl if fl is not None else flags(raw, p.window, p.std_scale)
    segs, tags = runs_of(fl, p.seg_dist)
    ans, t2 = pick(segs, p.window, p.hi, p.lo)
    return ans, tags | t2


# ---------------------------------------------------------------- the prefix steps (src/cfunc.c:169-216)
class PolyW(NamedTuple):
    corrector: int
    seg_dist: int
    window: int
    stall_len: float
    error: int
    shift: float
    band: float


POLYA_PRESET = PolyW(50, 200, 250, 1.0, 30, 30.0, 20.0)


def to_pa(raw, dig, off, rng):
    with np.errstate(all="ignore"):
        unit = F(np.float64(rng) / np.float64(dig))
        return (np.asarray(raw, dtype=F) + F(off)) * unit


def polya_thresholds(m_a, q: PolyW):
    """top = (m_a + shift) + band, bot = (m_a + shift) - band: one float32 rounding per operator (cfunc.c:191)"""
    with np.errstate(all="ignore"):
        mid = F(m_a) + F(q.shift)
        return mid + F(q.band), mid - F(q.band)


def polya_first(orc, pa, top, bot, q: PolyW):
    """first segment of oracle.jnn_pa with the set, (-1, -1) if none (find_polya, src/jnn.c:352-374)"""
    p = orc.jnn_param(std_scale=-1.0, corrector=q.corrector, seg_dist=q.seg_dist, window=q.window, stall_len=q.stall_len,
                      error=q.error, top=float(top), bot=float(bot))
    x, y = orc.jnn_pa(pa, p)
    return (int(x[0]), int(y[0])) if len(x) else (-1, -1)


def prefix_model(orc, raw, dig, off, rng, rna, ap: AdaptW, q: PolyW, adaptor=None):
    """-> (adaptor (x, y), polyA (x, y) RELATIVE to adapt_y as sgk_prefix_rec_t holds them); adaptor: jnnv2_model's
    answer for (raw, ap) where the caller has it already"""
    ax, ay = adaptor if adaptor is not None else jnnv2_model(raw, ap)[0]
    if ay <= 0 or not rna:
        return (ax, ay), (-1, -1)
    pa = to_pa(raw, dig, off, rng)
    top, bot = polya_thresholds(meanf(pa[ax:ay]), q)
    return (ax, ay), polya_first(orc, pa[ay:], top, bot, q)


# ---------------------------------------------------------------- the reads of the window grid
def gen_read(w: int, extra: int, seed: int, shift: int = 0):
    """A read of w + extra samples: piecewise levels whose pieces are a fraction of `extra` long (the rolling mean of a
    window moves only through the samples that enter and leave it), +-4 of noise, a few samples outside [0, 1200]
    for the outlier clamp; `shift` slides the read along its signal."""
    n = w + extra
    rng = np.random.default_rng([w, extra, seed])
    total = n + 64
    out = np.empty(total, dtype=np.int64)
    lo_len, hi_len = max(1, extra // 10), max(2, extra // 3)
    i = 0
    while i < total:
        k = int(rng.integers(lo_len, hi_len + 1))
        out[i:i + k] = int(rng.integers(300, 1101))
        i += k
    out += rng.integers(-4, 5, size=total)
    wild = rng.random(total) < 0.01
    out[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -50, 1500)
    return out[shift:shift + n].astype(np.int16)


class GridRead(NamedTuple):
    window: int
    extra: int
    seed: int
    shift: int


def variants_for(w: int, raw, std_scale: float):
    """parameter sets at the decision edges of THIS read's runs: merge at seg_dist - 1 and not at seg_dist, b - a at
    lo - 1, lo, hi, hi + 1 (the model's unmerged runs give the numbers; the sets are inputs like any other)"""
    out = [AdaptW(std_scale, 0, w, BIG, 1)]
    if len(raw) <= w:
        return out
    segs, _ = runs_of(flags(raw, w, std_scale), 0)
    if len(segs) >= 2:
        g = segs[1][0] - segs[0][1]
        if g >= 1:
            out += [AdaptW(std_scale, g + 1, w, BIG, 1), AdaptW(std_scale, g, w, BIG, 1)]
    long_runs = [b - a for a, b in segs if b - a >= 2]
    if long_runs:
        ln = long_runs[0]
        out += [AdaptW(std_scale, 0, w, BIG, ln), AdaptW(std_scale, 0, w, BIG, ln + 1), AdaptW(std_scale, 0, w, ln, 1),
                AdaptW(std_scale, 0, w, ln - 1, 1)]
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def grid_reads(gold, w: int):
    return [GridRead(w, e, s, sh) for (e, s, sh) in gold["windows"][str(w)]["reads"]]


def grid_variants(gold, w: int):
    return [AdaptW(F(v[0]).item(), v[1], w, v[2], v[3]) for v in gold["windows"][str(w)]["variants"]]


def trivial(ans) -> bool:
    return tuple(ans) in ((0, 0), (-1, -1))


# ---------------------------------------------------------------- the jnn and polyA sets and their reads
#: jnn_param_t sets: the two presets, two sets of neither, and one of the domain outside the wave kernel's
JNN_SETS = [dict(std_scale=0.75, corrector=50, seg_dist=50, window=150, stall_len=0.25, error=5),     # cDNA preset
            dict(std_scale=0.75, corrector=50, seg_dist=50, window=1000, stall_len=1.0, error=5),     # dRNA preset
            dict(std_scale=0.4, corrector=17, seg_dist=120, window=60, stall_len=0.5, error=2),       # none of them
            dict(std_scale=-1.0, corrector=50, seg_dist=200, window=250, stall_len=1.0, error=30, top=560.0, bot=420.0),
            dict(std_scale=0.6, corrector=17, seg_dist=30, window=32, stall_len=0.5, error=40)]       # outside the wave kernel
JNN_READS = ((3000, 1), (20011, 2), (40000, 3), (3000, 4), (20011, 5), (40000, 6))   # (samples, seed)


def gen_jnn_read(n: int, seed: int):
    """A read for jnn_core: noisy pieces around changing levels with quiet stretches (stalls) of up to 3 000 samples
    between them, a few samples outside [0, 1200]"""
    rng = np.random.default_rng([7, n, seed])
    out = np.empty(n, dtype=np.int64)
    i = 0
    while i < n:
        if rng.random() < 0.25:
            k, level, noise = int(rng.integers(40, 3001)), int(rng.integers(430, 560)), 6
        else:
            k, level, noise = int(rng.integers(5, 400)), int(rng.integers(300, 950)), 40
        k = min(k, n - i)
        out[i:i + k] = level + rng.integers(-noise, noise + 1, size=k)
        i += k
    wild = rng.random(n) < 0.003
    out[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -20, 1300)
    return out.astype(np.int16)


def jnn_reads():
    return [gen_jnn_read(n, seed) for n, seed in JNN_READS]


def polya_reads():
    """the RNA reads of the hand-made catalogue (tests/prefix_cases.py) that a file can hold, up to 60 000 samples"""
    import prefix_cases as P
    return [k for k in P.finite_cases(P.catalogue()) if k.rna and k.raw.size <= 60000]


POLYA_ADAPTOR = AdaptW(0.5, 1500, 2000, 200000, 2000)   # the adaptor set the polyA sets are tried behind


def polya_sets(cat):
    """polyA sets for both routes of the GPU: one ulp off the preset, error below and at the corrector, stall_len 0.5, a
    set whose `c % w` correction fires, short windows, and bands that put bot (then top) exactly ON a sample of a read's
    tail and one ulp to either side of it"""
    pre = POLYA_PRESET
    up = float(np.nextafter(F(30), F(31))), float(np.nextafter(F(20), F(19)))
    sets = [pre._replace(shift=up[0]), pre._replace(band=up[1]), pre._replace(error=49), pre._replace(error=50),
            pre._replace(stall_len=0.5), pre._replace(stall_len=0.5, window=300),
            pre._replace(corrector=10, error=10, window=64, seg_dist=40), pre._replace(corrector=12, error=3, window=40, seg_dist=25),
            pre._replace(shift=12.5, band=35.25), pre._replace(shift=-40.0, band=0.0)]
    for k in cat:
        (ax, ay), _ = jnnv2_model(k.raw, POLYA_ADAPTOR)
        if ay <= 0:
            continue
        pa = to_pa(k.raw, k.dig, k.off, k.rng)
        mid = F(meanf(pa[ax:ay]) + F(30))
        tail = pa[ay:]
        for side in (-1, 1):
            near = tail[(tail - mid) * side > 5]
            if not near.size:
                continue
            v = near[np.argmin(np.abs(near - mid))]
            band = F(abs(v - mid))
            if not (F(mid + side * band) == v):
                continue
            for bnd in (band, np.nextafter(band, F(0)), np.nextafter(band, F(1e9))):
                sets.append(pre._replace(band=float(bnd)))
        break
    return sets


def polya_inputs(k, q: PolyW, adaptor):
    """what find_polya is called with for catalogue read k behind the adaptor answer: (pA tail, top, bot), or None"""
    ax, ay = adaptor
    if ay <= 0:
        return None
    pa = to_pa(k.raw, k.dig, k.off, k.rng)
    top, bot = polya_thresholds(meanf(pa[ax:ay]), q)
    return pa[ay:], top, bot
