"""The catalogue of hand-made reads for the medians of `stat` and a plain model of the GPU's windows.

The three medians (raw, pA, and the region medians of prefix) are order statistics; the GPU finds them with windowed
histograms and a radix fallback.  `model(case)` restates the window arithmetic of every form -- mean = sequential
float32 sum / n, c = trunc(clamp(mean)), lo by the form's rule, ranks k = n // 2 and, for a negative unit, k2 = n - 1 - k
-- and returns, per form, the SET OF DECISION EDGES the read sits on (the tags below).  test_median_cases_cpu.py requires
every tag on every form it is meaningful on: that is what keeps this catalogue from going soft.

The forms:
    wave    k_stat_wave / k_long_chains: 2048 bins, lo clamped to int16, edge bins distrusted, 32 bins per lane
    kmed    k_median: 2048 bins up to 65 536 samples, 8192 above; clamped, edge bins distrusted, 8 / 32 bins per thread
    h32     k_moments<HIST>: 32 bins per lane, NOT clamped, bins 0 and 31 trusted, anything outside flagged
    select  block_select (4096 x 16), reached when kmed's window does not settle the read

The building block (`mix`) is a read with most samples at the wanted median and a minority far away: the minority places
the mean, and so the window, independently of the median.

The tie class (`Case.tie`): scales under which pA values compare equal without being the same bits (+0 / -0) or do not
order at all (NaN).  There the pA median is not pA(raw order statistic) but whatever element the reference's selection
leaves at n / 2.

No GPU, no torch.  `python tests/median_cases.py` prints the tag -> read table.
"""
import zlib
from typing import NamedTuple

import numpy as np

F = np.float32
DIG, OFF, RNG = 8192.0, 10.0, 1402.882324      # an ordinary scale


class Case(NamedTuple):
    name: str
    raw: np.ndarray      # int16
    dig: float
    off: float
    rng: float
    why: str
    lead: int = 0        # samples between a 16-byte boundary and the read's first sample (GPU placement)
    tie: bool = False    # the tie class: the pick among equal-comparing / unordered pA values matters


class FloatCase(NamedTuple):
    name: str
    x: np.ndarray        # float32
    why: str


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


# ---------------------------------------------------------------------------------------------- the model
def unit_of(dig, rng) -> np.float32:
    with np.errstate(all="ignore"):
        return F(rng) / F(dig)


def to_pa(v, dig, off, rng) -> np.float32:
    """signal_in_picoamps of one sample: ((float)raw + (float)offset) * ((float)range / (float)digitisation)"""
    with np.errstate(all="ignore"):
        return F(F(v) + F(off)) * unit_of(dig, rng)


def seq_mean(raw) -> np.float32:
    """float sum = 0; for (...) sum += x[i]; sum / n"""
    return np.cumsum(np.asarray(raw).astype(F), dtype=F)[-1] / F(len(raw))


def centre(mean) -> int:
    """(int) of the clamped float mean: truncation towards zero"""
    return int(np.trunc(min(max(float(mean), -32768.0), 32767.0)))


def ranks(n, unit):
    k = n // 2
    k2 = n - 1 - k
    mirrored = bool(unit < 0) and k2 != k      # (-0 < 0 is false: a unit of -0 is not mirrored)
    return k, (k2 if mirrored else k), mirrored


def _window_tags(s, k, k2, mirrored, mean, nb, per):
    """a clamped window of nb bins whose two edge bins are distrusted; `per` bins per lane / thread"""
    n = s.size
    tags = set()
    c = centre(mean)
    lo = min(max(c - nb // 2, -32768), 32768 - nb)
    cf = int(np.floor(min(max(float(mean), -32768.0), 32767.0)))
    lof = min(max(cf - nb // 2, -32768), 32768 - nb)

    def bin_of(v, lo_):
        return min(max(int(v) - lo_, 0), nb - 1)

    def inside(v, lo_):
        return 0 < bin_of(v, lo_) < nb - 1

    vk, vk2 = int(s[k]), int(s[k2])
    for p, nm in ((-1, "lo-1"), (0, "lo"), (1, "lo+1"), (nb - 2, "lo+nb-2"), (nb - 1, "lo+nb-1"), (nb, "lo+nb")):
        if vk - lo == p:
            tags.add("k@" + nm)
    trusted = inside(vk, lo) and inside(vk2, lo)
    tags.add("trusted" if trusted else "fallback")
    if mirrored:
        tags.add("mirrored")
        if inside(vk, lo) and not inside(vk2, lo):
            tags.add("k_in_k2_out")
        if not inside(vk, lo) and inside(vk2, lo):
            tags.add("k_out_k2_in")
        if trusted and bin_of(vk, lo) // per != bin_of(vk2, lo) // per:
            tags.add("k_k2_other_owner")
    if inside(vk, lo):
        acc, h = int(np.count_nonzero(s < vk)), int(np.count_nonzero(s == vk))
        if h > 1 and k == acc:
            tags.add("k==acc")
        if h > 1 and k == acc + h - 1:
            tags.add("k==acc+h-1")
    if -1.0 < float(mean) < 0.0:
        tags.add("mean_in(-1,0)")
    if -17.0 < float(mean) < -16.0:
        tags.add("mean_in(-17,-16)")
    if (inside(vk, lo) and inside(vk2, lo)) != (inside(vk, lof) and inside(vk2, lof)):
        tags.add("trunc_decides")
    if c - nb // 2 > 32768 - nb:
        tags.add("lo_clamped_high")
    if c - nb // 2 < -32768:
        tags.add("lo_clamped_low")
    return tags, trusted


def _h32_tags(s, k, k2, mirrored, mean):
    """32 bins per lane around the mean: not clamped, bins 0 and 31 trusted, a rank outside flags the read"""
    tags = set()
    c = centre(mean)
    lo = c - 16
    lof = int(np.floor(min(max(float(mean), -32768.0), 32767.0))) - 16
    vk, vk2 = int(s[k]), int(s[k2])
    for p, nm in ((-1, "lo-1"), (0, "lo"), (1, "lo+1"), (30, "lo+nb-2"), (31, "lo+nb-1"), (32, "lo+nb")):
        if vk - lo == p:
            tags.add("k@" + nm)

    def inside(v, lo_):
        return 0 <= int(v) - lo_ < 32

    found = inside(vk, lo) and inside(vk2, lo)
    tags.add("trusted" if found else "fallback")
    if mirrored:
        tags.add("mirrored")
        if inside(vk, lo) and not inside(vk2, lo):
            tags.add("k_in_k2_out")
        if not inside(vk, lo) and inside(vk2, lo):
            tags.add("k_out_k2_in")
        if found and vk != vk2:
            tags.add("k_k2_other_bin")
    if inside(vk, lo):
        acc, h = int(np.count_nonzero(s < vk)), int(np.count_nonzero(s == vk))
        if h > 1 and k == acc:
            tags.add("k==acc")
        if h > 1 and k == acc + h - 1:
            tags.add("k==acc+h-1")
    if -1.0 < float(mean) < 0.0:
        tags.add("mean_in(-1,0)")
    if -17.0 < float(mean) < -16.0:
        tags.add("mean_in(-17,-16)")
    if found != (inside(vk, lof) and inside(vk2, lof)):
        tags.add("trunc_decides")
    if lo + 31 > 32767:
        tags.add("window_above_int16")
    if lo < -32768:
        tags.add("window_below_int16")
    return tags


def _select_tags(s, k, k2, mirrored):
    """block_select: 4096 coarse bins of 16 keys (key = value + 32768), then the 16 fine bins of the coarse bin"""
    tags = set()
    keys = s.astype(np.int64) + 32768
    for w, rank in enumerate((k, k2) if mirrored else (k,)):
        key = int(keys[rank])
        coarse = key >> 4
        rank2 = rank - int(np.count_nonzero((keys >> 4) < coarse))
        in_bin = keys[(keys >> 4) == coarse]
        below = int(np.count_nonzero(in_bin < key))
        h = int(np.count_nonzero(in_bin == key))
        if (key & 15) == 0:
            tags.add("med%16==0")
        if (key & 15) == 15:
            tags.add("med%16==15")
        if rank2 == 0:
            tags.add("rank2==0")
        if h > 1 and rank2 == below + h - 1:
            tags.add("rank2==last_of_fine_bin")
        if key == 0:
            tags.add("median==-32768")
        if key == 65535:
            tags.add("median==32767")
    if np.count_nonzero(keys == keys[0]) == keys.size:
        tags.add("constant")
    if np.unique(keys).size > 8192:
        tags.add("distinct>8192")
    if mirrored and (int(keys[k]) >> 4) != (int(keys[k2]) >> 4):
        tags.add("mirror_other_coarse_bin")
    return tags


def model(case: Case):
    """-> {form: set of tags}; 'any' holds what does not depend on the form (length, scale)"""
    raw = np.asarray(case.raw, dtype=np.int16)
    n = raw.size
    unit = unit_of(case.dig, case.rng)
    k, k2, mirrored = ranks(n, unit)
    s = np.sort(raw)
    mean = seq_mean(raw)
    out = {}
    out["wave"], _ = _window_tags(s, k, k2, mirrored, mean, 2048, 32)
    nb = 2048 if n <= 65536 else 8192
    out["kmed"], settled = _window_tags(s, k, k2, mirrored, mean, nb, nb // 256)
    out["kmed"].add("nb=%d" % nb)
    out["h32"] = _h32_tags(s, k, k2, mirrored, mean)
    out["select"] = set() if settled else _select_tags(s, k, k2, mirrored)
    a = {"n=%d" % n} if n in (1, 2, 3, 8192, 8193, 20001, 65536, 65537) else set()
    if unit < 0:
        a.add("unit<0,n_odd" if n % 2 else "unit<0,n_even")
        if n == 2:
            a.add("unit<0,n=2")
    if unit == 0 and np.signbit(unit):
        a.add("unit=-0")
        assert not mirrored
    if case.tie:
        a.add("tie")
    out["any"] = a
    return out


def pa_rule(case: Case) -> np.float32:
    """what the windowed kernels rely on outside the tie class: pA median = pA(raw order statistic of rank k2)"""
    raw = np.asarray(case.raw, dtype=np.int16)
    _, k2, _ = ranks(raw.size, unit_of(case.dig, case.rng))
    return to_pa(np.sort(raw)[k2], case.dig, case.off, case.rng)


# ---------------------------------------------------------------------------------------------- builders
def mix(n, groups, target_mean, side, seed):
    """`groups` [(value, count)] as given + a minority on `side` (+1 above every group, -1 below) whose values make the
    real mean of the n samples target_mean; shuffled with `seed`"""
    fixed = sum(cnt for _, cnt in groups)
    m = n - fixed
    assert m >= 0
    vals = [np.full(cnt, v, dtype=np.int64) for v, cnt in groups]
    if m:
        need = int(round(target_mean * n)) - sum(v * cnt for v, cnt in groups)
        q, r = divmod(need, m)
        pull = np.full(m, q, dtype=np.int64)
        pull[:r] += 1
        gv = [v for v, _ in groups]
        assert -32768 <= pull.min() and pull.max() <= 32767, (pull.min(), pull.max())
        assert (pull.min() > max(gv)) if side > 0 else (pull.max() < min(gv)), (side, pull.min(), pull.max(), gv)
        vals.append(pull)
    a = np.concatenate(vals).astype(np.int16)
    np.random.RandomState(seed).shuffle(a)
    return a


def mix_to(n, groups, c, side, seed):
    """mix() with the minority tuned until the SEQUENTIAL FLOAT mean truncates to c (long sums round away from the real
    mean by a few codes)"""
    for d in sorted(np.arange(-4.0, 4.0, 0.05), key=abs):
        raw = mix(n, groups, mean_for(c) + d, side, seed)
        got = seq_mean(raw)
        if centre(got) == c and abs(float(got) - mean_for(c)) < 0.4:
            return raw
    raise AssertionError((n, groups, c))


def pull_count(n, value, target_mean, cap=None):
    """how many far samples move the mean of n samples at `value` to target_mean (they sit ~22 000 codes away)"""
    room = 22000.0
    m = int(np.ceil(abs(target_mean - value) * n / room))
    m = max(m, 1)
    assert m < (n - 1) // 2, (n, value, target_mean, m)
    return m


def mean_for(c):
    """a mean whose truncation is c (|c| >= 1)"""
    return c + 0.5 if c > 0 else c - 0.5


def at_offset(name, n, med, nb, p, seed, why, dig=DIG, off=OFF, rng=RNG, unclamped_lo=None):
    """a read whose median `med` sits at lo + p of a window of nb bins centred on trunc(mean)"""
    c = med - p + nb // 2
    assert abs(c) >= 1
    tm = mean_for(c)
    side = 1 if tm > med else -1
    m = pull_count(n, med, tm)
    raw = mix_to(n, [(med, n - m)], c, side, seed)
    return Case(name, raw, dig, off, rng, why)


def _positions(nb):
    return ((-1, "lo-1"), (0, "lo"), (1, "lo+1"), (nb - 2, "lo+nb-2"), (nb - 1, "lo+nb-1"), (nb, "lo+nb"))


def _edge_cases():
    out = []
    seed = 100
    # the rank-k value on and beside both edges of every window, on every form that has the window
    for nb, lens, med in ((2048, (1001, 8193), 700), (8192, (65537, 70001), -900), (32, (101, 20001), 480)):
        for n in lens:
            for p, nm in _positions(nb):
                seed += 1
                out.append(at_offset("edge%d_n%d_k@%s" % (nb, n, nm), n, med, nb, p, seed,
                                     "median at %s of the %d-bin window" % (nm, nb)))
    # the same with a negative unit and n odd (not mirrored) / n even inside one value (mirrored, both ranks one bin)
    for nb, n, med in ((2048, 1000, 650), (2048, 999, 650), (32, 100, 520), (32, 99, 520)):
        for p, nm in _positions(nb):
            seed += 1
            out.append(at_offset("edge%d_neg_n%d_k@%s" % (nb, n, nm), n, med, nb, p, seed,
                                 "negative unit, median at %s of the %d-bin window" % (nm, nb), rng=-RNG))
    return out


def _mirror_cases():
    """n even, unit < 0: rank k holds B, rank k2 = k - 1 holds A < B"""
    out = []

    def two(name, n, A, B, c, seed, why):
        h = n // 2
        tm = mean_for(c)
        mid = (A + B) / 2.0
        side = 1 if tm > mid else -1
        m = max(1, int(np.ceil(abs(tm - mid) * n / 20000.0)))
        assert m < h - 1
        groups = [(A, h - m), (B, h)] if side < 0 else [(A, h), (B, h - m)]
        raw = mix_to(n, groups, c, side, seed)
        s = np.sort(raw)
        assert s[h] == B and s[h - 1] == A
        return Case(name, raw, DIG, OFF, -RNG, why)

    for nb, n in ((2048, 1000), (2048, 8192), (8192, 65538), (32, 100)):
        far = 3 * nb // 2 if nb > 32 else 40
        step = 40 if nb > 32 else 5
        out.append(two("mirror%d_n%d_k_in_k2_out" % (nb, n), n, 300 - far, 300, 300 + nb // 4 + 1, 7,
                       "rank k inside the %d-bin window, the mirrored rank below it" % nb))
        out.append(two("mirror%d_n%d_k_out_k2_in" % (nb, n), n, 300, 300 + far, 300 - nb // 4 - 1, 8,
                       "the mirrored rank inside the %d-bin window, rank k above it" % nb))
        out.append(two("mirror%d_n%d_other_owner" % (nb, n), n, 300, 300 + step, 300 + 3, 9,
                       "both ranks inside the %d-bin window, in bins of different lanes / threads" % nb))
    # both ranks far from the mean and in different coarse bins of the two-level select
    out.append(two("mirror_select_other_coarse", 1000, -9000, -8000, -4000, 10, "block_select twice, different coarse bins"))
    return out


def _count_boundary_cases():
    out = []
    for n, unitsign in ((1001, 1), (1000, -1), (8193, 1), (101, 1), (65537, 1)):
        k = n // 2
        # k == acc: exactly k samples below the median's value (the minority, below)
        raw = mix(n, [(500, n - k)], 500 - 6.0 * k / n * 1.0, -1, 21)
        out.append(Case("rank_first_of_bin_n%d" % n, raw, DIG, OFF, unitsign * RNG, "k == acc in the owning bin"))
        # k == acc + h - 1: the median is the last sample of its value
        raw = mix(n, [(500, k + 1)], 500 + 6.0 * (n - k - 1) / n, 1, 22)
        out.append(Case("rank_last_of_bin_n%d" % n, raw, DIG, OFF, unitsign * RNG, "k == acc + h - 1 in the owning bin"))
    return out


def _trunc_cases():
    out = []

    def c_(name, n, med, tm, seed, why, **kw):
        side = 1 if tm > med else -1
        m = pull_count(n, med, tm) if abs(tm - med) * n >= 1 else 0
        raw = mix(n, [(med, n - m)], tm, side, seed)
        return Case(name, raw, kw.get("dig", DIG), kw.get("off", OFF), kw.get("rng", RNG), why)

    for n in (1001, 8193):
        # mean in (-1, 0): c = 0 where floor gives -1; the median at -1024 is in bin 0 (distrusted) instead of bin 1
        out.append(c_("trunc_mean_-0.5_edge2048_n%d" % n, n, -1024, -0.5, 31, "truncation puts the median into the edge bin"))
        out.append(c_("trunc_mean_-16.5_edge2048_n%d" % n, n, -1040, -16.5, 32, "truncation, mean in (-17, -16), edge bin"))
    out.append(c_("trunc_mean_-0.5_edge8192", 65537, -4096, -0.5, 33, "truncation puts the median into the 8192 window's edge bin"))
    out.append(c_("trunc_mean_-16.5_edge8192", 65537, -4112, -16.5, 33, "truncation, mean in (-17, -16), 8192 window"))
    # 32 bins: lo = c - 16; the median at lo - 1 under truncation is bin 0 under floor
    out.append(c_("trunc_mean_-0.5_h32", 101, -17, -0.5, 34, "32-bin window: truncation leaves the median outside"))
    out.append(c_("trunc_mean_-16.5_h32", 101, -33, -16.5, 35, "32-bin window, mean in (-17, -16)"))
    # clamped windows and the int16 limits themselves
    rs = np.random.RandomState(36)
    for n in (501, 8192):
        hi = (32767 - rs.randint(0, 300, size=n)).astype(np.int16)
        out.append(Case("clamp_high_n%d" % n, hi, DIG, OFF, RNG, "mean above 32767 - nb/2: lo clamped"))
        out.append(Case("clamp_low_n%d" % n, (-32768 + rs.randint(0, 300, size=n)).astype(np.int16), DIG, OFF, RNG,
                        "mean below -32768 + nb/2: lo clamped"))
    out.append(Case("clamp_high_8192", (32767 - rs.randint(0, 3000, size=65537)).astype(np.int16), DIG, OFF, RNG, "8192 window clamped high"))
    out.append(Case("clamp_low_8192", (-32768 + rs.randint(0, 3000, size=65537)).astype(np.int16), DIG, OFF, -RNG, "8192 window clamped low"))
    out.append(Case("h32_above_int16", (32767 - rs.randint(0, 9, size=101)).astype(np.int16), DIG, OFF, RNG, "32 bins reach past 32767"))
    out.append(Case("h32_below_int16", (-32768 + rs.randint(0, 9, size=101)).astype(np.int16), DIG, OFF, RNG, "32 bins reach below -32768"))
    for n in (1, 2, 9, 1001, 8192, 65537):
        out.append(Case("all_32767_n%d" % n, np.full(n, 32767, dtype=np.int16), DIG, OFF, RNG, "median 32767: key 65535, thread 255"))
        out.append(Case("all_-32768_n%d" % n, np.full(n, -32768, dtype=np.int16), DIG, OFF, -RNG, "median -32768: key 0, thread 0"))
    a = np.full(1000, 32767, dtype=np.int16); a[:400] = 32000
    out.append(Case("median_32767_mixed", a, DIG, OFF, -RNG, "median 32767, mirrored"))
    a = np.full(1000, -32768, dtype=np.int16); a[:400] = -32000
    out.append(Case("median_-32768_mixed", a, DIG, OFF, -RNG, "median -32768, mirrored"))
    return out


def _select_cases():
    out = []
    seed = 50
    for n, rng in ((1001, RNG), (1000, -RNG), (70001, RNG)):
        nb = 2048 if n <= 65536 else 8192
        for med in (-20000, -20000 + 15, 12000 - 32768 % 16, 12015):
            seed += 1
            tm = med + (nb if nb == 8192 else 6000) * (1 if med < 0 else -1) * 1.0
            m = pull_count(n, med, tm)
            out.append(Case("select_med%d_n%d" % (med, n), mix(n, [(med, n - m)], tm, 1 if tm > med else -1, seed), DIG, OFF, rng,
                            "two-level select, median = %d mod 16" % ((med + 32768) % 16)))
    # rank2 == 0: the median is the first sample of its coarse bin;  last of its fine bin
    n = 1001; k = n // 2
    raw = mix(n, [(8000, n - k)], 8000 - 9000.0 * 1.0, -1, 61)   # k samples ~18 000 below: mean far below the median
    out.append(Case("select_rank2_0", raw, DIG, OFF, RNG, "rank2 == 0"))
    raw = mix(n, [(-8000, k + 1)], -8000 + 9000.0, 1, 62)
    out.append(Case("select_rank2_last", raw, DIG, OFF, RNG, "rank2 == last of its fine bin"))
    # more than 8192 distinct values, the median ~2000 codes from the mean
    v = np.concatenate([np.arange(-9000, 1), 2 * np.arange(1, 11001)]).astype(np.int16)
    np.random.RandomState(63).shuffle(v)
    out.append(Case("select_distinct_20001", v, DIG, OFF, RNG, "20 001 distinct values"))
    out.append(Case("select_distinct_20001_neg", v[:-1].copy(), DIG, OFF, -RNG, "20 000 distinct values, mirrored"))
    return out


def _length_cases():
    out = []
    rs = np.random.RandomState(70)
    for n in (1, 2, 3, 4, 5, 8192, 8193, 20001, 65536, 65537):
        for sign in (1, -1):
            raw = np.clip(np.rint(rs.normal(500, 40, size=n)), -32768, 32767).astype(np.int16)
            out.append(Case("len%d_%s" % (n, "pos" if sign > 0 else "neg"), raw, DIG, OFF, sign * RNG, "length %d" % n))
    return out


def _alignment_cases():
    """visit_keys: `head` samples up to the first 16-byte boundary, whole 16-byte vectors, `tail` samples; every value
    is distinct, so a sample missed or counted twice moves the median"""
    out = []
    rs = np.random.RandomState(80)
    for lead in range(8):
        head = (8 - lead) % 8
        for tail in range(8):
            n = head + 8 * ((lead + tail) % 3) + tail
            if n == 0:
                n = 8
            raw = (400 + 3 * rs.permutation(n)).astype(np.int16)
            out.append(Case("align_lead%d_tail%d" % (lead, tail), raw, DIG, OFF, RNG if (lead + tail) % 2 else -RNG,
                            "head %d, tail %d, n %d" % (head, tail, n), lead=lead))
        for n in range(1, head):
            raw = (400 + 3 * rs.permutation(n)).astype(np.int16)
            out.append(Case("align_lead%d_n%d_lt_head" % (lead, n), raw, DIG, OFF, -RNG if n % 2 else RNG,
                            "n < head", lead=lead))
    return out


TIE_SCALES = (("range+0", 8192.0, 0.0), ("range-0", 8192.0, -0.0), ("range+1e-44", 8192.0, 1e-44),
              ("range-1e-44", 8192.0, -1e-44), ("dig0_range+", 0.0, 1402.882324), ("dig0_range-", 0.0, -1402.882324))


def _tie_cases():
    """raw + offset is positive, negative and exactly 0 inside one read, under scales that make pA +-0, or +-inf and NaN"""
    out = []
    for si, (nm, dig, rng) in enumerate(TIE_SCALES):
        for n in (3, 4, 6, 7, 16, 33, 64, 79, 200, 1001, 4096):
            rs = np.random.RandomState(1000 + 50 * si + n)
            raw = rs.randint(-20, 20, size=n).astype(np.int16)
            raw[rs.permutation(n)[:3]] = (3, 11, -9)      # raw + offset is zero, positive and negative at least once
            out.append(Case("tie_%s_n%d" % (nm, n), raw, dig, -3.0, rng, "tie class: " + nm, tie=True))
    rs = np.random.RandomState(99)
    raw = rs.randint(-20, 20, size=37).astype(np.int16)
    raw[:3] = (-4, 9, -15)
    out.append(Case("tie_lead5_range-0", raw, 8192.0, 4.0, -0.0,
                    "tie class off the aligned path", lead=5, tie=True))
    return out


def _scale_cases():
    rs = np.random.RandomState(90)
    out = []
    raw = np.clip(np.rint(rs.normal(500, 40, size=1000)), 0, 4000).astype(np.int16)
    out.append(Case("unit_-0_one_signed", raw, 8192.0, 10.0, -0.0, "unit = -0 is not mirrored (every pA is -0)"))
    out.append(Case("unit_tiny_neg", raw, 8192.0, 10.0, -1e-30, "tiny negative unit"))
    out.append(Case("one_sample_dig0", np.array([3], dtype=np.int16), 0.0, -3.0, 1402.882324, "n = 1 and pA = 0 * inf"))
    out.append(Case("one_sample_range0", np.array([-7], dtype=np.int16), 8192.0, 10.0, -0.0, "n = 1 and pA = -3 * -0"))
    out.append(Case("unit_huge_neg", raw[:999], 8192.0, 10.0, -1e38, "huge negative unit: pA overflows"))
    return out


def cases():
    out = (_edge_cases() + _mirror_cases() + _count_boundary_cases() + _trunc_cases() + _select_cases() + _length_cases()
           + _alignment_cases() + _tie_cases() + _scale_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


REGION_PORE = 0     # R9 (sqk-rna002)


def region_cases():
    """reads of tests/prefix_cases.py with an adaptor (and a polyA where the scale leaves one), for the region medians of
    prefix: ordinary, negative (mirrored), and the tie class with raw + offset changing sign inside the adaptor"""
    import prefix_cases
    cat = {k.name: k for k in prefix_cases.catalogue()}
    a, d, t = cat["pa_merge_199"], cat["scale_decreasing_polya"], cat["noisy_edges"]
    o = -401.0    # the median of noisy_edges' adaptor region (6025 .. 11977): raw + offset changes sign inside it
    return [Case("region_ordinary", a.raw, a.dig, a.off, a.rng, "adaptor and polyA, ordinary scale"),
            Case("region_negative", d.raw, d.dig, d.off, d.rng, "negative unit: mirrored region medians"),
            Case("region_polya_zero", a.raw, a.dig, -675.0, a.rng, "offset = -(median of the polyA): its pA median is exactly 0"),
            Case("region_range+0", t.raw, 8192.0, o, 0.0, "tie class in the adaptor region", tie=True),
            Case("region_range-0", t.raw, 8192.0, o, -0.0, "tie class in the adaptor region", tie=True),
            Case("region_range-1e-44", t.raw, 8192.0, o, -1e-44, "tie class, products underflow", tie=True),
            Case("region_dig0_range+", t.raw, 0.0, o, 1402.882324, "tie class: +-inf and NaN", tie=True),
            Case("region_dig0_range-", t.raw, 0.0, o, -1402.882324, "tie class: -+inf and NaN", tie=True)]


def region_file_cases():
    """what a text SLOW5 file can hold of region_cases (all of them: no NaN or infinite header value)"""
    return region_cases()


def range0_reads():
    """six short reads for a text SLOW5 file whose header scale is `range 0`"""
    want = ("tie_range+0_n6", "tie_range+0_n7", "tie_range+0_n33", "tie_range+0_n79", "tie_range+0_n200", "tie_range-0_n64")
    by = {c.name: c for c in _tie_cases()}
    return [by[w] for w in want]


def float_cases():
    """arrays for the float-key radix of k_statf_wave (three levels of 11, 11 and 10 bits)"""
    out = []
    rs = np.random.RandomState(7)

    def add(name, x, why):
        out.append(FloatCase(name, np.ascontiguousarray(x, dtype=F), why))

    nan_p, nan_n = np.uint32(0x7fc00000).view(F), np.uint32(0xffc00000).view(F)
    for n in (1, 2, 3, 10, 11, 100, 101, 2000, 3001):
        x = rs.choice(np.array([0.0, -0.0], dtype=F), size=n)
        add("zeros_mixed_n%d" % n, x, "+0 and -0 mixed")
        x = rs.normal(0, 1, size=n).astype(F)
        x[rs.randint(0, n, size=max(1, n // 3))] = 0.0
        x[rs.randint(0, n, size=max(1, n // 3))] = -0.0
        add("zeros_among_n%d" % n, x, "+-0 around the median")
        x = rs.normal(0, 1, size=n).astype(F)
        x[rs.randint(0, n)] = nan_p
        add("one_nan_n%d" % n, x, "one NaN")
        x = rs.normal(0, 1, size=n).astype(F)
        x[rs.randint(0, n)] = nan_n
        add("one_neg_nan_n%d" % n, x, "one NaN with the sign bit set")
        x = rs.normal(0, 1, size=n).astype(F)
        for _ in range(min(n, 4)):
            x[rs.randint(0, n)] = nan_p if rs.rand() < 0.5 else nan_n
        add("some_nans_n%d" % n, x, "several NaNs of both signs")
        x = rs.normal(0, 1, size=n).astype(F)
        x[rs.randint(0, n, size=max(1, n // 4))] = np.inf
        x[rs.randint(0, n, size=max(1, n // 4))] = -np.inf
        add("infs_n%d" % n, x, "+-inf")
        x = (rs.randint(-50, 50, size=n).astype(np.int32)).astype(F) * F(1e-45)
        add("denormals_n%d" % n, x, "denormals and zeros of both signs")
        base = np.uint32(0x42c80000)
        add("low_bits_n%d" % n, (base + rs.randint(0, 1 << 10, size=n).astype(np.uint32)).view(F), "differ only below bit 10")
        seam = base + (rs.randint(0, 4, size=n).astype(np.uint32) << 9) + (rs.randint(0, 4, size=n).astype(np.uint32) << 20)
        add("seams_n%d" % n, seam.view(F), "differ only around bits 10 and 21, the seams of the radix fields")
    add("all_nan", np.full(5, nan_p), "nothing orders")
    add("sorted", np.arange(1000, dtype=F), "already sorted")
    add("reversed", np.arange(1000, dtype=F)[::-1], "reversed")
    add("all_equal", np.full(1000, 2.5, dtype=F), "all equal")
    return out


if __name__ == "__main__":
    table = {}
    cs = cases()
    for c in cs:
        for form, tags in model(c).items():
            for t in tags:
                table.setdefault((form, t), []).append(c.name)
    for (form, t), names in sorted(table.items()):
        print("%-7s %-26s %3d  %s" % (form, t, len(names), ", ".join(names[:3])))
    print(len(cs), "cases,", sum(c.raw.size for c in cs), "samples;", len(float_cases()), "float cases")
