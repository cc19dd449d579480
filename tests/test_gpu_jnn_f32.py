"""GPU parity: sgk_jnn_f32, jnn_pa (src/jnn.c:295-306) of every read of a float batch and find_polya (src/jnn.c:352-374)
through per-read thresholds, against the oracle segment by segment as integers; there are no tolerances.  The reads are
pA of synthetic reads, the float arrays of tests/jnn_cases.py::pa_cases() (what no raw read can hold) and the hand-made
catalogue of tests/jnn_cases.py as floats, which carries the chunk-seam, merge-round and slot-overflow places of the
chunked automaton over to the float kernels (a read that starts on a 16-byte boundary has the int16 kernel's geometry)."""
import numpy as np
import pytest

import jnn_cases as J

pytestmark = pytest.mark.gpu

F = np.float32
#: the sets of tests/test_gpu_shims.py::test_jnn_raw_and_pa_shims_any_parameters
SETS = [J.JP(0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0),        # cDNA preset
        J.JP(0.75, 50, 50, 1000, 1.0, 5, 0.0, 0.0),        # dRNA preset
        J.JP(0.4, 17, 120, 60, 0.5, 2, 0.0, 0.0),          # none of them (window < 128: the literal loop)
        J.JP(-1.0, 50, 200, 250, 1.0, 30, 560.0, 420.0)]   # the polyA preset, fixed thresholds
POLYA = J.JP(-1.0, 50, 200, 250, 1.0, 30, 0.0, 0.0)        # JNNV1_R9_POLYA == JNNV1_RNA004_POLYA, src/jnn.h:52-72


def _pairs(x, y):
    return [(int(a), int(b)) for a, b in zip(x, y)]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _run(gpu, arrays, p, top=None, bot=None, leads=None, fill=None, slots=None, fb=None):
    """-> (segments per read, cut to the read's slots; n_segs; number of reads that overflowed their slots)"""
    import torch
    from sigtk_amd import device
    if fb is None:
        fb = device.upload_float_reads(arrays, _dev(), leads=leads, fill=fill)
    arena = device.FloatSegArena(fb, slots=slots)
    t = None if top is None else torch.from_numpy(np.asarray(top, dtype=F)).to(_dev())
    b = None if bot is None else torch.from_numpy(np.asarray(bot, dtype=F)).to(_dev())
    device.jnn_f32(fb, arena, gpu.JnnParam(*p), top=t, bot=b)
    torch.cuda.synchronize()
    ns = arena.n_segs.cpu().numpy().view(np.uint32)[:fb.n_reads]
    x, y = arena.x.cpu().numpy(), arena.y.cpu().numpy()
    segs = []
    for r in range(fb.n_reads):
        s, cap = int(arena.slots_host[r]), int(arena.slots_host[r + 1] - arena.slots_host[r])
        k = min(int(ns[r]), cap)
        segs.append(_pairs(x[s:s + k], y[s:s + k]))
    return segs, ns, arena.n_overflowed()


def _want(oracle, x, p):
    with np.errstate(all="ignore"):
        return _pairs(*oracle.jnn_pa(x, oracle.jnn_param(**p._asdict())))


def _compare(gpu, oracle, arrays, p, what, **kw):
    segs, ns, nerr = _run(gpu, arrays, p, **kw)
    bad = []
    for r, x in enumerate(arrays):
        e = _want(oracle, x, p)
        if segs[r] != e or int(ns[r]) != len(e):
            bad.append("%s read %d (n=%d) %r: n_segs %d gpu %r oracle %r" % (what, r, x.size, tuple(p), ns[r], segs[r][:6], e[:6]))
    assert not bad, "\n".join(bad[:20])
    assert nerr == 0, what
    return segs


@pytest.fixture(scope="module")
def synth_pa(gpu, oracle):
    """pA of synthetic reads of both kinds, lengths 1 .. 40 000"""
    lens = [1, 31, 32, 33, 150, 3000, 40000]
    out = []
    for kind in (0, 1):
        reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=43 + kind, kind=kind)
        out += [oracle.pa(raw, dig[r], off[r], rng[r]) for r, raw in enumerate(reads)]
    return out


@pytest.mark.parametrize("k", range(len(SETS)))
def test_parameter_sets(gpu, oracle, synth_pa, k):
    p = SETS[k]
    if p.std_scale < 0:   # fixed thresholds around the level of the signal
        m = float(np.median(np.concatenate(synth_pa)))
        p = p._replace(top=m + 8.0, bot=m - 8.0)
    segs = _compare(gpu, oracle, synth_pa, p, "set %d" % k, leads=[(3 * r) % 4 for r in range(len(synth_pa))], fill=np.nan)
    assert k != 0 or any(len(s) > 1 for s in segs)   # (the comparison is not one of empty lists)


def _in_domain(gpu, p):
    import ctypes as C
    jp = gpu.JnnParam(*p)
    return gpu._param_lib().sgk_jnn_params_check(C.byref(jp)) == gpu.SGK_OK


def _refused(gpu, arrays, p):
    """a set outside sgk_jnn_params_check's domain is SGK_ERR_ARG; -> the set with its window raised into the domain
    (32: from there on sgk_jnn_slots_for bounds a read's segments), or None when something else keeps it out"""
    with pytest.raises(gpu.SigtkGpuError):
        _run(gpu, arrays, p)
    q = p._replace(window=max(p.window, 32))
    return q if _in_domain(gpu, q) else None


def test_pa_cases(gpu, oracle):
    """every float array of pa_cases(), one batch per parameter set: NaN and infinite samples, -0.0 at and below bot,
    levels exactly at top and at bot, NaN thresholds, err-- once and twice.  The err-- sets of pa_cases() have window 20,
    which sgk_jnn_params_check refuses (window >= 32) and sgk_jnn_f32 with it: that refusal is asserted, and the same
    arrays run with window 32, where the model says they still take err-- once and twice."""
    cases = J.pa_cases()
    by_set = {}
    for k in cases:
        by_set.setdefault(k.params, []).append(k)
    assert len(by_set) >= 8
    corrections = set()
    for p, ks in by_set.items():
        arrays = [k.pa for k in ks]
        if not _in_domain(gpu, p):
            p = _refused(gpu, arrays, p)
            assert p is not None
        for x in arrays:
            corrections |= J.jnn_core_model(J.clamp_pa(x), p)[1] & {J.J_CORRECTION, J.J_CORRECTION_TWICE}
        _compare(gpu, oracle, arrays, p, "+".join(k.name for k in ks), leads=[(r + 1) % 4 for r in range(len(ks))], fill=100.0)
    assert corrections == {J.J_CORRECTION, J.J_CORRECTION_TWICE}


def _aligned_leads(arrays):
    """every read on a 16-byte boundary: q space is the int16 kernel's for a read at a multiple of 8 samples"""
    return [0] + [(-a.size) % 4 for a in arrays[:-1]]


def test_catalogue(gpu, oracle):
    """every read of the catalogue as floats, one batch per parameter set (the preset cases with both presets)"""
    cat = J.catalogue()
    by_set = {}
    for k in cat:
        for _, p in J.case_runs(k):
            by_set.setdefault(p, []).append(k)
    names = {k.name for k in cat}
    assert {"no_sync_16384", "no_sync_40000", "no_sync_all_5000", "rich_16384"} <= names
    for p, ks in by_set.items():
        arrays = [k.raw.astype(F) for k in ks]
        if not _in_domain(gpu, p):   # (error -1; window 20: run with the domain's smallest window instead)
            p = _refused(gpu, arrays, p)
            if p is None:
                continue
        segs = _compare(gpu, oracle, arrays, p, "catalogue", leads=_aligned_leads(arrays), fill=np.nan)
        with np.errstate(all="ignore"):
            for k, s in zip(ks, segs):
                if k.raw.min() >= 0 and k.raw.max() <= 1200:   # the clamp does nothing: jnn_core on the read itself
                    assert s == _pairs(*oracle.jnn_core(J.clamp_raw(k.raw), oracle.jnn_param(**p._asdict()))), k.name


@pytest.fixture(scope="module")
def tails(gpu, oracle):
    """pA behind the adaptor of RNA synthetic reads with the thresholds of src/cfunc.c:186-191 shifted as in
    tests/test_gpu_shims.py::test_adaptor_and_polya_shims -> [(tail, top, bot)]"""
    lens = [30000, 100000, 100000, 60000, 45000]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=47, kind=1)
    out = []
    for r, raw in enumerate(reads):
        pa = oracle.pa(raw, dig[r], off[r], rng[r])
        ax, ay = oracle.find_adaptor(raw, 0)
        if ay > 0:
            m_a = float(oracle.statf(pa[ax:ay])[0])
            out.append((pa[ay:], F(m_a + 50.0), F(m_a + 10.0)))
    assert len(out) >= 3
    return out


def test_per_read_thresholds_are_find_polya(gpu, oracle, tails):
    arrays = [t[0] for t in tails]
    top, bot = [t[1] for t in tails], [t[2] for t in tails]
    assert len(set(float(t) for t in top)) == len(top)   # distinct thresholds per read
    segs, ns, nerr = _run(gpu, arrays, POLYA, top=top, bot=bot, leads=[1, 2, 3, 0, 1][:len(arrays)], fill=np.nan)
    assert nerr == 0
    found = 0
    for r, x in enumerate(arrays):
        first = segs[r][0] if segs[r] else (-1, -1)
        for pore in (0, 2):
            assert first == oracle.find_polya(x, float(top[r]), float(bot[r]), pore), (r, pore)
        found += first != (-1, -1)
        # ... and the whole list is jnn_pa with these thresholds, as is the read run on its own
        e = _want(oracle, x, POLYA._replace(top=float(top[r]), bot=float(bot[r])))
        assert segs[r] == e and int(ns[r]) == len(e)
        alone, _, _ = _run(gpu, [x], POLYA, top=[top[r]], bot=[bot[r]])
        assert alone[0] == segs[r]
    assert found >= 2


def test_gaps_and_residues(gpu, oracle, synth_pa):
    """the same batch with its gaps filled with NaN, 3e38 and 0.0 -- in-range, out-of-range and unordered neighbours --
    gives the same segments; every offsets[r] mod 4, a first read at element 1, the last read flush against n_values"""
    from sigtk_amd import device
    cat = {k.name: k for k in J.catalogue()}
    arrays = [cat[n].raw.astype(F) for n in ("rich_511", "rich_512", "rich_513", "lanes_49_50", "rich_5000_seed4",
                                                   "rich_16384")] + synth_pa[4:7]   # (16 384 positions: the last mask row kept in LDS)
    leads = [1] + [(r * 7 + 3) % 5 for r in range(1, len(arrays))]
    leads[-1] += 2
    p = J.PRESET[0]
    got = []
    for fill in (np.nan, 3e38, 0.0, 500.0):
        fb = device.upload_float_reads(arrays, _dev(), leads=leads, fill=fill)
        assert int(fb.offsets_host[0]) == 1 and set((fb.offsets_host.astype(np.int64) % 4).tolist()) == {0, 1, 2, 3}
        assert int(fb.offsets_host[-1]) + int(fb.lengths_host[-1]) == fb.n_values == fb.x.numel()
        got.append(_run(gpu, arrays, p, fb=fb)[0])
    assert got[0] == got[1] == got[2] == got[3]
    for r, x in enumerate(arrays):
        assert got[0][r] == _want(oracle, x, p), r
    # every read at every residue
    for res in range(4):
        _compare(gpu, oracle, arrays, p, "residue %d" % res, leads=[res] + [(-a.size) % 4 for a in arrays[:-1]], fill=500.0)


def test_caller_sized_slots(gpu, oracle):
    """slot ranges of the caller's choosing, as sgk_jnn_param reports them: n_segs is the true count, the surplus is
    dropped, the reads that overflowed are counted, and the neighbours' segments are right; a range that holds the
    segments but not the chunked form's staging is still right (the literal loop redoes the read)"""
    cat = {k.name: k for k in J.catalogue()}
    mid = cat["rich_5000_seed4"].raw.astype(F)
    arrays = [cat["lanes_49_50"].raw.astype(F), mid, cat["rich_16384"].raw.astype(F)]
    p = J.PRESET[0]
    want = [_want(oracle, x, p) for x in arrays]
    nseg = len(want[1])
    assert nseg >= 3
    full = [a.size // 32 + 2 for a in arrays]
    for cap in (2 * nseg - 1, nseg, nseg - 1, 1, 0):
        caps = [full[0], cap, full[2]]
        slots = np.concatenate([[0], np.cumsum(caps)])
        segs, ns, nerr = _run(gpu, arrays, p, slots=slots, leads=[0, 1, 2])
        k = min(cap, nseg)
        assert [int(v) for v in ns] == [len(w) for w in want], cap
        assert segs[0] == want[0] and segs[2] == want[2], cap
        assert segs[1] == want[1][:k], cap
        assert nerr == (1 if cap < nseg else 0), cap
