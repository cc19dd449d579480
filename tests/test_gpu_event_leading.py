"""GPU parity of the leading-edge form of the fast detector pass (csrc/event_detect.h: LazyPass<.., LEAD>), which
k_event takes for the DNA preset: the short window's sums are formed W1 steps early and ringed as floats, the A sides
wait in a ring twice as deep, and the long detector's bound is formed from the f32 sums of the long window's two
halves (tstat_math.h: sgk_lside_halves).  What can go wrong is the rings at a pass' start -- the read's first indices,
every chunk start, every re-run from a snapshot -- and the bound on signals whose window halves have opposite signs.

Everything is compared with the oracle bit for bit (start, length, mean, stdv); there are no tolerances.  The path is
pinned with the event options so that k_event, one wavefront per read, runs (not the packed kernel, not segments); both
presets and both input types run, so the instances that keep the trailing form are held to the same reads."""
import numpy as np
import pytest

import event_cases as E
from test_gpu_event_cases import _event_pa, options  # noqa: F401  (options: a fixture)

pytestmark = pytest.mark.gpu

WHOLE = dict(lanes_per_short_read=-1, tail_split=-1)
#: every length up to 80 (the read's first and last W1 / W2 indices meet; chunks of 16 samples from 1 024 / 64 on), the
#: edges of the 16-step block, of the 32- and 128-sample loads, of a segment, and a read with many chunk starts
LENGTHS = list(range(1, 81)) + [95, 96, 97, 127, 128, 129, 1023, 1024, 1025, 5000]


def _same(g, exp):
    return g.start.size == exp.start.size and np.array_equal(g.start.astype(np.uint64), exp.start) and \
        np.array_equal(g.length.astype(np.float32), exp.length) and \
        np.array_equal(g.mean.view(np.uint32), exp.mean.view(np.uint32)) and np.array_equal(g.stdv.view(np.uint32), exp.stdv.view(np.uint32))


class _Expected:
    """the oracle's events, once per (read, scaling, preset) for the whole module"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def raw(self, raw, scale, rna):
        key = (raw.tobytes(), tuple(float(v) for v in scale), rna)
        if key not in self.memo:
            self.memo[key] = self.oracle.event_raw(raw, *scale, rna)
        return self.memo[key]

    def pa(self, pa, rna):
        key = (pa.tobytes(), "pa", rna)
        if key not in self.memo:
            self.memo[key] = self.oracle.getevents(pa, rna)
        return self.memo[key]


@pytest.fixture(scope="module")
def expected(oracle):
    return _Expected(oracle)


@pytest.fixture(scope="module")
def length_reads(gpu):
    reads, _, _, _ = gpu.synth_reads_host(len(LENGTHS), LENGTHS, seed=57, kind=0)
    return [r.astype(np.int16) for r in reads]


def _run_raw(gpu, reads, scale, rna):
    n = len(reads)
    return gpu.event(reads, *(np.full(n, v) for v in scale), rna)


def _whole_path(gpu, reads, rna, st):
    assert st.n_split_reads == 0 and st.n_capacity_overflow == 0
    plan = gpu.event_plan(len(reads), sum(r.size for r in reads), max(r.size for r in reads), rna)
    assert plan.lanes_per_short_read == 0


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
def test_every_short_length(gpu, oracle, options, expected, length_reads, rna, as_pa):
    """one read per call (lane 0 alone, then a few lanes, then chunks of 16 .. 80 samples), and all of them as one batch"""
    options(**WHOLE)
    failures = []
    pas = [oracle.pa(r, *E.SCALE) for r in length_reads]
    for raw, pa in zip(length_reads, pas):
        if as_pa:
            got, st = _event_pa(gpu, [pa], rna)
            exp = expected.pa(pa, rna)
        else:
            got, st = _run_raw(gpu, [raw], E.SCALE, rna)
            exp = expected.raw(raw, E.SCALE, rna)
        _whole_path(gpu, [raw], rna, st)
        if not _same(got[0], exp) or st.n_fallback_reads != 0:
            failures.append("alone n=%d: gpu starts %r oracle %r, %d fallback reads" % (raw.size, got[0].start[:8].tolist(),
                                                                                      exp.start[:8].tolist(), st.n_fallback_reads))
    got, st = _event_pa(gpu, pas, rna) if as_pa else _run_raw(gpu, length_reads, E.SCALE, rna)
    _whole_path(gpu, length_reads, rna, st)
    for raw, pa, g in zip(length_reads, pas, got):
        if not _same(g, expected.pa(pa, rna) if as_pa else expected.raw(raw, E.SCALE, rna)):
            failures.append("batch n=%d: gpu starts %r" % (raw.size, g.start[:8].tolist()))
    assert not failures, "\n".join(failures[:20])
    assert st.n_fallback_reads == 0


def _noise_steps(seed, n, amp=6):
    """levels that change every 5 .. 40 samples, with noise: pA of 40 .. 150 under the catalogue's scaling"""
    rs = np.random.RandomState(seed)
    out = []
    while sum(len(p) for p in out) < n:
        out.append(rs.randint(260, 840) + rs.randint(-amp, amp + 1, size=rs.randint(5, 41)))
    return np.concatenate(out)[:n].astype(np.int16)


def _flat_then_step(n=3000):
    """flat stretches, each followed by a step: the shape on which the long detector emits (event_cases.flat / sig)"""
    rs = np.random.RandomState(9)
    parts, level = [], 500
    while sum(len(p) for p in parts) < n:
        parts.append(E.flat(int(rs.randint(20, 120)), level))
        level = int(np.clip(level + rs.choice([-1, 1]) * rs.randint(2, 60), 300, 800))
        parts.append(level + rs.randint(-1, 2, size=int(rs.randint(3, 30))))
    return np.concatenate([np.asarray(p) for p in parts])[:n].astype(np.int16)


def _sign_patterns(pa, rna):
    """{name: pA}: the same magnitudes with signs that put the halves of long windows on opposite sides of zero"""
    w1 = E.PRESET[rna].w1
    idx = np.arange(pa.size)
    rs = np.random.RandomState(77)
    blocks = np.repeat(rs.choice([-1.0, 1.0], size=pa.size // 5 + 1), 5)[:pa.size]
    return {"negated": -pa,
            "halves_w1": np.where((idx // w1) % 2 == 0, pa, -pa),          # every long window: one half +, one half -
            "halves_w1_shifted": np.where(((idx + 1) // w1) % 2 == 0, pa, -pa),
            "alternating": np.where(idx % 2 == 0, pa, -pa),
            "blocks_of_5": pa * blocks,
            "one_crossing": np.where(idx < pa.size // 2, pa, -pa)}


@pytest.mark.parametrize("rna", [0, 1])
def test_halves_of_opposite_sign_pa(gpu, oracle, options, expected, rna):
    """float pA input: magnitudes of 40 .. 150 pA with either sign pass the exactness guard, so these reads stay on the fast
    pass; |S1| + |S2| of a long window is then far larger than |S1 + S2| -- the term the re-proved bound charges to the
    sums of squares"""
    options(**WHOLE)
    names, pas = [], []
    for base_name, raw in (("noise_steps", _noise_steps(3, 4000)), ("flat_then_step", _flat_then_step()),
                           ("constant", np.full(2000, 640, dtype=np.int16))):
        pa = oracle.pa(raw, *E.SCALE)
        for name, x in _sign_patterns(pa, rna).items():
            names.append(base_name + ":" + name)
            pas.append(np.ascontiguousarray(x, dtype=np.float32))
    got, st = _event_pa(gpu, pas, rna)
    print("leading: opposite signs rna %d: n_fallback_reads %d n_long_replays %d n_replay_indices %d" % (
        rna, st.n_fallback_reads, st.n_long_replays, st.n_replay_indices))
    bad = [n for n, x, g in zip(names, pas, got) if not _same(g, expected.pa(x, rna))]
    assert not bad, bad
    assert st.n_split_reads == 0 and st.n_capacity_overflow == 0
    # only the constant reads (too many hot runs for a lane's records) may leave the fast path
    assert st.n_fallback_reads <= sum(1 for n in names if n.startswith("constant"))


@pytest.mark.parametrize("rna", [0, 1])
def test_negative_offset_constant_and_steps_int16(gpu, options, expected, rna):
    """int16 input: an offset that puts zero pA inside the read's range (such a read fails the guard and is redone by the
    fallback kernel -- after the fast pass ran on it), one that makes every sample negative, a constant read, flat
    stretches followed by steps"""
    options(**WHOLE)
    dig, rng = E.SCALE[0], E.SCALE[2]
    cases = [("crossing_zero", _noise_steps(4, 4000), (dig, -550.0, rng)),
             ("all_negative", _noise_steps(5, 4000), (dig, -1200.0, rng)),
             ("constant", np.full(3000, 512, dtype=np.int16), E.SCALE),
             ("constant_negative", np.full(3000, 512, dtype=np.int16), (dig, -1000.0, rng)),
             ("flat_then_step", _flat_then_step(), E.SCALE),
             ("flat_then_step_negative", _flat_then_step(), (dig, -1300.0, rng))]
    bad = []
    for name, raw, scale in cases:
        got, st = _run_raw(gpu, [raw], scale, rna)
        print("leading: %-24s rna %d: n_fallback_reads %d n_long_replays %d" % (name, rna, st.n_fallback_reads, st.n_long_replays))
        if not _same(got[0], expected.raw(raw, scale, rna)):
            bad.append(name)
        if name == "all_negative":
            assert st.n_fallback_reads == 0     # same sign: the fast pass' result is the one that is kept
    assert not bad, bad


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
def test_magnitudes_at_both_ends_of_the_guard(gpu, oracle, options, expected, rna, as_pa):
    """|pA| from 2^-19 and up to 2^19.2: the guard takes non-zero magnitudes in [2^-20, 2^20]"""
    options(**WHOLE)
    raw = np.concatenate([_noise_steps(6, 2500), _flat_then_step(1500)])
    bad = []
    for k in (-25, 12):
        scale = (E.SCALE[0], E.SCALE[1], float(np.float32(E.SCALE[2]) * np.float32(2.0) ** k))
        if as_pa:
            pa = oracle.pa(raw, *scale)
            assert (2.0 ** -20 <= np.abs(pa).min()) and (np.abs(pa).max() < 2.0 ** 20)
            got, st = _event_pa(gpu, [pa], rna)
            exp = expected.pa(pa, rna)
        else:
            got, st = _run_raw(gpu, [raw], scale, rna)
            exp = expected.raw(raw, scale, rna)
        if not _same(got[0], exp) or st.n_fallback_reads != 0:
            bad.append("2^%d: %d events, oracle %d, %d fallback reads" % (k, got[0].start.size, exp.start.size, st.n_fallback_reads))
    assert not bad, bad


@pytest.mark.parametrize("rna", [0, 1])
def test_reruns_from_a_snapshot(gpu, options, expected, rna):
    """warm-ups of 16 and 32 samples, too short for the automaton to converge at every chunk start: chunks whose
    speculation failed are run again from the state the chunk in front ended with -- the rings are initialised at the chunk
    start with no warm-up, the detector state (the long detector's mask and run start with it) comes from the snapshot"""
    lens = [20000] + [int(v) for v in np.random.RandomState(11).randint(3000, 6001, size=64)]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=40 + rna, kind=rna)
    reruns = {}
    for warmup in (16, 32):
        options(warmup=warmup, **WHOLE)
        for what, sel in (("one read of 20 000", slice(0, 1)), ("64 reads of 3 000 - 6 000", slice(1, None))):
            rr = reads[sel]
            got, st = gpu.event(rr, dig[sel], off[sel], rng[sel], rna)
            print("leading: re-runs, %s, warm-up %d, rna %d: n_rerun_passes %d n_fallback_reads %d" % (
                what, warmup, rna, st.n_rerun_passes, st.n_fallback_reads))
            bad = [r for r, (raw, g) in enumerate(zip(rr, got))
                   if not _same(g, expected.raw(raw, (dig[sel][r], off[sel][r], rng[sel][r]), rna))]
            assert not bad, (what, warmup, bad)
            assert st.n_split_reads == 0 and st.n_capacity_overflow == 0
            reruns[what] = reruns.get(what, 0) + int(st.n_rerun_passes)
    # the test must not pass without the snapshot path: both the single read and the batch took it
    assert all(v > 0 for v in reruns.values()), reruns
