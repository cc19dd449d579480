"""GPU parity: reads that several wavefronts share (segments), against the oracle (bit-exact).

A read of at least `long_min` samples is cut into segments of `seg_len` samples; each segment's detector starts
speculatively in front of the segment, k_event_seam compares the states at the seams (and runs a segment again when
its speculation failed), replays the long-detector runs that cross a seam, and k_event_build_seg builds the events
per segment.  the segment_len / long_min options (api.event_configure) shrinks the segments so that ordinary test reads have hundreds of seams, and
shortens the speculative warm-up so that speculation does fail.  Results must not depend on any of it.
"""
import numpy as np
import pytest

from test_gpu_event import _check_events

pytestmark = pytest.mark.gpu


@pytest.fixture()
def configure(gpu):
    def f(seg, lmin, lead=0):
        gpu.event_configure(seg, lmin, lead)
    yield f
    gpu.event_configure(0, 0, 0)


@pytest.mark.parametrize("rna", [0, 1])
def test_long_reads_default_segments(gpu, oracle, rna):
    lens = [700000, 300000, 262144, 262143, 100000, 50, 3000001]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=21 + rna, kind=rna)
    got, st = gpu.event(reads, dig, off, rng, rna)
    _check_events(oracle, reads, dig, off, rng, rna, got)
    # (a batch this small: reads from 131 072 samples on are cut into segments of 65 536, event_plan.hip: event_config_for; and it
    # is a partial round of waves: the tail split cuts the 100 000-sample read as well, into segments of 82 944 samples =
    # ceil(mean / 8) rounded up to 1024)
    assert st.n_split_reads == 6 and st.n_segments == 11 + 5 + 4 + 4 + 2 + 46
    assert st.n_capacity_overflow == 0 and st.n_fallback_reads == 0
    assert st.n_events_total == sum(g.start.size for g in got)


@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("seg,lmin", [(1024, 1025), (4096, 10000), (2048, 2049)])
def test_small_segments_on_the_fixture(gpu, oracle, sp1, configure, rna, seg, lmin):
    recs = sp1.reads[:60]
    reads = [r.raw for r in recs]
    dig = np.array([r.digitisation for r in recs]); off = np.array([r.offset for r in recs])
    rng = np.array([r.range for r in recs])
    configure(seg, lmin)
    got, st = gpu.event(reads, dig, off, rng, rna)
    _check_events(oracle, reads, dig, off, rng, rna, got)
    nlong = sum(1 for r in reads if r.size >= lmin)
    assert st.n_split_reads == nlong and st.n_segments == sum(-(-r.size // seg) for r in reads if r.size >= lmin)


@pytest.mark.parametrize("rna", [0, 1])
def test_failed_speculation_at_seams_is_rerun(gpu, oracle, configure, rna):
    """a 16-sample warm-up is too short for the automaton to converge: many seams (and chunk boundaries) disagree and
    their segments are run again from the true state, some of them in a chain"""
    lens = [40000, 33333, 2049, 2048, 4097, 100000, 12345, 20480]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=5 + rna, kind=rna)
    configure(2048, 2049, 16)
    got, st = gpu.event(reads, dig, off, rng, rna)
    _check_events(oracle, reads, dig, off, rng, rna, got)
    assert st.n_seam_reruns > 0 and st.n_rerun_passes > 0
    configure(1024, 1025, 32)
    got, st = gpu.event(reads, dig, off, rng, rna)
    _check_events(oracle, reads, dig, off, rng, rna, got)


def test_edge_signals_in_segments(gpu, oracle, configure):
    """constant stretches (hot long-detector runs that cross seams, events longer than a segment), dense boundaries,
    a read that fails the exactness guard in one segment only, full-range noise"""
    rs = np.random.RandomState(3)
    n = 30000
    const = np.full(n, 500, dtype=np.int16)
    steps = np.repeat(rs.randint(300, 700, size=n // 10), 10).astype(np.int16)
    noise = rs.randint(-32768, 32767, size=n).astype(np.int16)
    tiny = (rs.randint(400, 600, size=n)).astype(np.int16)
    tiny[20001] = -9
    zeros = np.zeros(n, dtype=np.int16)
    dense = (np.repeat(np.tile([420, 610], n // 6 + 1), 3)[:n] + rs.randint(-2, 3, size=n)).astype(np.int16)
    # long flat stretches between bursts: events that span several segments
    flat = np.full(n, 480, dtype=np.int16)
    for p in (100, 9000, 9003, 25000):
        flat[p:p + 40] = rs.randint(300, 700, size=40)
    ramp = (400 + (np.arange(n) // 1500) * 7 + rs.randint(-3, 4, size=n)).astype(np.int16)
    reads = [const, steps, noise, tiny, zeros, dense, flat, ramp]
    R = len(reads)
    dig = np.full(R, 8192.0); off = np.array([10.0, 3.0, 0.0, 11.0, 0.0, 5.0, 6.0, 2.0]); rng = np.full(R, 1402.882324)
    for seg, lmin, lead in ((1024, 1025, 0), (3072, 3073, 0), (2048, 2049, 16)):
        configure(seg, lmin, lead)
        for rna in (0, 1):
            got, st = gpu.event(reads, dig, off, rng, rna)
            _check_events(oracle, reads, dig, off, rng, rna, got)
            assert st.n_fallback_reads >= 1


def test_segments_device_api_layouts_and_capacity(gpu, oracle, configure):
    """odd alignment (no fast path: the read's segments decline and the read takes the exact fallback), too few slots"""
    from test_gpu_device_api import _run_layout
    configure(2048, 2049)
    reads, _, _, _ = gpu.synth_reads_host(3, [30000, 20000, 25000], seed=31, kind=0)
    offsets = [0, 30001, 50008]
    b, arena = _run_layout(gpu, oracle, reads, offsets, 75016, 0)
    st = arena.status()
    assert st.n_split_reads == 3 and st.n_fallback_reads >= 1 and st.n_capacity_overflow == 0
    for r, raw in enumerate(reads):
        exp = oracle.event_raw(raw, 8192.0, 7.0, 1402.882324, 0)
        got = arena.read_events(r)
        assert got.start.size == exp.start.size, "read %d" % r
        assert np.array_equal(got.start.astype(np.uint64), exp.start)
        assert np.array_equal(got.mean.view(np.uint32), exp.mean.view(np.uint32))
        assert np.array_equal(got.stdv.view(np.uint32), exp.stdv.view(np.uint32))
    b, arena = _run_layout(gpu, oracle, reads[:2], [256, 256 + 30016], 256 + 30016 + 20000 + 320, 0,
                           slots_for=lambda n: 100)
    st = arena.status()
    assert st.n_capacity_overflow == 2
    exp = oracle.event_raw(reads[0], 8192.0, 7.0, 1402.882324, 0)
    assert int(arena.n_events[0].item()) == exp.start.size
    got = arena.read_events(0)
    assert np.array_equal(got.start[:100].astype(np.uint64), exp.start[:100])


@pytest.mark.parametrize("name,seg,lmin", [("soak_seed41_b3403_r1243.npz", 0, 0), ("soak_seed41_b4551_r8.npz", 2048, 7101),
                                            ("soak_seed41_b4551_r8.npz", 0, 0)])
def test_soak_regression_run_start_behind_the_mask(gpu, oracle, configure, name, seg, lmin):
    """seed 41, batches 3403 (read 1243, 200 samples) and 4551 (read 8, 16 557 samples) of tests/soak_parity.py with a
    16-sample warm-up, RNA parameters: a lane whose speculation failed takes its start state from the lane in front.
    The state carried the index of the long detector's last reset but (normalised) not the mask that reset had set, so
    a hot run that was open at the hand-over was replayed from the reset -- through indices the reference's long
    detector never saw (a statistic of 9.47 two indices before the mask ended became a boundary).  The state now
    carries the first index of the run.  With the presets' warm-ups a lane is re-run about once per 10^5 chunk
    boundaries, which is why 11 million soak reads had not met it."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    raw = z["samples"].astype(np.int16)
    dig, off, rng = z["dig"], z["off"], z["rng"]
    configure(seg, lmin, 16)
    for rna in (1, 0):
        got, st = gpu.event([raw], dig, off, rng, rna)
        _check_events(oracle, [raw], dig, off, rng, rna, got)
        assert st.n_rerun_passes > 0 or rna == 0


def test_flat_signal_costs_no_more_than_its_length(gpu, oracle, configure):
    """seed 41, batch 1310, read 21 of tests/soak_parity.py: a constant read (raw 254, offset 0) of 75 651 samples with
    RNA parameters.  The short detector enters a peak near the read's start that nothing ever emits; while the owner
    of a pending peak had to run on until it was emitted, every pass of every lane walked to the end of the read: 5 s in
    one wavefront, 150 s as 37 segments (every segment of a flat read is re-run: its long detector's run started at
    the read's first index, which no speculative start can know)."""
    import time
    flat = np.full(75651, 254, dtype=np.int16)
    other = np.full(33932, 174, dtype=np.int16)
    reads = [flat, other]
    dig = np.full(2, 8192.0); off = np.array([0.0, 13.0]); rng = np.array([1402.882324, -1402.882324])
    gpu.event([flat[:4000]], dig[:1], off[:1], rng[:1], 1)   # (first call of the process: module load)
    for seg, lmin in ((0, 0), (2048, 3287)):
        configure(seg, lmin)
        for rna in (1, 0):
            t0 = time.time()
            got, st = gpu.event(reads, dig, off, rng, rna)
            dt = time.time() - t0
            _check_events(oracle, reads, dig, off, rng, rna, got)
            assert dt < 2.0, "flat reads took %.1f s (segments %d / %d, rna %d)" % (dt, seg, lmin, rna)


@pytest.mark.parametrize("rna", [0, 1])
def test_tail_split_rule_is_no_cliff(gpu, rna):
    """VERDICT r04 task 8b: the tail split (event_plan.hip: event_tail_plan -- the reads of a batch's last, partial round of
    wavefronts are cut into segments iff the batch is at most 0.55 of a round, or that round at most a quarter of a round
    behind one full round, a sixth behind more) is a measured choice (tools/tail_sweep.py ->
    profiles/r05_tail_split_sweep.txt).  Either side of every cut the batch is timed with and without the split: what the
    rule picks may be at most 1.10 x the other (+ 30 us).  The events are the same either way (test_gpu_device_api.py,
    the soaks); this guards the rule against a kernel change that moves the cross-over -- its first run found the round's
    first rule (a third / a sixth) 25 % slower than the other choice on batches of 1 100 - 1 600 reads.
    RNA preset (two waves per SIMD): a batch of at most 7 / 8 of a round is cut, and no read behind a full round."""
    import torch
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    # wave slots: 256 CUs x 4 SIMDs x 3 waves with the DNA preset (k_event<3, short>: 168 registers), x 2 with the RNA preset
    slots = 2048 if rna else 3072
    if rna:
        sizes, want = (slots * 7 // 8 - 40, slots * 7 // 8 + 60, slots + slots // 8, 3 * slots + slots // 8), ["split", "whole", "whole", "whole"]
    else:
        sizes = (slots * 11 // 20 - 40, slots * 11 // 20 + 60, slots + slots // 4 - 12, slots + slots // 4 + 40,
                 3 * slots + slots // 6 - 12, 3 * slots + slots // 6 + 40)
        want = ["split", "whole"] * 3

    def timed(b, tail):
        old = gpu.EVENT_OPTIONS.tail_split
        gpu.EVENT_OPTIONS.tail_split = tail
        try:
            arena = device.EventArena(b)
        finally:
            gpu.EVENT_OPTIONS.tail_split = old
        for _ in range(3):
            device.event(b, arena, rna)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); device.event(b, arena, rna); e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    report = []
    for n in sizes:
        b = device.synth_reads(n, 100000, seed=9, kind=rna, device=dev)
        plan = gpu.event_plan(n, b.total_samples, 100000, rna)
        split = plan.tail_segment_len != 0
        rem = n % slots
        t_off, t_on = timed(b, -1), timed(b, rem)
        t_rule, t_other = (t_on, t_off) if split else (t_off, t_on)
        report.append((n, "split" if split else "whole", round(t_on, 3), round(t_off, 3)))
        assert t_rule <= 1.10 * t_other + 0.03, report
        del b
        torch.cuda.empty_cache()
    assert [r[1] for r in report] == want, report
    print(report)


def test_long_read_threshold_is_no_cliff(gpu):
    """From what length on a read is shared by several wavefronts follows the batch (event_plan.hip: event_config_for): 262 144
    samples (segments of 131 072) in a batch of 10^9 samples, 131 072 (65 536) in one of 3 x 10^8.  Both geometries are
    timed on both kinds of batch: what the rule picks may be at most 1.10 x the other (+ 30 us)."""
    import torch
    from sigtk_amd import device
    dev = torch.device("cuda", 0)

    def timed(b, seg, lmin):
        o = gpu.EVENT_OPTIONS
        old = (o.segment_len, o.long_min)
        o.segment_len, o.long_min = seg, lmin
        try:
            arena = device.EventArena(b)
        finally:
            o.segment_len, o.long_min = old
        for _ in range(3):
            device.event(b, arena, 0)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); device.event(b, arena, 0); e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    rs = np.random.RandomState(5)
    ragged = np.clip(100000 * np.exp(rs.normal(-0.32, 0.8, size=10000)), 200, 1600000).astype(np.int64)
    few_long = np.full(3016, 100000, dtype=np.int64)
    few_long[:16] = 250000
    report = []
    for name, lens, want in (("10 000 log-normal reads", ragged, 262144), ("3 000 reads + 16 of 250 000", few_long, 131072),
                             ("3 000 log-normal reads", ragged[:3000], 131072)):
        b = device.synth_reads(len(lens), 100000, seed=13, kind=0, device=dev, lengths=lens)
        plan = gpu.event_plan(len(lens), b.total_samples, int(lens.max()), 0)
        t_rule = timed(b, 0, 0)
        other = (65536, 131072) if plan.long_min > 200000 else (131072, 262144)
        t_other = timed(b, *other)
        report.append((name, plan.long_min, round(t_rule, 3), round(t_other, 3)))
        assert abs(int(plan.long_min) - want) <= 8192, report
        assert t_rule <= 1.10 * t_other + 0.03, report
        del b
        torch.cuda.empty_cache()
    print(report)
