"""GPU parity: the boundaries the LONG detector emits, on every path of `event`.

The reads are the hand-made catalogue of tests/event_cases.py (tests/test_event_cases_cpu.py proves that every branch of the
reference's peak detector and every special place of the lazy long detector -- chunk ends, warm-ups, seams, the lanes' run
records, the bitmap ring -- is taken by one of them; tests/test_oracle_vs_ref.py that the oracle equals the real reference
on them).  On the GPU the long detector is never stepped: it is proven silent from bounds, and where the proof fails the
run is recorded and replayed after the pass (event_detect.h).  Nothing else in the suite holds a read on which that replay
has a boundary to emit.  Everything here is compared with the ORACLE by _check_events: starts, lengths, mean and stdv bit
for bit; there are no tolerances and no timing.  Each test prints the counters of the status word (pytest -s)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import event_cases as E
from test_gpu_event import _check_events

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: the BLOW5 headers the CLI picks the preset by (as tests/golden/make_golden_event_cases.py wrote them)
HEADERS = {"dna": {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"},
           "rna": {"experiment_type": "rna", "sequencing_kit": "sqk-rna002"}}
TINY = int(1 - E.SCALE[1])         # raw + offset == 1: |pA| = 0.17, the read fails the exactness guard


class _Memo:
    """the oracle's events, computed once per read and preset for the whole module (what _check_events asks for)"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def event_raw(self, raw, dig, off, rng, rna):
        key = (hashlib.sha1(np.ascontiguousarray(raw, dtype=np.int16).tobytes()).digest(), float(dig), float(off), float(rng), int(rna))
        if key not in self.memo:
            self.memo[key] = self.oracle.event_raw(raw, dig, off, rng, rna)
        return self.memo[key]


@pytest.fixture(scope="module")
def cat():
    return E.catalogue()


@pytest.fixture(scope="module")
def memo(oracle, cat):
    m = _Memo(oracle)
    for k in cat:
        for _, rna in E.case_runs(k):
            m.event_raw(k.raw, *E.SCALE, rna)
    return m


@pytest.fixture(scope="module")
def longs(cat):
    """{run label: the boundaries the model attributes to the long detector}"""
    return E.tag_table(cat)[1]


@pytest.fixture()
def options(gpu):
    """sets fields of gpu.EVENT_OPTIONS for the calls that follow; the defaults come back afterwards"""
    o = gpu.EVENT_OPTIONS
    names = ("segment_len", "long_min", "warmup", "lanes_per_short_read", "short_max", "tail_split")
    saved = [getattr(o, f) for f in names]

    def f(**kw):
        for name, v in zip(names, saved):
            setattr(o, name, v)
        for name, v in kw.items():
            assert name in names
            setattr(o, name, int(v))
    yield f
    for name, v in zip(names, saved):
        setattr(o, name, v)


def _scal(n):
    return tuple(np.full(n, v) for v in E.SCALE)


def _batch(cat, rna):
    cases = [k for k in cat if rna in k.rna]
    return cases, [k.raw for k in cases]


def _compare(memo, names, reads, rna, got, what):
    """read by read, so that a failure names the read; all of them are reported"""
    failures = []
    for r, (name, raw) in enumerate(zip(names, reads)):
        try:
            _check_events(memo, [raw], [E.SCALE[0]], [E.SCALE[1]], [E.SCALE[2]], rna, [got[r]])
        except AssertionError as e:
            failures.append("%s rna %d %s (n=%d): %s" % (what, rna, name, raw.size, str(e).strip().split("\n")[0][:200]))
    assert not failures, "\n".join(failures)


def _report(what, rna, st, n_long_reads):
    print("event_cases %-28s rna %d: %3d reads with a long-detector boundary, n_long_replays %d n_replay_indices %d "
          "n_fallback_reads %d n_split_reads %d n_rerun_passes %d" % (what, rna, n_long_reads, st.n_long_replays, st.n_replay_indices,
                                                                      st.n_fallback_reads, st.n_split_reads, st.n_rerun_passes))


#: every path of sgk_event: the defaults; one wavefront per read; `lanes` lanes per read (at 4 and 16 also with a warm-up of
#: 16 samples, after which speculation fails; short_max above the longest read: a batch without a dispatch order is packed
#: only if every read is short); segments; the tail split on every read
CONFIGS = {"default": {}, "whole": dict(lanes_per_short_read=-1, tail_split=-1)}
for _l in (1, 2, 4, 8, 16, 32):
    CONFIGS["packed%d" % _l] = dict(lanes_per_short_read=_l, tail_split=-1, short_max=65536)
for _l in (4, 16):
    CONFIGS["packed%d_warmup16" % _l] = dict(lanes_per_short_read=_l, tail_split=-1, short_max=65536, warmup=16)
for _seg, _lmin, _lead in ((1024, 1025, 0), (3072, 3073, 0), (2048, 2049, 16)):
    CONFIGS["segments%d_warmup%d" % (_seg, _lead)] = dict(segment_len=_seg, long_min=_lmin, warmup=_lead)
CONFIGS["tail_split_all"] = dict(tail_split="n")


@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_whole_catalogue(gpu, memo, cat, longs, options, config, rna):
    cases, reads = _batch(cat, rna)
    kw = dict(CONFIGS[config])
    if kw.get("tail_split") == "n":
        kw["tail_split"] = len(reads)
    options(**kw)
    got, st = gpu.event(reads, *_scal(len(reads)), rna)
    n_long = sum(1 for k in cases if longs["%s/rna%d" % (k.name, rna)])
    _report(config, rna, st, n_long)
    _compare(memo, [k.name for k in cases], reads, rna, got, config)
    assert st.n_capacity_overflow == 0
    assert st.n_events_total == sum(g.start.size for g in got)
    # the batch holds dozens of reads with a long-detector boundary that no rule sends to the fallback
    assert n_long >= 25 and st.n_long_replays > 0 and st.n_replay_indices > 0
    if config.startswith("segments"):
        lmin = CONFIGS[config]["long_min"]
        assert st.n_split_reads == sum(1 for r in reads if r.size >= lmin)


@pytest.mark.parametrize("rna", [0, 1])
def test_long_reads_in_noise_stay_on_the_fast_path(gpu, memo, cat, longs, options, rna):
    """chunks of 512 - 640 samples with warm-ups of 32 / 64 (DNA) and 128 / 256 (RNA) either side of 32 768 samples: the
    reads with both seeds in noise have at most 4 certainly hot runs in a chunk (test_event_cases_cpu.py) and noise that
    the cold proof can take (event_cases.quiet_long), so a wavefront each takes them without the fallback"""
    cases = [k for k in cat if k.name in ("long_40000_quiet", "long_32767", "long_32768", "long_32769")]
    reads = [k.raw for k in cases]
    options(lanes_per_short_read=-1, tail_split=-1)
    got, st = gpu.event(reads, *_scal(len(reads)), rna)
    _report("long reads in noise, whole", rna, st, len(reads))
    _compare(memo, [k.name for k in cases], reads, rna, got, "whole")
    assert len(reads) == 4 and st.n_fallback_reads == 0 and st.n_split_reads == 0
    assert st.n_long_replays >= 20 and st.n_replay_indices > 0
    for k, g in zip(cases, got):
        want = longs["%s/rna%d" % (k.name, rna)]
        assert len(want) >= 20 and set(want) <= set(g.start.tolist()), k.name


@pytest.mark.parametrize("rna", [0, 1])
def test_tail_split_cuts_the_long_reads(gpu, memo, cat, longs, options, rna):
    """the tail split takes no batch whose reads are shorter than 32 768 samples on average (event_plan.hip: event_tail_plan), so
    on the whole catalogue tail_split = n changes nothing; the five reads from 32 767 samples on are cut, all of them"""
    cases = [k for k in cat if k.raw.size >= 32767]
    reads = [k.raw for k in cases]
    assert len(reads) == 5 and sum(r.size for r in reads) // 5 >= 32768
    options(tail_split=len(reads), lanes_per_short_read=-1)
    got, st = gpu.event(reads, *_scal(len(reads)), rna)
    _report("tail split, long reads", rna, st, sum(1 for k in cases if longs["%s/rna%d" % (k.name, rna)]))
    _compare(memo, [k.name for k in cases], reads, rna, got, "tail split")
    assert st.n_split_reads == 5 and st.n_capacity_overflow == 0 and st.n_long_replays > 0 and st.n_replay_indices > 0


@pytest.mark.parametrize("rna", [0, 1])
def test_the_boundaries_come_from_the_long_detector(gpu, memo, cat, longs, options, rna):
    """given parity this is implied -- but it is what a failure should show: per read, the boundaries the model
    attributes to the long detector that the GPU does not have"""
    cases, reads = _batch(cat, rna)
    options(lanes_per_short_read=-1, tail_split=-1)
    got, st = gpu.event(reads, *_scal(len(reads)), rna)
    missing, total = [], 0
    for k, g in zip(cases, got):
        want = longs["%s/rna%d" % (k.name, rna)]
        total += len(want)
        lost = sorted(set(want) - set(g.start.tolist()))
        if lost:
            missing.append("%s rna %d: long-detector boundaries %r of %r are missing" % (k.name, rna, lost[:8], want[:8]))
    assert total >= 80 and not missing, "\n".join(missing)


def test_too_many_hot_runs(gpu, memo, cat, options):
    """more than LZ_NREC = 8 hot runs end in one lane's chunk: the read goes to the exact fallback; with exactly 8 it stays
    on the fast path; packed between ordinary neighbours only that read falls back"""
    by_name = {k.name: k for k in cat}
    for rna, d in ((0, "d"), (1, "r")):
        over, eight = by_name["nrec_over_" + d].raw, by_name["nrec_8_" + d].raw
        options(lanes_per_short_read=-1, tail_split=-1)
        got, st = gpu.event([over], *_scal(1), rna)
        _report("nrec_over alone", rna, st, 0)
        _compare(memo, ["nrec_over_" + d], [over], rna, got, "alone")
        assert st.n_fallback_reads == 1
        got, st = gpu.event([eight], *_scal(1), rna)
        _report("nrec_8 alone", rna, st, 0)
        _compare(memo, ["nrec_8_" + d], [eight], rna, got, "alone")
        assert st.n_fallback_reads == 0 and st.n_long_replays > 0
        # packed: the chunks are longer (16 or 4 per read), the same plateaus are more than 8 runs in each.  The neighbours
        # are the seeds: fewer than 8 runs in all, so that no lane of theirs can meet more
        names = ["dna_seed", "rna_seed", "nrec_over_" + d, "seed_300_dna", "seed_300_rna"]
        reads = [by_name[n].raw for n in names]
        assert all(len(E.analyse(by_name[n].raw, rna)[2]["runs"]) <= E.LZ_NREC for n in names if n != "nrec_over_" + d)
        for lanes in (4, 16):
            options(lanes_per_short_read=lanes, tail_split=-1, short_max=32768)
            got, st = gpu.event(reads, *_scal(len(reads)), rna)
            _report("nrec_over packed%d" % lanes, rna, st, 2)
            _compare(memo, names, reads, rna, got, "packed%d" % lanes)
            assert st.n_fallback_reads == 1 and st.n_long_replays > 0


def _tiny_variants(raw, rna, boundary=2048):
    """a read with a long-detector boundary at `boundary`, with tiny-|pA| samples: one inside the run that emits it (as far
    from the boundary as the run allows), one 2 * w2 in front of the run, one 1500 samples in front of it, and 40 of them
    (the repair list holds 32: every index is then evaluated from the prefix arrays).  Each keeps the run's boundaries"""
    p = E.PRESET[rna]
    info = E.analyse(raw, rna)[2]
    run = next(r for r in info["runs"] if boundary in r.peaks)
    assert run.a > 1600
    inside = sorted(range(run.a, run.b), key=lambda i: -min(abs(i - q) for q in run.peaks))
    out = {}
    for name, places in (("inside", [[i] for i in inside]), ("front", [[run.a - 2 * p.w2]]), ("far", [[run.a - 1500]]),
                         ("all_dirty", [[run.a - 1500 + 9 * j for j in range(40)]])):
        for cand in places:
            x = raw.copy()
            x[cand] = TINY
            if set(run.peaks) <= set(E.analyse(x, rna)[2]["long"]):
                out[name] = x
                break
    return out, run


@pytest.mark.parametrize("rna", [0, 1])
def test_fallback_replays_long_boundaries_from_the_prefix_arrays(gpu, memo, cat, options, rna):
    """a read that fails the exactness guard takes the fallback kernel, whose replay of the hot runs reads the reference's
    sequential prefix arrays (FLAGGED): it must emit the same long-detector boundaries"""
    from test_gpu_device_api import _run_layout
    base = {k.name: k for k in cat}["seam+0_" + "dr"[rna]].raw
    variants, run = _tiny_variants(base, rna)
    assert sorted(variants) == ["all_dirty", "far", "front", "inside"], sorted(variants)
    names, reads = list(variants), list(variants.values())
    for config in ("default", "whole", "segments1024_warmup0"):
        options(**CONFIGS[config])
        got, st = gpu.event(reads, *_scal(len(reads)), rna)
        _report("tiny samples, " + config, rna, st, len(reads))
        _compare(memo, names, reads, rna, got, config)
        assert st.n_fallback_reads == len(reads)
        for name, g in zip(names, got):
            assert set(run.peaks) <= set(g.start.tolist()), "%s: long-detector boundaries %r missing" % (name, run.peaks)
    # the same reads and the clean one on odd sample offsets (no fast path for them), through the device API
    options()
    reads = [base] + reads
    offsets, o = [], 257
    for r in reads:
        offsets.append(o)
        o += r.size + 33 + (r.size + 33) % 2        # every read on an odd sample
    shifted = [r + np.int16(3) for r in reads]      # (_run_layout scales with offset 7, the catalogue with 10: the same pA)
    b, arena = _run_layout(gpu, memo.oracle, shifted, offsets, (o + 64 + 7) // 8 * 8, rna)
    st = arena.status()
    _report("tiny samples, odd offsets", rna, st, len(reads))
    assert st.n_fallback_reads == len(reads) and st.n_capacity_overflow == 0
    for r, raw in enumerate(reads):
        exp = memo.event_raw(raw, *E.SCALE, rna)
        got = arena.read_events(r)
        assert got.start.size == exp.start.size, "read %d" % r
        assert np.array_equal(got.start.astype(np.uint64), exp.start) and np.array_equal(got.length.astype(np.float32), exp.length)
        assert np.array_equal(got.mean.view(np.uint32), exp.mean.view(np.uint32))
        assert np.array_equal(got.stdv.view(np.uint32), exp.stdv.view(np.uint32))


#: the reads that were tuned for a place of the geometry
TUNED = ("dna_seed", "rna_seed", "seed_300_", "chunk_", "between_", "mask_pair_r", "decline_d_120", "decline_r_120", "row_smooth_61",
         "row_smooth_0", "dna_seed_cut", "rna_seed_cut", "len_13", "len_29")


@pytest.mark.parametrize("rna", [0, 1])
def test_every_sample_offset(gpu, memo, cat, longs, options, rna):
    """the tuned reads packed back to back behind fillers of odd lengths, each of them 16 times so that it starts at every
    sample offset modulo 16 (the lanes' chunks and the bitmap's 16-bit units are laid out from the read's first sample;
    the 32-byte loads are not).  Reads on even samples stay on the fast path, reads on odd ones take the fallback"""
    from test_gpu_device_api import _run_layout
    options(lanes_per_short_read=-1, tail_split=-1)
    pick = [k for k in cat if k.name.startswith(TUNED) and rna in k.rna]
    assert len(pick) >= 14 and sum(1 for k in pick if longs["%s/rna%d" % (k.name, rna)]) >= 8
    filler = E.train(5, 400, noise=2).astype(np.int16)
    reads, names, offsets, cur = [], [], [], 256
    for j in range(16):
        for i, k in enumerate(pick):
            flen = 301 + ((i + j) - (cur + 301)) % 16      # this copy starts at offset i + j (mod 16)
            for raw, name in ((filler[:flen], None), (k.raw, k.name)):
                reads.append(raw); names.append(name); offsets.append(cur)
                cur += raw.size
    starts = {}
    for name, o in zip(names, offsets):
        if name:
            starts.setdefault(name, set()).add(o % 16)
    assert all(v == set(range(16)) for v in starts.values())
    shifted = [r + np.int16(3) for r in reads]      # (_run_layout scales with offset 7, the catalogue with 10: the same pA)
    b, arena = _run_layout(gpu, memo.oracle, shifted, offsets, (cur + 64 + 7) // 8 * 8, rna)
    st = arena.status()
    _report("every sample offset", rna, st, 16 * sum(1 for k in pick if longs["%s/rna%d" % (k.name, rna)]))
    assert st.n_capacity_overflow == 0 and st.n_long_replays > 0
    assert st.n_fallback_reads == sum(1 for o, r in zip(offsets, reads) if o % 2 and r.size)
    failures = []
    for r, raw in enumerate(reads):
        exp = memo.event_raw(raw, *E.SCALE, rna)
        got = arena.read_events(r)
        same = got.start.size == exp.start.size and np.array_equal(got.start.astype(np.uint64), exp.start) and \
            np.array_equal(got.length.astype(np.float32), exp.length) and \
            np.array_equal(got.mean.view(np.uint32), exp.mean.view(np.uint32)) and np.array_equal(got.stdv.view(np.uint32), exp.stdv.view(np.uint32))
        if not same:
            failures.append("rna %d read %d (%s, n=%d, offset %d mod 16): gpu starts %r oracle %r" % (
                rna, r, names[r] or "filler", raw.size, offsets[r] % 16, got.start[:8].tolist(), exp.start[:8].tolist()))
    assert not failures, "\n".join(failures[:20])


def _event_pa(gpu, pas, rna):
    """sgk_event_pa_opt on pA arrays laid out like a batch of reads -> (list of Events, status)"""
    import ctypes as C
    import torch
    from sigtk_amd import device
    L = gpu.load_library()
    dev = torch.device("cuda", 0)
    b = device.alloc_reads(np.array([x.size for x in pas], dtype=np.int64), dev)
    host = np.zeros(b.n_samples, dtype=np.float32)
    for r, x in enumerate(pas):
        o = int(b.offsets_host[r])
        host[o:o + x.size] = x
    pa = torch.from_numpy(host).to(dev)
    assert pa.data_ptr() % 16 == 0
    arena = device.EventArena(b)
    gpu.check(L.sgk_event_pa_opt(pa.data_ptr(), b.offsets.data_ptr(), b.lengths.data_ptr(), b.n_reads, b.max_read_len, b.n_samples,
                                 int(rna), arena.slots.data_ptr(), arena.events.data_ptr(), arena.n_events.data_ptr(),
                                 arena.ws.data_ptr(), arena.ws_bytes, device._stream_ptr(), C.byref(arena.opt)), "sgk_event_pa_opt")
    torch.cuda.synchronize()
    return [arena.read_events(r) for r in range(len(pas))], arena.status()


@pytest.mark.parametrize("rna", [0, 1])
def test_event_pa(gpu, oracle, cat, longs, options, rna):
    """sgk_event_pa: the raw catalogue converted with oracle.pa, and what int16 cannot express -- a statistic that equals
    thr1 (as a peak's value: not above it), thr2 or peak_height (as the first rise: no peak), -0.0 samples"""
    cases, reads = _batch(cat, rna)
    pa_only = [k for k in E.pa_cases() if k.rna == rna]
    assert len(pa_only) == 4
    names = [k.name for k in cases] + ["pa:" + k.name for k in pa_only]
    pas = [oracle.pa(r, *E.SCALE) for r in reads] + [k.pa for k in pa_only]
    for config in ("default", "whole", "segments2048_warmup16"):
        options(**CONFIGS[config])
        got, st = _event_pa(gpu, pas, rna)
        _report("pA, " + config, rna, st, sum(1 for k in cases if longs["%s/rna%d" % (k.name, rna)]))
        failures = []
        for name, x, g in zip(names, pas, got):
            exp = oracle.getevents(x, rna)
            same = g.start.size == exp.start.size and np.array_equal(g.start.astype(np.uint64), exp.start) and \
                np.array_equal(g.length.astype(np.float32), exp.length) and \
                np.array_equal(g.mean.view(np.uint32), exp.mean.view(np.uint32)) and np.array_equal(g.stdv.view(np.uint32), exp.stdv.view(np.uint32))
            if not same:
                failures.append("%s rna %d %s (n=%d): gpu starts %r oracle %r" % (config, rna, name, x.size, g.start[:8].tolist(),
                                                                                 exp.start[:8].tolist()))
        assert not failures, "\n".join(failures)
        assert st.n_capacity_overflow == 0 and st.n_long_replays > 0 and st.n_replay_indices > 0


@pytest.mark.parametrize("lanes", [4, 32])
def test_neighbour_independence_in_a_packed_wave(gpu, memo, cat, options, lanes):
    """a 300-sample read whose hot run is open at n (and emits) next to a 16 000-sample read in the same wavefront: the short
    read's lanes step on past n for as long as the long one lasts, through whatever lies behind the read"""
    by_name = {k.name: k for k in cat}
    long_one = E.train(9, 16000, noise=2).astype(np.int16)     # (with noise: hot runs are rare, no lane meets more than 8)
    for rna in (0, 1):
        short = by_name["seed_300_" + ("dna", "rna")[rna]].raw
        assert short.size == 300 and E.G_RUN_AT_END_EMITS in E.analyse(short, rna)[1]
        assert len(E.analyse(short, rna)[2]["runs"]) <= E.LZ_NREC       # (the short read cannot overflow a lane's records)
        reads = [short, long_one] + [by_name["row_noise_1"].raw, short] * (32 // lanes - 1)
        names = ["seed_300", "long_16000"] + ["row_noise_1", "seed_300"] * (32 // lanes - 1)
        options(lanes_per_short_read=lanes, tail_split=-1, short_max=65536)
        got, st = gpu.event(reads, *_scal(len(reads)), rna)
        _report("neighbours packed%d" % lanes, rna, st, len(reads) // 2 + 1)
        _compare(memo, names, reads, rna, got, "packed%d" % lanes)
        assert st.n_fallback_reads <= 32 // lanes and st.n_long_replays > 0   # (at most the reads with noise)


@pytest.mark.parametrize("svb", [False, True])
def test_job_api(gpu, memo, cat, longs, svb):
    """more than 1024 reads through the job API (the cases of up to 5000 samples, many times over): the dispatch order and
    the packed tail; plain samples and svb-zd blobs"""
    from sigtk_amd import blow5
    for rna in (0, 1):
        small = [k for k in cat if k.raw.size <= 5000 and rna in k.rna]
        cases = small * (1024 // len(small) + 1)
        assert len(cases) > 1024
        reads = [k.raw for k in cases]
        sig = [blow5.svb_zd_encode(r) for r in reads] if svb else reads
        job = gpu.Job(0)
        try:
            job.submit(gpu.TOOL_EVENT, sig, *_scal(len(reads)), rna=rna, counts=[r.size for r in reads] if svb else None)
            res = job.wait()
        finally:
            job.close()
        st = res["status"]
        _report("job%s" % (" svb" if svb else ""), rna, st, sum(1 for k in cases if longs["%s/rna%d" % (k.name, rna)]))
        _compare(memo, [k.name for k in cases], reads, rna, res["events"], "job")
        assert st.n_capacity_overflow == 0 and st.n_long_replays > 0 and st.n_replay_indices > 0
        assert st.n_events_total == sum(g.start.size for g in res["events"])


@pytest.mark.parametrize("kind", ["dna", "rna"])
def test_cli_is_byte_identical_to_the_reference(gpu, cat, tmp_path, kind):
    """`sigtk-amd event` and `event -c`, each also with --gpu-text, on a BLOW5 of event_cases.cli_cases(), against what the
    reference CLI printed for the same file (tests/golden/make_golden_event_cases.py)"""
    from sigtk_amd import blow5, build
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    path = str(tmp_path / "cases.blow5")
    recs = [blow5.Read(k.name, 0, *E.SCALE, 4000.0, k.raw) for k in E.cli_cases(cat)]
    assert len(recs) == 30
    blow5.write_blow5(path, recs, HEADERS[kind])
    for fname, tool in (("event_cases_%s.event.tsv" % kind, ["event"]), ("event_cases_%s.event_c.tsv" % kind, ["event", "-c"])):
        want = open(os.path.join(GOLDEN, fname), "rb").read()
        for opts in ([], ["--gpu-text"]):
            p = subprocess.run([build.CLI, *tool, *opts, path], capture_output=True)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert p.stdout == want, "%s options %s: first differing row %r" % (
                fname, opts, next((a, b) for a, b in zip(p.stdout.split(b"\n") + [b""], want.split(b"\n")) if a != b))


def _three_reads(cat, rna):
    """the three longest catalogue reads of this preset with at most 3 000 samples"""
    reads = sorted((k.raw for k in cat if rna in k.rna and k.raw.size <= 3000), key=lambda x: -x.size)[:3]
    assert len(reads) == 3 and reads[-1].size >= 1000
    return reads


def _opt_records(gpu, reads, rna):
    """sgk_event_opt with the default options on `reads` -> (the batch, per read its records as an int32 array [k, 4])"""
    import torch
    from sigtk_amd import device
    b = device.upload_reads(reads, *_scal(len(reads)), torch.device("cuda", 0))
    arena = device.EventArena(b)
    device.event(b, arena, rna)
    torch.cuda.synchronize()
    assert arena.status().n_capacity_overflow == 0
    recs = [arena.events[int(arena.slots_host[r]):int(arena.slots_host[r]) + int(arena.n_events[r].item())].cpu().numpy()
            for r in range(len(reads))]
    assert all(x.shape[0] >= 1 for x in recs) and sum(x.shape[0] for x in recs) > 10   # (one of the reads may be flat)
    return b, recs


@pytest.mark.parametrize("rna", [0, 1])
def test_plain_sgk_event_equals_sgk_event_opt(gpu, cat, rna):
    """sgk_event (no options argument) has no other caller in the suite: its records on three catalogue reads are
    sgk_event_opt's with the default options, bit for bit"""
    import ctypes as C
    import torch
    from sigtk_amd import device
    b, want = _opt_records(gpu, _three_reads(cat, rna), rna)
    L = gpu.load_library()
    arena = device.EventArena(b)
    assert arena.ws_bytes == L.sgk_event_workspace_bytes(b.n_reads, b.n_samples, b.max_read_len)
    arena.events.fill_(-1)
    arena.n_events.fill_(-1)
    view = b.view()
    gpu.check(L.sgk_event(C.byref(view), rna, arena.slots.data_ptr(), arena.events.data_ptr(), arena.n_events.data_ptr(),
                          arena.ws.data_ptr(), arena.ws_bytes, device._stream_ptr()), "sgk_event")
    torch.cuda.synchronize()
    for r, w in enumerate(want):
        s = int(arena.slots_host[r])
        assert int(arena.n_events[r].item()) == w.shape[0]
        assert np.array_equal(arena.events[s:s + w.shape[0]].cpu().numpy(), w), "read %d" % r


@pytest.mark.parametrize("rna", [0, 1])
def test_plain_sgk_event_host_equals_sgk_event_opt(gpu, cat, rna):
    """sgk_event_host (no options argument) likewise: host arrays in, the four host arrays out, against sgk_event_opt's
    records on the same three reads, bit for bit"""
    import ctypes as C
    reads = _three_reads(cat, rna)
    _, want = _opt_records(gpu, reads, rna)
    L = gpu.load_library()
    hb = gpu._HB(reads, *E.SCALE)
    ev = gpu.EventsHost()
    gpu.check(L.sgk_event_host(C.byref(hb.c), rna, C.byref(ev)), "sgk_event_host")
    try:
        offs = gpu._np_from(ev.ev_offsets, len(reads) + 1, np.uint64)
        tot = int(offs[-1])
        cols = [gpu._np_from(p, tot, t) for p, t in ((ev.start, np.uint32), (ev.length, np.uint32), (ev.mean, np.float32),
                                                     (ev.stdv, np.float32))]
    finally:
        L.sgk_events_host_free(C.byref(ev))
    assert offs.tolist() == np.concatenate([[0], np.cumsum([w.shape[0] for w in want])]).tolist()
    for r, w in enumerate(want):
        for c, col in enumerate(cols):
            assert np.array_equal(col[int(offs[r]):int(offs[r + 1])].view(np.int32), w[:, c]), "read %d column %d" % (r, c)
