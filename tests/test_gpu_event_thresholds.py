"""GPU: the presets' kernels with run-time thresholds (SGK_EVENT_PARAMS_PRESET_KERNELS: k_event, k_event_seg, k_event_multi
and k_event_fallback as <W1, T, RT = true>) -- windows 3/6 and 7/14 with the caller's threshold1, threshold2 >= 9 and
peak_height.

The yardstick is the model of tests/event_params_model.py, bit for bit; tests/test_event_thresholds_cpu.py shows that the
reads of tests/event_threshold_cases.py tell every run-time threshold from the preset's constant.  The generic kernel
k_event_param (SGK_EVENT_PARAMS_GENERIC) is compared as a second, independent implementation.  Wherever a buffer is handed
in, the event arena, the counts and the workspace sit between canary regions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import event_params_model as M
import event_threshold_cases as TC
import tsv_grammar as G

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
GUARD = 4096            # canary bytes on either side of a buffer
CAN32 = 0x5A5A5A5A      # canary word


def _torch():
    import torch
    return torch


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def _params(gpu, p, fast=True, generic=False):
    flags = (gpu.SGK_EVENT_PARAMS_PRESET_KERNELS if fast else 0) | (gpu.SGK_EVENT_PARAMS_GENERIC if generic else 0)
    return gpu.EventParams(p.w1, p.w2, p.thr1, p.thr2, p.ph, flags)


def _opts(gpu, **kw):
    o = gpu.EventOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Run:
    """one sgk_event_param / sgk_event_pa_param call on a list of TC.Read, canaries around everything it is given"""

    def __init__(self, gpu, reads, params, oracle_pa=None, leads=None, caps=None, ws_short=0, **options):
        torch = _torch()
        from sigtk_amd import device
        dev = torch.device("cuda", 0)
        L = gpu.load_library()
        n = len(reads)
        lens = np.array([rd.raw.size for rd in reads], dtype=np.int64)
        b = device.alloc_reads(lens, dev, leads=leads)
        host = np.zeros(b.n_samples, dtype=np.int16)
        hostf = np.zeros(b.n_samples, dtype=F)
        for r, rd in enumerate(reads):
            o = int(b.offsets_host[r])
            if oracle_pa is not None:
                hostf[o:o + rd.raw.size] = oracle_pa.pa(rd.raw, *rd.scale)
            else:
                host[o:o + rd.raw.size] = rd.raw
        b.samples.copy_(torch.from_numpy(host))
        if n:
            for k, t in enumerate((b.dig, b.off, b.rng)):
                t[:n] = torch.from_numpy(np.array([rd.scale[k] for rd in reads], dtype=np.float64))
        self.b = b
        caps = gpu.event_slots_for(lens) if caps is None else np.asarray(caps, dtype=np.int64)
        slots = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(caps, out=slots[1:])
        self.slots_host, self.caps = slots, caps
        n_slots = int(slots[-1])
        gw = GUARD // 4
        self.ev = torch.full((gw + 4 * max(n_slots, 1) + gw,), CAN32, dtype=torch.int32, device=dev)
        self.cnt = torch.full((gw + max(n, 1) + gw,), CAN32, dtype=torch.int32, device=dev)
        d_slots = torch.from_numpy(slots).to(dev)
        self.opt = opt = _opts(gpu, **options)
        self.ws_bytes = int(L.sgk_event_workspace_bytes_param(b.n_reads, b.n_samples, b.max_read_len, C.byref(opt), C.byref(params)))
        assert self.ws_bytes > 0
        self.ws = torch.full((GUARD + self.ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws_ptr, ev_ptr = self.ws.data_ptr() + GUARD, self.ev.data_ptr() + GUARD
        assert ws_ptr % 64 == 0 and ev_ptr % 16 == 0
        stream = torch.cuda.current_stream().cuda_stream
        if oracle_pa is not None:
            pa = torch.from_numpy(hostf).to(dev)
            self.rc = L.sgk_event_pa_param(pa.data_ptr(), b.offsets.data_ptr(), b.lengths.data_ptr(), n, b.max_read_len,
                                           b.n_samples, C.byref(params), d_slots.data_ptr(), ev_ptr, self.cnt.data_ptr() + GUARD,
                                           ws_ptr, self.ws_bytes - ws_short, stream, C.byref(opt))
        else:
            view = b.view()
            self.rc = L.sgk_event_param(C.byref(view), C.byref(params), d_slots.data_ptr(), ev_ptr, self.cnt.data_ptr() + GUARD,
                                        ws_ptr, self.ws_bytes - ws_short, stream, C.byref(opt))
        torch.cuda.synchronize()
        self.status = gpu.EventStatus()
        self.status_rc = None
        if self.rc == gpu.SGK_OK and n:
            self.status_rc = L.sgk_event_status(ws_ptr, C.byref(self.status), stream)
        ev, cnt, ws = self.ev.cpu().numpy(), self.cnt.cpu().numpy(), self.ws.cpu().numpy()
        self.canaries_ok = bool((ev[:gw] == CAN32).all() and (ev[gw + 4 * max(n_slots, 1):] == CAN32).all() and
                                (cnt[:gw] == CAN32).all() and (cnt[gw + max(n, 1):] == CAN32).all() and
                                (ws[:GUARD] == 0xA5).all() and (ws[GUARD + self.ws_bytes:] == 0xA5).all())
        self.ev_host = ev[gw:gw + 4 * max(n_slots, 1)].reshape(-1, 4)
        self.cnt_host = cnt[gw:gw + max(n, 1)][:n]
        self.ws_host = ws[GUARD:GUARD + self.ws_bytes]

    def events(self, r):
        k = min(int(self.cnt_host[r]), int(self.caps[r]))
        s = int(self.slots_host[r])
        rec = self.ev_host[s:s + k]
        return M.Events(rec[:, 0].copy().view(np.uint32), rec[:, 1].copy().view(np.uint32),
                        rec[:, 2].copy().view(F), rec[:, 3].copy().view(F))


def _same(got, want, what, keep=None):
    k = want.start.size if keep is None else keep
    assert got.start.size == k, "%s: %d events, want %d" % (what, got.start.size, k)
    assert np.array_equal(got.start, want.start[:k]), "%s: starts" % what
    assert np.array_equal(got.length, want.length[:k]), "%s: lengths" % what
    assert np.array_equal(_bits(got.mean), _bits(want.mean[:k])), "%s: mean bits" % what
    assert np.array_equal(_bits(got.stdv), _bits(want.stdv[:k])), "%s: stdv bits" % what


class _Model:
    """the model's events, computed once per (read, parameters) for the whole module"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, rd, p):
        key = (rd.raw.tobytes(), rd.scale, p)
        if key not in self.memo:
            self.memo[key] = M.events_raw(self.oracle, rd.raw, *rd.scale, p)
        return self.memo[key]


@pytest.fixture(scope="module")
def model(oracle):
    return _Model(oracle)


def _check(run, gpu, reads, p, model, what):
    """rc, canaries, every read's count and events, the total"""
    assert run.rc == gpu.SGK_OK and run.status_rc == gpu.SGK_OK, (what, run.rc, run.status_rc)
    assert run.canaries_ok, what
    total = 0
    for r, rd in enumerate(reads):
        want = model(rd, p)
        assert int(run.cnt_host[r]) == want.start.size, "%s read %s (n=%d): count %d, want %d" % (
            what, rd.name, rd.raw.size, int(run.cnt_host[r]), want.start.size)
        _same(run.events(r), want, "%s read %s (n=%d)" % (what, rd.name, rd.raw.size))
        total += want.start.size
    assert run.status.n_events_total == total and run.status.n_capacity_overflow == 0, what
    return run.status


def _generic_zeros(st):
    return (st.n_fallback_reads, st.n_long_replays, st.n_split_reads, st.n_segments, st.n_seam_reruns, st.n_replay_indices) == (0,) * 6


def _line(what, st):
    print("%s: n_events_total %d n_fallback_reads %d n_rerun_passes %d n_long_replays %d n_replay_indices %d n_split_reads %d "
          "n_segments %d n_seam_reruns %d" % (what, st.n_events_total, st.n_fallback_reads, st.n_rerun_passes, st.n_long_replays,
                                              st.n_replay_indices, st.n_split_reads, st.n_segments, st.n_seam_reruns))


def _plan(gpu, reads, rna, **options):
    lens = np.array([rd.raw.size for rd in reads], dtype=np.int64)
    p = gpu.EventPlan()
    assert gpu.load_library().sgk_event_plan_opt(len(lens), int(((lens + 7) // 8 * 8).sum()), int(lens.max()), rna,
                                                 C.byref(_opts(gpu, **options)), C.byref(p)) == 0
    return p


# ------------------------------------------------------------------------------------------------ 1. every set

@pytest.mark.parametrize("as_pa", [False, True], ids=["raw", "pa"])
@pytest.mark.parametrize("p", TC.FAST, ids=[TC.ident(p) for p in TC.FAST])
def test_fast_sets_against_the_model_and_the_generic_kernel(gpu, oracle, model, p, as_pa):
    reads = TC.reads()
    assert gpu.event_params_route(_params(gpu, p)) == gpu.SGK_EVENT_ROUTE_PRESET_WINDOWS
    fast = Run(gpu, reads, _params(gpu, p), oracle_pa=oracle if as_pa else None)
    st = _check(fast, gpu, reads, p, model, "fast %s" % TC.ident(p))
    _line("fast %s %s" % (TC.ident(p), "pA" if as_pa else "int16"), st)
    # the workspace and the status are sgk_event_opt's
    assert fast.ws_bytes == gpu.load_library().sgk_event_workspace_bytes_opt(fast.b.n_reads, fast.b.n_samples, fast.b.max_read_len, C.byref(fast.opt))
    assert st.n_fallback_reads >= 1                      # the read that fails the exactness guard, on k_event_fallback<.., true>
    gen = Run(gpu, reads, _params(gpu, p, generic=True), oracle_pa=oracle if as_pa else None)
    assert gen.rc == gpu.SGK_OK and gen.status_rc == gpu.SGK_OK and gen.canaries_ok and _generic_zeros(gen.status)
    assert np.array_equal(gen.cnt_host, fast.cnt_host)
    for r, rd in enumerate(reads):
        _same(fast.events(r), gen.events(r), "fast against generic, read %s" % rd.name)
    assert gen.status.n_events_total == st.n_events_total
    if p.thr1 == M.FLT_MAX:
        assert st.n_long_replays + st.n_replay_indices > 0, "no run of the long detector was replayed"


def test_presets_with_the_flag_take_the_presets_kernels(gpu):
    """parameters equal to a preset take sgk_event_opt's launch, flag or not: identical arena, counts and status"""
    torch = _torch()
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    reads = TC.catalogue_reads(20000) + [TC.guard_read(), TC.guard_fail_read()]
    b = device.upload_reads([rd.raw for rd in reads], *(np.array([rd.scale[k] for rd in reads]) for k in range(3)), dev)
    for rna in (0, 1):
        a0, a1 = device.EventArena(b), device.EventArena(b)
        a0.events.fill_(CAN32), a1.events.fill_(CAN32)
        device.event(b, a0, rna)
        p = gpu.EventParams.preset(rna).preset_kernels()
        assert p.route() == gpu.SGK_EVENT_ROUTE_PRESET and a1.param_workspace_bytes(b, p) == a0.ws_bytes
        device.event(b, a1, rna, params=p)
        torch.cuda.synchronize()
        assert torch.equal(a0.events, a1.events) and torch.equal(a0.n_events, a1.n_events)
        assert bytes(a0.status()) == bytes(a1.status())


# ------------------------------------------------------------------------------------------------ 2. every launch form

FORMS = [(rna, p) for rna in (0, 1) for p in TC.FORM_SETS[rna]]
FORM_IDS = [TC.ident(p) for _, p in FORMS]


def _long_reads(n=40000):
    return [TC._r("thr2_steps_long_seed%d" % s, TC.thr2_read(s, n)) for s in (9200, 9201, 9202)]


@pytest.mark.parametrize("rna,p", FORMS, ids=FORM_IDS)
def test_whole_reads(gpu, model, rna, p):
    reads = TC.catalogue_reads(20000) + TC.thr2_reads() + TC.ulp_reads() + _long_reads()[:1]
    form = dict(lanes_per_short_read=-1, tail_split=-1)
    pl = _plan(gpu, reads, rna, **form)
    assert pl.lanes_per_short_read == 0 and pl.tail_segment_len == 0
    run = Run(gpu, reads, _params(gpu, p), **form)
    st = _check(run, gpu, reads, p, model, "whole")
    _line("whole %s" % TC.ident(p), st)
    assert st.n_split_reads == 0 and st.n_segments == 0


@pytest.mark.parametrize("lanes", [2, 32])
@pytest.mark.parametrize("rna,p", FORMS, ids=FORM_IDS)
def test_short_read_packing(gpu, model, rna, p, lanes):
    reads = [TC._r("short_%d" % k, x) for k, x in enumerate(M.random_reads(606, 260, 3000)) if x.size >= 64][:200]
    reads += TC.thr2_reads() + TC.ulp_reads()
    assert len(reads) > 200 and max(rd.raw.size for rd in reads) <= 3000
    form = dict(lanes_per_short_read=lanes, tail_split=-1)
    assert _plan(gpu, reads, rna, **form).lanes_per_short_read == lanes
    run = Run(gpu, reads, _params(gpu, p), **form)
    st = _check(run, gpu, reads, p, model, "packed %d" % lanes)
    _line("packed %d %s" % (lanes, TC.ident(p)), st)
    assert st.n_split_reads == 0


@pytest.mark.parametrize("rna,p", FORMS, ids=FORM_IDS)
def test_long_reads_on_several_wavefronts(gpu, model, rna, p):
    """the smallest segments the options accept: every read from 1 025 samples on is cut into 1 024-sample segments"""
    reads = _long_reads()[:1] + TC.thr2_reads() + TC.catalogue_reads(6000) + [TC._r("n1025", TC.thr2_read(77, 1025))]
    form = dict(segment_len=1024, long_min=1025)
    pl = _plan(gpu, reads, rna, **form)
    assert (pl.segment_len, pl.long_min) == (1024, 1025)
    run = Run(gpu, reads, _params(gpu, p), **form)
    st = _check(run, gpu, reads, p, model, "segments")
    _line("segments %s" % TC.ident(p), st)
    n_long = sum(1 for rd in reads if rd.raw.size >= 1025)
    assert n_long >= 3 and st.n_split_reads == n_long
    assert st.n_segments == sum((rd.raw.size + 1023) // 1024 for rd in reads if rd.raw.size >= 1025)


@pytest.mark.parametrize("rna,p", FORMS, ids=FORM_IDS)
def test_forced_tail_split(gpu, model, rna, p):
    reads = _long_reads()
    form = dict(tail_split=len(reads), lanes_per_short_read=-1)
    pl = _plan(gpu, reads, rna, **form)
    assert pl.tail_split_from == 0 and 16384 <= pl.tail_segment_len < 40000
    run = Run(gpu, reads, _params(gpu, p), **form)
    st = _check(run, gpu, reads, p, model, "tail split")
    _line("tail split %s" % TC.ident(p), st)
    assert st.n_split_reads == len(reads) and st.n_segments >= 2 * len(reads)


@pytest.mark.parametrize("rna,p", FORMS, ids=FORM_IDS)
def test_speculation_failing_changes_nothing(gpu, model, rna, p):
    """a warm-up of 16 samples: chunks and segments start from wrong states and are run again"""
    reads = TC.catalogue_reads(20000) + TC.thr2_reads() + _long_reads(12000)[:2]
    whole = Run(gpu, reads, _params(gpu, p), warmup=16, lanes_per_short_read=-1, tail_split=-1)
    st = _check(whole, gpu, reads, p, model, "warmup 16, whole")
    _line("warmup 16 whole %s" % TC.ident(p), st)
    assert st.n_rerun_passes > 0
    cut = Run(gpu, reads, _params(gpu, p), warmup=16, segment_len=1024, long_min=1025)
    st = _check(cut, gpu, reads, p, model, "warmup 16, segments")
    _line("warmup 16 segments %s" % TC.ident(p), st)
    assert st.n_split_reads > 0 and st.n_seam_reruns > 0


def test_more_reads_than_the_dispatch_order_needs(gpu, model):
    """from 1 024 reads of unequal length on: the dispatch order, packed short reads on a side stream beside k_event"""
    p = TC.FAST_DNA[0]
    reads = [TC._r("r%d" % k, x) for k, x in enumerate(M.random_reads(4243, 1100, 90))]
    reads[17] = TC._r("r17", TC.thr2_read(5, 20000))
    run = Run(gpu, reads, _params(gpu, p))
    _check(run, gpu, reads, p, model, "1100 reads")


# ------------------------------------------------------------------------------------------------ 3. alignment

@pytest.mark.parametrize("rna", [0, 1])
def test_every_sample_offset_residue(gpu, model, rna):
    p = TC.FORM_SETS[rna][0]
    reads = [TC._r("res_n%d" % n, TC.thr2_read(40 + n, n)) for n in (777, 4097, 130, 64, 1000, 333, 2048, 65)]
    for shift in range(8):
        leads = [(shift + r) % 8 for r in range(len(reads))]
        run = Run(gpu, reads, _params(gpu, p), leads=leads)
        assert all(int(o) % 8 == (shift + r) % 8 for r, o in enumerate(run.b.offsets_host))
        _check(run, gpu, reads, p, model, "shift %d" % shift)


# ------------------------------------------------------------------------------------------------ 4. outside the domain

@pytest.mark.parametrize("p", TC.GENERIC_WITH_FLAG, ids=[TC.ident(p) for p in TC.GENERIC_WITH_FLAG])
def test_sets_outside_the_fast_domain_ignore_the_flag(gpu, model, p):
    reads = TC.catalogue_reads(20000) + TC.thr2_reads() + TC.edge_reads()
    assert gpu.event_params_route(_params(gpu, p)) == gpu.SGK_EVENT_ROUTE_GENERIC
    run = Run(gpu, reads, _params(gpu, p))
    st = _check(run, gpu, reads, p, model, "generic with the flag")
    assert _generic_zeros(st)
    assert run.ws_bytes == gpu.load_library().sgk_event_workspace_bytes_param(run.b.n_reads, run.b.n_samples, run.b.max_read_len, None, C.byref(_params(gpu, p, fast=False)))


# ------------------------------------------------------------------------------------------------ 5. capacity, workspace

def _three():
    return [TC._r("cap_n%d" % n, TC.thr2_read(300 + n, n)) for n in (900, 2500, 40)]


def test_slot_range_one_short(gpu, model):
    p = TC.FAST_DNA[3]
    reads = _three()
    want = [model(rd, p) for rd in reads]
    k = want[1].start.size
    assert k > 10
    caps = gpu.event_slots_for(np.array([rd.raw.size for rd in reads]))
    caps[1] = k - 1
    run = Run(gpu, reads, _params(gpu, p), caps=caps)
    assert run.rc == gpu.SGK_OK and run.canaries_ok
    assert run.status_rc == gpu.SGK_ERR_CAPACITY and run.status.n_capacity_overflow == 1
    assert [int(c) for c in run.cnt_host] == [w.start.size for w in want]        # the true counts
    _same(run.events(0), want[0], "read 0")
    _same(run.events(1), want[1], "read 1", keep=k - 1)                           # the surplus is dropped
    _same(run.events(2), want[2], "read 2")                                      # ... not written into the next read's slots


def _nothing_written(run, gpu):
    assert run.rc == gpu.SGK_ERR_WORKSPACE
    assert run.canaries_ok
    assert (run.ev_host.view(np.uint32) == CAN32).all() and (run.cnt_host.view(np.uint32) == CAN32).all()
    assert (run.ws_host == 0xA5).all()


def test_workspace_one_byte_short(gpu, model):
    """The route's workspace rule is sgk_event_opt's: sgk_event_workspace_bytes_opt sizes one scratch region of
    16 (max_read_len + 1) bytes per persistent fallback workgroup (min(n_reads, 256) of them), and a call with less runs
    with as many as fit while one does.  So with ONE read a byte less is SGK_ERR_WORKSPACE and nothing is written; with
    three reads a byte less costs a fallback workgroup and nothing else, and a byte less than ONE region is the error."""
    p = TC.FAST_DNA[0]
    _nothing_written(Run(gpu, _three()[1:2], _params(gpu, p), ws_short=1), gpu)
    reads = _three() + [TC.guard_fail_read()]
    per_block = 16 * (max(rd.raw.size for rd in reads) + 1)
    run = Run(gpu, reads, _params(gpu, p), ws_short=1)
    st = _check(run, gpu, reads, p, model, "a byte short with four reads")
    assert st.n_fallback_reads >= 1 and (run.ws_host[-1:] == 0xA5).all()      # (the last byte was not the call's)
    _nothing_written(Run(gpu, reads, _params(gpu, p), ws_short=3 * per_block + 1), gpu)


# ------------------------------------------------------------------------------------------------ 6. jobs

def test_jobs_use_their_parameters(gpu, model):
    torch = _torch()
    from sigtk_amd import api, blow5, device
    p = TC.FAST_DNA[7]
    lens = [5000, 333, 0, 1, 12001, 64, 4097]
    raws, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=72, kind=0)
    reads = [TC._r("job_%d" % r, raws[r], (dig[r], off[r], rng[r])) for r in range(len(lens))]
    ids = [("read-%04d-%s" % (r, "x" * (r * 5))).encode() for r in range(len(lens))]
    run = Run(gpu, reads, _params(gpu, p))
    _check(run, gpu, reads, p, model, "device call")
    changed = sum(1 for rd in reads if TC.differ(model(rd, p), model(rd, TC.preset_of(p))))
    assert changed >= 3, "the job's reads do not tell the tuned set from the preset"
    dev = torch.device("cuda", 0)
    b = device.upload_reads(raws, dig, off, rng, dev)
    arena = device.EventArena(b, params=_params(gpu, p))
    assert arena.ws_bytes == int(gpu.load_library().sgk_event_workspace_bytes_opt(b.n_reads, b.n_samples, b.max_read_len, C.byref(arena.opt)))
    device.event(b, arena, 0, params=_params(gpu, p))
    rows = {c: device.TextWriter(b, ids, api.TEXT_EVENT_COMPACT if c else api.TEXT_EVENT, arena).run() for c in (False, True)}
    assert rows[True] == b"".join(G.event_rows(ids[r].decode(), lens[r], *run.events(r), True).encode() for r in range(len(lens)))

    job = gpu.Job(0)
    job.set_event_params(_params(gpu, p))
    job.stage([blow5.svb_zd_encode(r) for r in raws], dig, off, rng, counts=[r.size for r in raws], ids=ids)
    job.launch(gpu.TOOL_EVENT)
    ev = job.wait()["events"]
    for r in range(len(lens)):
        _same(M.Events(*ev[r]), run.events(r), "job read %d" % r)
    for flags in (gpu.JOB_EVENTS_COMPACT, gpu.JOB_EVENTS_LENGTHS):
        job.launch(gpu.TOOL_EVENT, flags=flags)
        ev = job.wait()["events"]
        for r in range(len(lens)):
            assert np.array_equal(ev[r].start, run.events(r).start) and np.array_equal(ev[r].length, run.events(r).length)
    for flags, compact in ((gpu.JOB_TEXT, False), (gpu.JOB_TEXT | gpu.JOB_EVENTS_COMPACT, True), (gpu.JOB_TEXT | gpu.JOB_EVENTS_LENGTHS, True)):
        job.launch(gpu.TOOL_EVENT, flags=flags)
        assert job.wait()["text"] == rows[compact]
    # back to the presets by rna
    job.set_event_params(None)
    job.launch(gpu.TOOL_EVENT, rna=1)
    ev = job.wait()["events"]
    want, _ = gpu.event(raws, dig, off, rng, 1)
    for r in range(len(lens)):
        _same(M.Events(*ev[r]), M.Events(*want[r]), "presets again, read %d" % r)
    job.close()


# ------------------------------------------------------------------------------------------------ 7. CLI

def _cli():
    from sigtk_amd import build
    assert os.path.exists(build.CLI), "sigtk-amd is not built"
    return build.CLI


BLOW5 = os.path.join(GOLDEN, "sp1_dna.blow5")


@pytest.mark.parametrize("gpu_text", [False, True])
def test_cli_detector_on_the_presets_windows(gpu, oracle, sp1, gpu_text):
    p = TC.FAST_DNA[0]
    cmd = [_cli(), "event", "-c", "-v", "4", "--detector", "3,6,1.0,9,0.1"] + (["--gpu-text"] if gpu_text else []) + [BLOW5]
    done = subprocess.run(cmd, capture_output=True, check=True)
    assert done.stderr.decode().count("[event] detector route: preset windows\n") == 1
    out = done.stdout.decode().split("\n")
    assert out[0].startswith("read_id\t")
    changed = 0
    for r, rd in enumerate(sp1.reads[:10]):
        want = M.events_raw(oracle, rd.raw, rd.digitisation, rd.offset, rd.range, p)
        changed += TC.differ(want, M.events_raw(oracle, rd.raw, rd.digitisation, rd.offset, rd.range, M.PRESETS[0]))
        f = out[1 + r].split("\t")
        assert f[0] == rd.read_id and int(f[1]) == rd.raw.size
        lengths = np.array([int(x) for x in f[5].rstrip(",").split(",")], dtype=np.uint32)
        assert int(f[4]) == want.start.size
        assert np.array_equal(lengths, want.length), rd.read_id
        assert np.array_equal(np.cumsum(lengths) - lengths, want.start), rd.read_id
        assert (int(f[2]), int(f[3])) == (0, rd.raw.size)
    assert changed >= 3
    # without -v 4 nothing is added to stderr's lines, and the rows are the same bytes
    quiet = subprocess.run([c for c in cmd if c not in ("-v", "4")], capture_output=True, check=True)
    assert quiet.stdout == done.stdout and "detector route" not in quiet.stderr.decode()


def test_cli_names_the_generic_route(gpu):
    done = subprocess.run([_cli(), "event", "-c", "-v", "4", "--detector", "3,6,1.4,3,0.2", BLOW5], capture_output=True, check=True)
    assert done.stderr.decode().count("[event] detector route: generic\n") == 1
    assert done.stdout.startswith(b"read_id\t")


def test_cli_detector_with_the_preset_is_still_the_golden(gpu):
    done = subprocess.run([_cli(), "event", "-c", "-v", "4", "--detector", "3,6,1.4,9,0.2", BLOW5], capture_output=True, check=True)
    assert done.stdout == open(os.path.join(GOLDEN, "sp1_dna.event_c.tsv"), "rb").read()
    assert done.stderr.decode().count("[event] detector route: preset\n") == 1
