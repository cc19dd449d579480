"""GPU: event detection with caller-supplied detector parameters (sgk_event_param / sgk_event_pa_param, k_event_param,
sgk_job_set_event_params, sigtk-amd event --detector).

The yardstick is never the generic kernel itself: for the two presets it is sgk_event's own kernels, for every other
parameter set the model of tests/event_params_model.py (the oracle's generic pieces composed with free parameters, pinned
to oracle.getevents by tests/test_event_params_cpu.py).  Everything is compared bit for bit; there are no tolerances.
Wherever a buffer is handed in, the event arena, the counts and the workspace sit between canary regions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import event_cases as E
import event_params_model as M
import tsv_grammar as G

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
GUARD = 4096            # canary bytes on either side of a buffer
CAN32 = 0x5A5A5A5A      # canary word (as int32: 1515870810)


def _torch():
    import torch
    return torch


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def _params(gpu, p, generic=False):
    return gpu.EventParams(p.w1, p.w2, p.thr1, p.thr2, p.ph, gpu.SGK_EVENT_PARAMS_GENERIC if generic else 0)


class Run:
    """one sgk_event_param / sgk_event_pa_param call with canaries around everything it is given"""

    def __init__(self, gpu, reads, p, scal=None, warmup=0, leads=None, caps=None, ws_short=0, oracle_pa=None, pa_rna=None):
        """oracle_pa: the reads go in as pA floats (oracle_pa.pa converts them); pa_rna: ... through plain sgk_event_pa
        with this preset instead of sgk_event_pa_param (the yardstick of the presets; `p` is not used then)"""
        torch = _torch()
        from sigtk_amd import device
        dev = torch.device("cuda", 0)
        L = gpu.load_library()
        n = len(reads)
        lens = np.array([len(r) for r in reads], dtype=np.int64)
        b = device.alloc_reads(lens, dev, leads=leads)
        host = np.zeros(b.n_samples, dtype=np.int16)
        hostf = np.zeros(b.n_samples, dtype=F)
        dig, off, rng = scal if scal is not None else tuple(np.full(max(n, 1), v) for v in E.SCALE)
        for r, raw in enumerate(reads):
            o = int(b.offsets_host[r])
            if oracle_pa is not None:
                hostf[o:o + len(raw)] = oracle_pa.pa(raw, float(dig[r]), float(off[r]), float(rng[r]))
            else:
                host[o:o + len(raw)] = raw
        b.samples.copy_(torch.from_numpy(host))
        if n:
            b.dig[:n] = torch.from_numpy(np.asarray(dig, dtype=np.float64)[:n])
            b.off[:n] = torch.from_numpy(np.asarray(off, dtype=np.float64)[:n])
            b.rng[:n] = torch.from_numpy(np.asarray(rng, dtype=np.float64)[:n])
        self.b = b
        caps = gpu.event_slots_for(lens) if caps is None else np.asarray(caps, dtype=np.int64)
        slots = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(caps, out=slots[1:])
        self.slots_host = slots
        n_slots = int(slots[-1])
        gw = GUARD // 4
        self.ev = torch.full((gw + 4 * max(n_slots, 1) + gw,), CAN32, dtype=torch.int32, device=dev)
        self.cnt = torch.full((gw + max(n, 1) + gw,), CAN32, dtype=torch.int32, device=dev)
        d_slots = torch.from_numpy(slots).to(dev)
        opt = gpu.EventOptions(0, 0, int(warmup), 0, 0, 0)
        if pa_rna is not None:
            assert oracle_pa is not None and not warmup
            self.ws_bytes = int(L.sgk_event_workspace_bytes(b.n_reads, b.n_samples, b.max_read_len))
        else:
            self.ws_bytes = int(L.sgk_event_workspace_bytes_param(b.n_reads, b.n_samples, b.max_read_len, C.byref(opt), C.byref(p)))
        assert self.ws_bytes > 0
        self.ws = torch.full((GUARD + self.ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws_ptr = self.ws.data_ptr() + GUARD
        ev_ptr = self.ev.data_ptr() + GUARD
        assert ws_ptr % 64 == 0 and ev_ptr % 16 == 0
        stream = torch.cuda.current_stream().cuda_stream
        if pa_rna is not None:
            pa = torch.from_numpy(hostf).to(dev)
            self.rc = L.sgk_event_pa(pa.data_ptr(), b.offsets.data_ptr(), b.lengths.data_ptr(), n, b.max_read_len, b.n_samples,
                                     int(pa_rna), d_slots.data_ptr(), ev_ptr, self.cnt.data_ptr() + GUARD, ws_ptr,
                                     self.ws_bytes - ws_short, stream)
        elif oracle_pa is not None:
            pa = torch.from_numpy(hostf).to(dev)
            self.rc = L.sgk_event_pa_param(pa.data_ptr(), b.offsets.data_ptr(), b.lengths.data_ptr(), n, b.max_read_len,
                                           b.n_samples, C.byref(p), d_slots.data_ptr(), ev_ptr, self.cnt.data_ptr() + GUARD,
                                           ws_ptr, self.ws_bytes - ws_short, stream, C.byref(opt))
        else:
            view = b.view()
            self.rc = L.sgk_event_param(C.byref(view), C.byref(p), d_slots.data_ptr(), ev_ptr, self.cnt.data_ptr() + GUARD,
                                        ws_ptr, self.ws_bytes - ws_short, stream, C.byref(opt))
        torch.cuda.synchronize()
        self.status = gpu.EventStatus()
        self.status_rc = None
        if self.rc == gpu.SGK_OK and n:
            self.status_rc = L.sgk_event_status(ws_ptr, C.byref(self.status), stream)
        ev = self.ev.cpu().numpy()
        cnt = self.cnt.cpu().numpy()
        ws = self.ws.cpu().numpy()
        self.canaries_ok = bool((ev[:gw] == CAN32).all() and (ev[gw + 4 * max(n_slots, 1):] == CAN32).all() and
                                (cnt[:gw] == CAN32).all() and (cnt[gw + max(n, 1):] == CAN32).all() and
                                (ws[:GUARD] == 0xA5).all() and (ws[GUARD + self.ws_bytes:] == 0xA5).all())
        self.ev_host = ev[gw:gw + 4 * max(n_slots, 1)].reshape(-1, 4)
        self.cnt_host = cnt[gw:gw + max(n, 1)][:n]
        self.ws_host = ws[GUARD:GUARD + self.ws_bytes]
        self.caps = caps

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


class _AsIs:
    """for Run(oracle_pa=...): the reads are pA arrays already"""

    @staticmethod
    def pa(raw, *scale):
        return raw


class _Model:
    """the model's events, computed once per (read, parameters) for the whole module"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, raw, p, scal=E.SCALE):
        key = (np.ascontiguousarray(raw, dtype=np.int16).tobytes(), p, tuple(float(v) for v in scal))
        if key not in self.memo:
            self.memo[key] = M.events_raw(self.oracle, raw, *scal, p)
        return self.memo[key]


@pytest.fixture(scope="module")
def model(oracle):
    return _Model(oracle)


@pytest.fixture(scope="module")
def cat():
    return E.catalogue()


def _edge_lengths(gpu, p):
    """0, 1, around 2w for both windows, around every length at which the kernel's chunk length changes, and 20 000"""
    c = gpu.EVENT_GENERIC_CHUNK_SAMPLES
    out = [0, 1]
    for w in (p.w1, p.w2):
        out += [2 * w - 1, 2 * w, 2 * w + 1]
    out += [c - 1, c, c + 1, 2 * c, 2 * c + 1, 20000]
    return out


def _edge_reads(gpu, p, seed):
    rng = np.random.default_rng(seed)
    return [M.random_read(rng, n) for n in _edge_lengths(gpu, p)]


def _check_run(run, gpu, reads, p, model, what, scal=None):
    assert run.rc == gpu.SGK_OK and run.status_rc == gpu.SGK_OK, (what, run.rc, run.status_rc)
    assert run.canaries_ok, what
    total = 0
    for r, raw in enumerate(reads):
        sc = E.SCALE if scal is None else (float(scal[0][r]), float(scal[1][r]), float(scal[2][r]))
        want = model(raw, p, sc)
        assert int(run.cnt_host[r]) == want.start.size, "%s read %d (n=%d): count %d, want %d" % (
            what, r, len(raw), int(run.cnt_host[r]), want.start.size)
        _same(run.events(r), want, "%s read %d (n=%d)" % (what, r, len(raw)))
        total += want.start.size
    st = run.status
    assert st.n_events_total == total and st.n_capacity_overflow == 0
    assert (st.n_fallback_reads, st.n_long_replays, st.n_split_reads, st.n_segments, st.n_seam_reruns, st.n_replay_indices) == (0,) * 6


# ------------------------------------------------------------------------------------------------ 1. presets

@pytest.mark.parametrize("rna", [0, 1])
def test_presets_on_the_generic_kernel_equal_sgk_event(gpu, cat, rna):
    """both presets with SGK_EVENT_PARAMS_GENERIC over the whole catalogue, raw reads (here) and pA arrays (the next
    test): every field is sgk_event's"""
    reads = [k.raw for k in cat]
    scal = tuple(np.full(len(reads), v) for v in E.SCALE)
    want, st0 = gpu.event(reads, *scal, rna)
    run = Run(gpu, reads, _params(gpu, M.PRESETS[rna], generic=True))
    assert run.rc == gpu.SGK_OK and run.status_rc == gpu.SGK_OK and run.canaries_ok
    for r, k in enumerate(cat):
        assert int(run.cnt_host[r]) == want[r].start.size, k.name
        _same(run.events(r), M.Events(want[r].start, want[r].length, want[r].mean, want[r].stdv), k.name)
    assert run.status.n_events_total == st0.n_events_total and run.status.n_fallback_reads == 0
    print("generic kernel on preset %d: %d events, %d re-run chunks" % (rna, run.status.n_events_total, run.status.n_rerun_passes))


@pytest.mark.parametrize("rna", [0, 1])
def test_presets_on_the_generic_kernel_equal_sgk_event_pa(gpu, rna):
    """the catalogue's pA arrays -- what raw reads cannot hold, the -0.0 plateaus among them -- through sgk_event_pa_param
    with SGK_EVENT_PARAMS_GENERIC against plain sgk_event_pa on the same arrays, every one with both presets: every field
    bit for bit (arrays with NaN or infinite samples are outside the generic path's contract)"""
    cases = [k for k in E.pa_cases() if np.isfinite(k.pa).all()]
    assert any(np.signbit(k.pa[k.pa == 0]).any() for k in cases), "no -0.0 among the pA arrays"
    arrays = [k.pa for k in cases]
    want = Run(gpu, arrays, None, oracle_pa=_AsIs, pa_rna=rna)
    got = Run(gpu, arrays, _params(gpu, M.PRESETS[rna], generic=True), oracle_pa=_AsIs)
    for run in (want, got):
        assert run.rc == gpu.SGK_OK and run.status_rc == gpu.SGK_OK and run.canaries_ok
    assert got.status.n_fallback_reads == 0 and got.status.n_events_total == want.status.n_events_total
    for r, k in enumerate(cases):
        assert int(got.cnt_host[r]) == int(want.cnt_host[r]), k.name
        _same(got.events(r), want.events(r), k.name)
    assert sum(int(c) for c in want.cnt_host) > len(cases)      # the arrays have peaks: more than one event each on average


@pytest.mark.parametrize("rna", [0, 1])
def test_presets_without_the_flag_take_sgk_event_opt(gpu, cat, rna):
    """identical arena, counts and status as sgk_event_opt: the same kernels through the same launch"""
    torch = _torch()
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    reads = [k.raw for k in cat] + [np.full(300, 1 - int(E.SCALE[1]), dtype=np.int16)]   # the last one fails the exactness guard
    scal = tuple(np.full(len(reads), v) for v in E.SCALE)
    b = device.upload_reads(reads, *scal, dev)
    a0, a1 = device.EventArena(b), device.EventArena(b)
    a0.events.fill_(CAN32), a1.events.fill_(CAN32)
    device.event(b, a0, rna)
    p = gpu.EventParams.preset(rna)
    assert a1.param_workspace_bytes(b, p) == a0.ws_bytes
    device.event(b, a1, rna, params=p)
    torch.cuda.synchronize()
    assert torch.equal(a0.events, a1.events) and torch.equal(a0.n_events, a1.n_events)
    s0, s1 = a0.status(), a1.status()
    assert bytes(s0) == bytes(s1)
    assert s0.n_fallback_reads >= 1


# ------------------------------------------------------------------------------------------------ 2. the grid

@pytest.mark.parametrize("p", M.GRID_OFF, ids=["%d-%d-%g-%g-%g" % tuple(p) for p in M.GRID_OFF])
def test_grid_against_the_model(gpu, model, cat, p):
    reads = [k.raw for k in cat] + _edge_reads(gpu, p, seed=1000 + p.w1 * 100 + p.w2)
    run = Run(gpu, reads, _params(gpu, p))
    _check_run(run, gpu, reads, p, model, "grid %r" % (p,))
    print("%r: %d events, %d re-run chunks" % (p, run.status.n_events_total, run.status.n_rerun_passes))


def test_more_reads_than_the_dispatch_order_needs(gpu, model):
    """from 1024 reads of unequal length on the wavefronts take the reads longest first"""
    p = M.GRID_OFF[1]
    reads = M.random_reads(4242, 1100, 90)
    reads[17] = M.random_read(np.random.default_rng(3), 5000)
    run = Run(gpu, reads, _params(gpu, p))
    _check_run(run, gpu, reads, p, model, "1100 reads")


# ------------------------------------------------------------------------------------------------ 3. speculation failing

def _pending_peak_read():
    """a short peak pending across a chunk end: plateaus with a step a few samples in front of index 64 k, so that the
    chunk behind starts in the middle of a peak whatever a 16-sample warm-up saw"""
    rng = np.random.default_rng(99)
    x = np.full(4096, 500.0)
    for k in range(1, 64):
        x[64 * k - 3:] += float(rng.choice([-60.0, 60.0]))
    x += rng.normal(0.0, 2.0, x.size)
    return np.rint(x).astype(np.int16)


def test_speculation_failing_changes_nothing(gpu, model, cat):
    """a warm-up of 16 samples: chunks start from wrong states and are re-run; the results are the model's"""
    reads = [k.raw for k in cat if k.raw.size <= 20000] + [_pending_peak_read()] + M.random_reads(31, 20, 6000)
    reruns = {}
    for p in M.GRID:
        preset = p in M.PRESETS.values()
        run = Run(gpu, reads, _params(gpu, p, generic=preset), warmup=16)
        _check_run(run, gpu, reads, p, model, "warmup 16 %r" % (p,))
        reruns[p] = run.status.n_rerun_passes
    print("re-run chunks with a warm-up of 16:", reruns)
    assert max(reruns.values()) > 0, reruns


# ------------------------------------------------------------------------------------------------ 4. alignment

def test_every_sample_offset_residue(gpu, model):
    p = M.GRID_OFF[3]
    rng = np.random.default_rng(8)
    reads = [M.random_read(rng, n) for n in (777, 4097, 130, 64, 1000, 333, 2048, 65)]
    for shift in range(8):
        leads = [(shift + r) % 8 for r in range(len(reads))]
        run = Run(gpu, reads, _params(gpu, p), leads=leads)
        assert all(int(o) % 8 == (shift + r) % 8 for r, o in enumerate(run.b.offsets_host))
        _check_run(run, gpu, reads, p, model, "shift %d" % shift)


# ------------------------------------------------------------------------------------------------ 5. pA input

def test_pa_input(gpu, oracle, model, cat):
    p = M.GRID_OFF[1]
    reads = [k.raw for k in cat if k.raw.size <= 20000][:40] + _edge_reads(gpu, p, seed=77)
    run = Run(gpu, reads, _params(gpu, p), oracle_pa=oracle)
    _check_run(run, gpu, reads, p, model, "pa")
    # pA arrays that no raw read holds (-0.0 among them), against the model on the array itself
    for k in E.pa_cases():
        if not np.isfinite(k.pa).all():
            continue
        want = M.events_pa(oracle, k.pa, p)
        run = Run(gpu, [k.pa], _params(gpu, p), oracle_pa=_AsIs)
        assert run.rc == gpu.SGK_OK and run.canaries_ok
        _same(run.events(0), want, k.name)


def test_getevents_param_shim(gpu, oracle, sp1):
    """sgk_getevents_param(nsample, pA*, params): getevents() with the caller's detector_param, per read"""
    L = gpu.load_library()

    class Tab(C.Structure):
        _fields_ = [("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t), ("event", C.c_void_p)]

    L.sgk_getevents_param.restype = Tab
    L.sgk_getevents_param.argtypes = [C.c_size_t, C.c_void_p, C.POINTER(gpu.EventParams)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    rec_t = np.dtype([("start", "<u8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4"), ("pad", "<u4")])
    for p in (M.GRID_OFF[1], M.PRESETS[1]):
        for r in sp1.reads[:2]:
            pa = oracle.pa(r.raw, r.digitisation, r.offset, r.range)
            want = M.events_pa(oracle, pa, p)
            t = L.sgk_getevents_param(pa.size, pa.ctypes.data, C.byref(_params(gpu, p)))
            assert t.n == want.start.size and t.start == 0 and t.end == t.n
            rec = np.frombuffer(C.string_at(t.event, t.n * rec_t.itemsize), dtype=rec_t)
            libc.free(t.event)
            _same(M.Events(rec["start"].astype(np.uint32), rec["length"].astype(np.uint32), rec["mean"], rec["stdv"]), want, r.read_id)
    # out of domain, or no parameters: an empty table
    pa = oracle.pa(sp1.reads[0].raw, 8192.0, 10.0, 1400.0)
    t = L.sgk_getevents_param(pa.size, pa.ctypes.data, C.byref(gpu.EventParams(1, 6, 1.0, 1.0, 1.0, 0)))
    assert t.n == 0 and not t.event
    t = L.sgk_getevents_param(pa.size, pa.ctypes.data, None)
    assert t.n == 0 and not t.event


# ------------------------------------------------------------------------------------------------ 6. capacity

def test_slot_range_one_short(gpu, model):
    p = M.GRID_OFF[0]
    rng = np.random.default_rng(12)
    reads = [M.random_read(rng, n) for n in (900, 2500, 40)]
    want = [model(r, p) for r in reads]
    k = want[1].start.size
    assert k > 10
    caps = gpu.event_slots_for(np.array([len(r) for r in reads]))
    caps[1] = k - 1
    run = Run(gpu, reads, _params(gpu, p), caps=caps)
    assert run.rc == gpu.SGK_OK and run.canaries_ok
    assert run.status_rc == gpu.SGK_ERR_CAPACITY and run.status.n_capacity_overflow == 1
    assert [int(c) for c in run.cnt_host] == [w.start.size for w in want]        # the true counts
    _same(run.events(0), want[0], "read 0")
    _same(run.events(1), want[1], "read 1", keep=k - 1)                           # the surplus is dropped
    _same(run.events(2), want[2], "read 2")                                      # ... not written into the next read's slots


# ------------------------------------------------------------------------------------------------ 7. workspace

def test_workspace_one_byte_short(gpu):
    p = M.GRID_OFF[1]
    rng = np.random.default_rng(13)
    reads = [M.random_read(rng, n) for n in (900, 2500, 40)]
    run = Run(gpu, reads, _params(gpu, p), ws_short=1)
    assert run.rc == gpu.SGK_ERR_WORKSPACE
    assert run.canaries_ok
    assert (run.ev_host.view(np.uint32) == CAN32).all() and (run.cnt_host.view(np.uint32) == CAN32).all()
    assert (run.ws_host == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 8. jobs

def test_jobs_use_their_parameters(gpu, model):
    torch = _torch()
    from sigtk_amd import api, blow5, device
    p = M.GRID_OFF[3]
    lens = [5000, 333, 0, 1, 12001, 64, 4097]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=71, kind=0)
    ids = [("read-%04d-%s" % (r, "x" * (r * 5))).encode() for r in range(len(lens))]
    # the device call's events: the model's (checked), and the rows TextWriter makes from them
    run = Run(gpu, reads, _params(gpu, p), scal=(dig, off, rng))
    _check_run(run, gpu, reads, p, model, "device call", scal=(dig, off, rng))
    dev = torch.device("cuda", 0)
    b = device.upload_reads(reads, dig, off, rng, dev)
    arena = device.EventArena(b, params=_params(gpu, p))
    device.event(b, arena, 0, params=_params(gpu, p))
    rows = {c: device.TextWriter(b, ids, api.TEXT_EVENT_COMPACT if c else api.TEXT_EVENT, arena).run() for c in (False, True)}
    assert rows[True] == b"".join(G.event_rows(ids[r].decode(), lens[r], *run.events(r), True).encode() for r in range(len(lens)))

    job = gpu.Job(0)
    job.set_event_params(_params(gpu, p))
    job.stage([blow5.svb_zd_encode(r) for r in reads], dig, off, rng, counts=[r.size for r in reads], ids=ids)
    job.launch(gpu.TOOL_EVENT)
    ev = job.wait()["events"]
    for r in range(len(lens)):
        _same(M.Events(*ev[r]), run.events(r), "job read %d" % r)
    job.launch(gpu.TOOL_EVENT, flags=gpu.JOB_EVENTS_COMPACT)
    ev = job.wait()["events"]
    for r in range(len(lens)):
        assert np.array_equal(ev[r].start, run.events(r).start) and np.array_equal(ev[r].length, run.events(r).length)
    job.launch(gpu.TOOL_EVENT, flags=gpu.JOB_EVENTS_LENGTHS)
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
    want, _ = gpu.event(reads, dig, off, rng, 1)
    for r in range(len(lens)):
        _same(M.Events(*ev[r]), M.Events(*want[r]), "presets again, read %d" % r)
    # out of domain: refused, the job keeps what it had
    with pytest.raises(Exception):
        job.set_event_params(gpu.EventParams(1, 6, 1.0, 1.0, 1.0, 0))
    job.close()


# ------------------------------------------------------------------------------------------------ 9. CLI

def _cli():
    from sigtk_amd import build
    assert os.path.exists(build.CLI), "sigtk-amd is not built"
    return build.CLI


def test_cli_detector_with_the_preset_is_the_golden(gpu):
    path = os.path.join(GOLDEN, "sp1_dna.blow5")
    out = subprocess.run([_cli(), "event", "-c", "--detector", "3,6,1.4,9,0.2", path], capture_output=True, check=True).stdout
    assert out == open(os.path.join(GOLDEN, "sp1_dna.event_c.tsv"), "rb").read()


@pytest.mark.parametrize("gpu_text", [False, True])
def test_cli_detector_off_preset(gpu, oracle, sp1, gpu_text):
    p = M.GRID_OFF[1]
    path = os.path.join(GOLDEN, "sp1_dna.blow5")
    arg = "%d,%d,1.4,3,0.2" % (p.w1, p.w2)
    cmd = [_cli(), "event", "-c", "--detector", arg] + (["--gpu-text"] if gpu_text else []) + [path]
    out = subprocess.run(cmd, capture_output=True, check=True).stdout.decode().split("\n")
    assert out[0].startswith("read_id\t")
    for r, rd in enumerate(sp1.reads[:10]):
        want = M.events_raw(oracle, rd.raw, rd.digitisation, rd.offset, rd.range, p)
        f = out[1 + r].split("\t")
        assert f[0] == rd.read_id and int(f[1]) == rd.raw.size
        lengths = np.array([int(x) for x in f[5].rstrip(",").split(",")], dtype=np.uint32)
        assert int(f[4]) == want.start.size
        assert np.array_equal(lengths, want.length), rd.read_id
        assert np.array_equal(np.cumsum(lengths) - lengths, want.start), rd.read_id
        assert (int(f[2]), int(f[3])) == (0, rd.raw.size)
