"""Device-resident batches on top of the C ABI.  torch is used only as the allocator / stream
provider (plumbing): every compute call goes through libsigtk_gpu.so with raw device pointers
and the current torch HIP stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import api


def _stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


@dataclass
class DeviceReads:
    """A batch of reads resident in HBM (sgk_batch_t view + owning tensors)."""
    samples: torch.Tensor   # int16 [n_samples]
    offsets: torch.Tensor   # int64 (uint64 bits) [n_reads]
    lengths: torch.Tensor   # int32 (uint32 bits) [n_reads]
    dig: torch.Tensor       # float64 [n_reads]
    off: torch.Tensor
    rng: torch.Tensor
    n_reads: int
    max_read_len: int
    n_samples: int
    offsets_host: np.ndarray
    lengths_host: np.ndarray

    def view(self) -> api.Batch:
        return api.Batch(_ptr(self.samples), _ptr(self.offsets), _ptr(self.lengths), _ptr(self.dig),
                         _ptr(self.off), _ptr(self.rng), self.n_reads, self.max_read_len, self.n_samples)

    @property
    def total_samples(self) -> int:
        return int(self.lengths_host.astype(np.int64).sum())

    def normalise(self, method: int, y: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
        """sgk_normalise: the batch's pA signal normalised (api.NORM_ZSCORE / api.NORM_MEDMAD) -> (y, records): y a
        float32 tensor of the samples' layout (y[offsets[r] + i]; what lies outside the reads is left as it was), records
        a uint8 tensor holding n_reads sgk_norm_rec_t (view it with api.NORM_DTYPE)."""
        L = api._float_lib()
        dev = self.samples.device
        if y is None:
            y = torch.zeros(self.n_samples, dtype=torch.float32, device=dev)
        rec = torch.zeros(max(self.n_reads, 1) * api.NORM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        if ws is None:
            n = int(L.sgk_normalise_workspace_bytes(self.n_reads, self.n_samples, self.max_read_len))
            ws = torch.zeros(max(n, 64), dtype=torch.uint8, device=dev)
        view = self.view()
        api.check(L.sgk_normalise(C.addressof(view), int(method), _ptr(y), _ptr(rec), _ptr(ws), ws.numel(), _stream_ptr()),
                  "sgk_normalise")
        return y, rec


def alloc_reads(lengths: np.ndarray, device: torch.device, align: int = 64, leads=None) -> DeviceReads:
    """Lay out reads of the given lengths with every read starting on an `align`-sample boundary, or, with `leads`,
    leads[r] samples behind it (the padding grows with the lead: reads never overlap)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.size
    lead = np.zeros(n, dtype=np.int64) if leads is None else np.asarray(leads, dtype=np.int64)
    assert lead.size == n and (n == 0 or int(lead.min()) >= 0)
    padded = (lengths + lead + align - 1) // align * align
    # 64 samples of head room and tail room: the event fast path reads a little outside each read
    offsets = np.full(n, 256, dtype=np.int64)
    if n > 1:
        offsets[1:] += np.cumsum(padded[:-1])
    offsets += lead
    n_samples = ((int(padded.sum()) if n else 0) + 320 + 7) // 8 * 8   # the ABI wants a multiple of 8
    return DeviceReads(
        samples=torch.zeros(n_samples, dtype=torch.int16, device=device),
        offsets=torch.from_numpy(offsets).to(device),
        lengths=torch.from_numpy(lengths.astype(np.int32)).to(device),
        dig=torch.zeros(max(n, 1), dtype=torch.float64, device=device),
        off=torch.zeros(max(n, 1), dtype=torch.float64, device=device),
        rng=torch.zeros(max(n, 1), dtype=torch.float64, device=device),
        n_reads=n, max_read_len=int(lengths.max()) if n else 0, n_samples=n_samples,
        offsets_host=offsets.astype(np.uint64), lengths_host=lengths.astype(np.uint32))


def synth_reads(n_reads: int, read_len: int, seed: int, kind: int, device: torch.device,
                first_read: int = 0, lengths=None) -> DeviceReads:
    """Synthetic reads generated on the device (same generator as api.synth_reads_host); `lengths` (one per read)
    replaces the common `read_len`."""
    L = api.load_library()
    lens = np.full(n_reads, read_len, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    b = alloc_reads(lens, device)
    api.check(L.sgk_synth_reads(_ptr(b.samples), _ptr(b.offsets), _ptr(b.lengths), _ptr(b.dig), _ptr(b.off),
                                _ptr(b.rng), b.n_reads, b.max_read_len, first_read, seed, kind, _stream_ptr()),
              "sgk_synth_reads")
    return b


def upload_reads(reads, dig, off, rng, device: torch.device) -> DeviceReads:
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    b = alloc_reads(lens, device)
    host = np.zeros(b.n_samples, dtype=np.int16)
    for r, raw in enumerate(reads):
        o = int(b.offsets_host[r])
        host[o:o + len(raw)] = raw
    b.samples.copy_(torch.from_numpy(host))
    b.dig[:b.n_reads] = torch.from_numpy(np.asarray(dig, dtype=np.float64))
    b.off[:b.n_reads] = torch.from_numpy(np.asarray(off, dtype=np.float64))
    b.rng[:b.n_reads] = torch.from_numpy(np.asarray(rng, dtype=np.float64))
    return b


class EventArena:
    """Output arena + workspace of sgk_event for one batch shape (allocated once, reused)."""

    def __init__(self, b: DeviceReads, params: Optional["api.EventParams"] = None):
        """`params`: size the workspace for sgk_event_param with these detector parameters as well (by their route,
        api.event_params_route: sgk_event_opt's workspace for a preset and for the presets' kernels with run-time
        thresholds, the generic kernel's otherwise -- sgk_event_workspace_bytes_param decides)"""
        L = api.load_library()
        dev = b.samples.device
        slots = np.zeros(b.n_reads + 1, dtype=np.int64)
        np.cumsum(api.event_slots_for(b.lengths_host), out=slots[1:])
        self.slots_host = slots
        self.n_slots = int(slots[-1])
        self.slots = torch.from_numpy(slots).to(dev)
        # sgk_event_rec_t[n_slots]: (start u32, length u32, mean f32, stdv f32) per slot
        self.events = torch.empty((max(self.n_slots, 1), 4), dtype=torch.int32, device=dev)
        assert self.events.data_ptr() % 16 == 0
        self.n_events = torch.zeros(max(b.n_reads, 1), dtype=torch.int32, device=dev)
        # (sized for the options of the call that follows: api.EVENT_OPTIONS as they are now)
        self.opt = api.EventOptions.from_buffer_copy(bytes(api.EVENT_OPTIONS))
        self.ws_bytes = int(L.sgk_event_workspace_bytes_opt(b.n_reads, b.n_samples, b.max_read_len, C.byref(self.opt)))
        if params is not None:
            self.ws_bytes = max(self.ws_bytes, self.param_workspace_bytes(b, params))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        assert self.ws.data_ptr() % 64 == 0

    def param_workspace_bytes(self, b: DeviceReads, params: "api.EventParams") -> int:
        params.check()
        return int(api.load_library().sgk_event_workspace_bytes_param(b.n_reads, b.n_samples, b.max_read_len,
                                                                     C.byref(self.opt), C.byref(params)))

    def ensure_workspace(self, nbytes: int) -> None:
        if nbytes > self.ws_bytes:
            self.ws_bytes = int(nbytes)
            self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.ws.device)
            assert self.ws.data_ptr() % 64 == 0

    def status(self) -> api.EventStatus:
        L = api.load_library()
        st = api.EventStatus()
        rc = L.sgk_event_status(_ptr(self.ws), C.byref(st), _stream_ptr())
        if rc != api.SGK_OK and rc != api.SGK_ERR_CAPACITY:
            api.check(rc, "sgk_event_status")
        return st

    def read_events(self, r: int) -> api.Events:
        k = int(self.n_events[r].item())
        s = int(self.slots_host[r])
        rec = self.events[s:s + k].cpu().numpy()
        return api.Events(rec[:, 0].copy().view(np.uint32), rec[:, 1].copy().view(np.uint32),
                          rec[:, 2].copy().view(np.float32), rec[:, 3].copy().view(np.float32))

    # column views of the record array (device tensors; mean / stdv as float32)
    @property
    def start(self) -> torch.Tensor:
        return self.events[:, 0]

    @property
    def length(self) -> torch.Tensor:
        return self.events[:, 1]

    @property
    def mean(self) -> torch.Tensor:
        return self.events.view(torch.float32)[:, 2]

    @property
    def stdv(self) -> torch.Tensor:
        return self.events.view(torch.float32)[:, 3]


def event(b: DeviceReads, arena: EventArena, rna: int, params: Optional["api.EventParams"] = None) -> None:
    """Enqueue one pass of the event path over the batch on the current stream (async).  With `params` the detector
    takes the caller's parameters (sgk_event_param) and `rna` is ignored; the arena's workspace grows when it was not
    sized for them.  `params.preset_kernels()` opts in to the presets' kernels with run-time thresholds (windows 3/6 and
    7/14, threshold2 >= 9); the arena's options (`arena.opt`) apply there as they do to the presets."""
    L = api.load_library()
    view = b.view()
    if params is not None:
        arena.ensure_workspace(arena.param_workspace_bytes(b, params))
        api.check(L.sgk_event_param(C.byref(view), C.byref(params), _ptr(arena.slots), _ptr(arena.events),
                                    _ptr(arena.n_events), _ptr(arena.ws), arena.ws_bytes, _stream_ptr(),
                                    C.byref(arena.opt)), "sgk_event_param")
        return
    api.check(L.sgk_event_opt(C.byref(view), int(rna), _ptr(arena.slots), _ptr(arena.events), _ptr(arena.n_events),
                              _ptr(arena.ws), arena.ws_bytes, _stream_ptr(), C.byref(arena.opt)), "sgk_event_opt")


def event_pa(pa: torch.Tensor, b: DeviceReads, arena: EventArena, rna: int,
             params: Optional["api.EventParams"] = None) -> None:
    """The event path on pA floats laid out like the batch's samples (sgk_event_pa_opt / sgk_event_pa_param)."""
    L = api.load_library()
    assert pa.dtype == torch.float32 and pa.numel() >= b.n_samples and pa.data_ptr() % 16 == 0
    if params is not None:
        arena.ensure_workspace(arena.param_workspace_bytes(b, params))
        api.check(L.sgk_event_pa_param(_ptr(pa), _ptr(b.offsets), _ptr(b.lengths), b.n_reads, b.max_read_len,
                                       b.n_samples, C.byref(params), _ptr(arena.slots), _ptr(arena.events),
                                       _ptr(arena.n_events), _ptr(arena.ws), arena.ws_bytes, _stream_ptr(),
                                       C.byref(arena.opt)), "sgk_event_pa_param")
        return
    api.check(L.sgk_event_pa_opt(_ptr(pa), _ptr(b.offsets), _ptr(b.lengths), b.n_reads, b.max_read_len, b.n_samples,
                                 int(rna), _ptr(arena.slots), _ptr(arena.events), _ptr(arena.n_events), _ptr(arena.ws),
                                 arena.ws_bytes, _stream_ptr(), C.byref(arena.opt)), "sgk_event_pa_opt")


# ---------------------------------------------------------------------- stat / jnn / prefix / pa (device API)

def _workspace(b: "DeviceReads", size_fn_name: str) -> torch.Tensor:
    """the workspace sgk_<tool>_workspace_bytes asks for (counters + the longest-first dispatch order of the
    wave-per-read kernels), allocated once per batch"""
    cache = b.__dict__.setdefault("_ws_cache", {})
    if size_fn_name not in cache:
        L = api.load_library()
        n = int(getattr(L, size_fn_name)(b.n_reads, b.n_samples, b.max_read_len))
        cache[size_fn_name] = torch.zeros(max(n, 64), dtype=torch.uint8, device=b.samples.device)
    return cache[size_fn_name]


def long_status(b: "DeviceReads", tool: str = "stat", ws: Optional[torch.Tensor] = None) -> "api.LongStatus":
    """sgk_stat_long_status of the workspace the last stat / prefix call on this batch used (jnn: pass arena.ws);
    synchronises"""
    if ws is None:
        ws = _workspace(b, "sgk_%s_workspace_bytes" % tool)
    torch.cuda.synchronize()
    st = api.LongStatus()
    api.check(api.load_library().sgk_stat_long_status(_ptr(ws), ws.numel(), b.n_reads, C.byref(st)), "sgk_stat_long_status")
    return st


def literal_status(b: "DeviceReads", tool: str = "stat") -> "api.LiteralStatus":
    """sgk_stat_literal_status of the workspace the last stat / prefix call on this batch used; synchronises"""
    ws = _workspace(b, "sgk_%s_workspace_bytes" % tool)
    torch.cuda.synchronize()
    st = api.LiteralStatus()
    api.check(api.load_library().sgk_stat_literal_status(_ptr(ws), ws.numel(), b.n_reads, C.byref(st)), "sgk_stat_literal_status")
    return st


def stat(b: DeviceReads) -> torch.Tensor:
    """sgk_stat -> uint8 tensor holding n_reads sgk_stat_rec_t (view it with api.STAT_DTYPE)."""
    L = api.load_library()
    out = torch.zeros(max(b.n_reads, 1) * api.STAT_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
    view = b.view()
    ws = _workspace(b, "sgk_stat_workspace_bytes")
    api.check(L.sgk_stat_opt(C.byref(view), _ptr(out), _ptr(ws), ws.numel(), _stream_ptr(), C.byref(api.STAT_OPTIONS)),
              "sgk_stat_opt")
    return out


def stat_pa(b: DeviceReads, pa_out: Optional[torch.Tensor] = None):
    """sgk_stat_pa (BASELINE config 4): stat records + pA of every sample in one launch sequence; the pA values
    are written by the median pass.  -> (stat record bytes, pa tensor laid out like b.samples)"""
    L = api.load_library()
    out = torch.zeros(max(b.n_reads, 1) * api.STAT_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
    if pa_out is None:
        pa_out = torch.empty(b.n_samples, dtype=torch.float32, device=b.samples.device)
    view = b.view()
    ws = _workspace(b, "sgk_stat_workspace_bytes")
    api.check(L.sgk_stat_pa_opt(C.byref(view), _ptr(out), _ptr(pa_out), _ptr(ws), ws.numel(), _stream_ptr(),
                                C.byref(api.STAT_OPTIONS)), "sgk_stat_pa_opt")
    return out, pa_out


def pipeline(b: DeviceReads, arena: "EventArena", rna: int, pa_out: Optional[torch.Tensor] = None,
             stat_out: Optional[torch.Tensor] = None):
    """sgk_pipeline (BASELINE config 5): pa -> event -> stat over one resident batch; the event builder writes the pA.
    -> (stat record bytes, pa tensor laid out like b.samples); events land in `arena`"""
    L = api.load_library()
    if stat_out is None:
        stat_out = torch.zeros(max(b.n_reads, 1) * api.STAT_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
    if pa_out is None:
        pa_out = torch.empty(b.n_samples, dtype=torch.float32, device=b.samples.device)
    view = b.view()
    ws = _workspace(b, "sgk_stat_workspace_bytes")
    api.check(L.sgk_pipeline(C.byref(view), int(rna), _ptr(arena.slots), _ptr(arena.events), _ptr(arena.n_events), _ptr(pa_out),
                             _ptr(stat_out), _ptr(arena.ws), arena.ws_bytes, _ptr(ws), ws.numel(), _stream_ptr(),
                             C.byref(arena.opt), C.byref(api.STAT_OPTIONS)), "sgk_pipeline")
    return stat_out, pa_out


def prefix(b: DeviceReads, rna: int, pore: int, params: "api.PrefixParams" = None) -> torch.Tensor:
    """sgk_prefix_opt, or with `params` sgk_prefix_param (`pore` is then ignored: the sets are the caller's)"""
    L = api.load_library()
    out = torch.zeros(max(b.n_reads, 1) * api.PREFIX_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
    view = b.view()
    ws = _workspace(b, "sgk_prefix_workspace_bytes")
    if params is not None:
        api.check(api._param_lib().sgk_prefix_param(C.byref(view), int(rna), C.byref(params), _ptr(out), _ptr(ws), ws.numel(),
                                                    _stream_ptr(), C.addressof(api.STAT_OPTIONS)), "sgk_prefix_param")
        return out
    api.check(L.sgk_prefix_opt(C.byref(view), int(rna), int(pore), _ptr(out), _ptr(ws), ws.numel(), _stream_ptr(),
                               C.byref(api.STAT_OPTIONS)), "sgk_prefix_opt")
    return out


class SegArena:
    def __init__(self, b: DeviceReads):
        dev = b.samples.device
        slots = np.zeros(b.n_reads + 1, dtype=np.int64)
        np.cumsum(b.lengths_host.astype(np.int64) // 32 + 2, out=slots[1:])
        self.slots_host = slots
        self.slots = torch.from_numpy(slots).to(dev)
        self.x = torch.empty(max(int(slots[-1]), 1), dtype=torch.int32, device=dev)
        self.y = torch.empty(max(int(slots[-1]), 1), dtype=torch.int32, device=dev)
        self.n_segs = torch.zeros(max(b.n_reads, 1), dtype=torch.int32, device=dev)
        n = int(api.load_library().sgk_jnn_workspace_bytes(b.n_reads, b.n_samples, b.max_read_len))
        self.ws = torch.zeros(max(n, 64), dtype=torch.uint8, device=dev)


def jnn(b: DeviceReads, arena: SegArena, rna: int, params: "api.JnnParam" = None) -> None:
    """sgk_jnn_opt, or with `params` sgk_jnn_param (`rna` is then ignored)"""
    L = api.load_library()
    view = b.view()
    if params is not None:
        api.check(api._param_lib().sgk_jnn_param(C.byref(view), C.byref(params), _ptr(arena.slots), _ptr(arena.x), _ptr(arena.y),
                                                 _ptr(arena.n_segs), _ptr(arena.ws), arena.ws.numel(), _stream_ptr(),
                                                 C.addressof(api.STAT_OPTIONS)), "sgk_jnn_param")
        return
    api.check(L.sgk_jnn_opt(C.byref(view), int(rna), _ptr(arena.slots), _ptr(arena.x), _ptr(arena.y),
                            _ptr(arena.n_segs), _ptr(arena.ws), arena.ws.numel(), _stream_ptr(), C.byref(api.STAT_OPTIONS)),
              "sgk_jnn_opt")


# ---------------------------------------- float (pA) batches: sgk_stat_f32, sgk_jnn_f32, sgk_normalise_f32, sgk_sdtw_f32
@dataclass
class FloatReads:
    """A batch of float signals resident in HBM: read r is x[offsets[r] : offsets[r] + lengths[r]], at any element
    offset.  `x` may be a view that starts at any element of its storage (4-byte alignment is all the library asks)."""
    x: torch.Tensor         # float32 [n_values]
    offsets: torch.Tensor   # int64 (uint64 bits) [n_reads]
    lengths: torch.Tensor   # int32 (uint32 bits) [n_reads]
    n_reads: int
    max_read_len: int
    n_values: int
    offsets_host: np.ndarray
    lengths_host: np.ndarray

    def view(self):
        """the six leading arguments of sgk_stat_f32 / sgk_jnn_f32"""
        return (_ptr(self.x), _ptr(self.offsets), _ptr(self.lengths), self.n_reads, self.max_read_len, self.n_values)

    def normalise_f32(self, method: int, y: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
        """sgk_normalise_f32 (api.NORM_ZSCORE / api.NORM_MEDMAD) -> (y, records).  y: a float32 tensor of x's layout --
        x itself normalises in place, None allocates one (zeros outside the reads); nothing of it outside the reads is
        written.  records: a uint8 tensor holding n_reads sgk_norm_rec_t (view it with api.NORM_DTYPE)."""
        L = api._float_lib()
        if y is None:
            y = torch.zeros_like(self.x)
        rec = torch.zeros(max(self.n_reads, 1) * api.NORM_DTYPE.itemsize, dtype=torch.uint8, device=self.x.device)
        if ws is None:
            ws = _float_workspace(self, "sgk_normalise_f32_workspace_bytes")
        api.check(L.sgk_normalise_f32(*self.view(), int(method), _ptr(y), _ptr(rec), _ptr(ws), ws.numel(), _stream_ptr()),
                  "sgk_normalise_f32")
        return y, rec


def float_reads(x: torch.Tensor, offsets, lengths) -> FloatReads:
    """A float batch over values that are on the device already (pA from sgk_pa, a normalised signal ...)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert x.dtype == torch.float32 and x.is_contiguous() and offsets.size == lengths.size
    assert lengths.size == 0 or (int(lengths.min()) >= 0 and int((offsets + lengths).max()) <= x.numel())
    n = max(lengths.size, 1)
    off_d = torch.zeros(n, dtype=torch.int64, device=x.device)
    len_d = torch.zeros(n, dtype=torch.int32, device=x.device)
    off_d[:offsets.size] = torch.from_numpy(offsets)
    len_d[:lengths.size] = torch.from_numpy(lengths.astype(np.int32))
    return FloatReads(x=x, offsets=off_d, lengths=len_d, n_reads=int(lengths.size),
                      max_read_len=int(lengths.max()) if lengths.size else 0, n_values=int(x.numel()),
                      offsets_host=offsets.astype(np.uint64), lengths_host=lengths.astype(np.uint32))


def upload_float_reads(arrays, device: torch.device, leads=None, fill=None) -> FloatReads:
    """Float arrays packed one behind the other.  leads[r] is the number of gap elements in front of read r (default
    0: the reads touch), `fill` what the gaps hold (default 0.0).  The allocation ends with the last read."""
    arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    lens = np.array([a.size for a in arrays], dtype=np.int64)
    lead = np.zeros(lens.size, dtype=np.int64) if leads is None else np.asarray(leads, dtype=np.int64)
    assert lead.size == lens.size and (lens.size == 0 or int(lead.min()) >= 0)
    offsets = np.cumsum(lead + lens) - lens
    host = np.full(int((lead + lens).sum()), 0.0 if fill is None else fill, dtype=np.float32)
    for a, o in zip(arrays, offsets.tolist()):
        host[o:o + a.size] = a
    return float_reads(torch.from_numpy(host).to(device), offsets, lens)


def _float_workspace(fb: FloatReads, size_fn_name: str) -> torch.Tensor:
    n = int(getattr(api._float_lib(), size_fn_name)(fb.n_reads, fb.n_values, fb.max_read_len))
    return torch.zeros(max(n, 64), dtype=torch.uint8, device=fb.x.device)


def stat_f32(fb: FloatReads, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sgk_stat_f32 -> uint8 tensor holding n_reads sgk_statf_rec_t (view it with api.STATF_DTYPE)."""
    L = api._float_lib()
    out = torch.zeros(max(fb.n_reads, 1) * api.STATF_DTYPE.itemsize, dtype=torch.uint8, device=fb.x.device)
    if ws is None:
        ws = _float_workspace(fb, "sgk_stat_f32_workspace_bytes")
    api.check(L.sgk_stat_f32(*fb.view(), _ptr(out), _ptr(ws), ws.numel(), _stream_ptr()), "sgk_stat_f32")
    return out


def sdtw_workspace(queries: FloatReads, targets: FloatReads) -> torch.Tensor:
    n = int(api._float_lib().sgk_sdtw_f32_workspace_bytes(queries.n_reads, queries.max_read_len, targets.n_reads,
                                                          targets.max_read_len))
    return torch.zeros(max(n, 64), dtype=torch.uint8, device=queries.x.device)


def sdtw_f32(queries: FloatReads, targets: FloatReads, options: int = 0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sgk_sdtw_f32: every query aligned against every target (subsequence DTW; api.SDTW_NO_START drops `start`) ->
    uint8 tensor holding n_queries x n_targets sgk_sdtw_rec_t, record [qi * n_targets + ti] (view it with
    api.SDTW_DTYPE)."""
    L = api._float_lib()
    out = torch.zeros(max(queries.n_reads * targets.n_reads, 1) * api.SDTW_DTYPE.itemsize, dtype=torch.uint8,
                      device=queries.x.device)
    if ws is None:
        ws = sdtw_workspace(queries, targets)
    api.check(L.sgk_sdtw_f32(*queries.view(), *targets.view(), int(options), _ptr(out), _ptr(ws), ws.numel(), _stream_ptr()),
              "sgk_sdtw_f32")
    return out


class FloatSegArena:
    """The segment arena of sgk_jnn_f32 (SegArena's layout): sgk_jnn_slots_for(n) slots per read, or the caller's
    `slots` (n_reads + 1 increasing slot indices)."""

    def __init__(self, fb: FloatReads, slots=None):
        dev = fb.x.device
        if slots is None:
            slots = np.zeros(fb.n_reads + 1, dtype=np.int64)
            np.cumsum(fb.lengths_host.astype(np.int64) // 32 + 2, out=slots[1:])
        slots = np.asarray(slots, dtype=np.int64)
        assert slots.size == fb.n_reads + 1
        self.slots_host = slots
        self.slots = torch.from_numpy(slots).to(dev)
        self.x = torch.empty(max(int(slots[-1]), 1), dtype=torch.int32, device=dev)
        self.y = torch.empty(max(int(slots[-1]), 1), dtype=torch.int32, device=dev)
        self.n_segs = torch.zeros(max(fb.n_reads, 1), dtype=torch.int32, device=dev)
        self.ws = _float_workspace(fb, "sgk_jnn_f32_workspace_bytes")

    def n_overflowed(self) -> int:
        """reads whose segments overflowed their slots in the last call (synchronises)"""
        return int(self.ws[:4].cpu().numpy().view(np.uint32)[0])


def jnn_f32(fb: FloatReads, arena: FloatSegArena, params: "api.JnnParam", top: Optional[torch.Tensor] = None,
            bot: Optional[torch.Tensor] = None) -> None:
    """sgk_jnn_f32: jnn_pa of every read with `params`; top / bot (float32 tensors, one value per read) give each read
    its own fixed thresholds (params.std_scale <= 0)."""
    L = api._float_lib()
    api.check(L.sgk_jnn_f32(*fb.view(), C.byref(params), _ptr(top), _ptr(bot), _ptr(arena.slots), _ptr(arena.x),
                            _ptr(arena.y), _ptr(arena.n_segs), _ptr(arena.ws), arena.ws.numel(), _stream_ptr()),
              "sgk_jnn_f32")


def pa(b: DeviceReads, out: torch.Tensor) -> None:
    L = api.load_library()
    view = b.view()
    api.check(L.sgk_pa(C.byref(view), _ptr(out), _stream_ptr()), "sgk_pa")


# ---------------------------------------------------------------------- svb-zd decode (device API)

def svbzd_decode(blobs, counts, device: torch.device, blob_leads=None, sample_leads=None, fill=None):
    """Decode svb-zd signal blobs (bytes objects) on the device.  Blob r starts on a 16-byte boundary of the blob buffer,
    or blob_leads[r] (0 - 15) bytes behind one, and the bytes between the blobs are then 0xC3, not 0; read r starts
    sample_leads[r] samples behind its aligned slot (alloc_reads); fill: the int16 the sample arena holds before the launch.
    -> (DeviceReads with the decoded samples and zeroed scaling, status tensor [n_reads] int32)"""
    L = api.load_library()
    n = len(blobs)
    blens = np.array([len(b) for b in blobs], dtype=np.uint32)
    lead = np.zeros(n, dtype=np.int64) if blob_leads is None else np.asarray(blob_leads, dtype=np.int64)
    assert lead.size == n and (n == 0 or (0 <= int(lead.min()) and int(lead.max()) <= 15))
    boffs = np.zeros(n, dtype=np.int64)
    pos = 0
    for i in range(n):
        boffs[i] = (pos + 15) // 16 * 16 + int(lead[i])   # blob starts: 16-byte aligned + lead
        pos = int(boffs[i]) + int(blens[i])
    total = pos
    # (at least 4 readable bytes behind the last blob: the kernel's aligned dword loads end past it)
    host = np.full(max(total + 16, 16), 0 if blob_leads is None else 0xC3, dtype=np.uint8)
    for i, b in enumerate(blobs):
        host[int(boffs[i]):int(boffs[i]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    d_blobs = torch.from_numpy(host).to(device)
    assert _ptr(d_blobs) % 16 == 0
    d_boffs = torch.from_numpy(boffs).to(device)
    d_blens = torch.from_numpy(blens.astype(np.int32)).to(device)
    reads = alloc_reads(np.asarray(counts, dtype=np.int64), device, leads=sample_leads)
    if fill is not None:
        reads.samples.fill_(int(np.int16(fill)))
    status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=device)
    api.check(L.sgk_svbzd_decode(_ptr(d_blobs), _ptr(d_boffs), _ptr(d_blens), n, _ptr(reads.samples),
                                 _ptr(reads.offsets), _ptr(reads.lengths), _ptr(status), _stream_ptr()),
              "sgk_svbzd_decode")
    return reads, status


# ---------------------------------------------------------------------- text SLOW5 signal parse (device API)

def sigtext_decode(texts, counts, device: torch.device):
    """Parse SLOW5 raw_signal text columns (bytes objects) on the device; counts[r] = the samples read r announces.
    Every column starts 16-byte aligned; the arena has 16 bytes of padding at both ends.
    -> (DeviceReads with the parsed samples and zeroed scaling, status tensor [n_reads] int32)"""
    L = api.load_library()
    n = len(texts)
    tlens = np.array([len(t) for t in texts], dtype=np.uint32)
    toffs = np.zeros(n, dtype=np.int64)
    pos = 16
    for i in range(n):
        pos = (pos + 15) // 16 * 16
        toffs[i] = pos
        pos += int(tlens[i])
    host = np.zeros((pos + 15) // 16 * 16 + 16, dtype=np.uint8)
    for i, t in enumerate(texts):
        host[int(toffs[i]):int(toffs[i]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d_text = torch.from_numpy(host).to(device)
    d_toffs = torch.from_numpy(toffs).to(device)
    d_tlens = torch.from_numpy(tlens.astype(np.int32)).to(device)
    reads = alloc_reads(np.asarray(counts, dtype=np.int64), device)
    status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=device)
    api.check(L.sgk_sigtext_decode(_ptr(d_text), _ptr(d_toffs), _ptr(d_tlens), n, _ptr(reads.samples),
                                   _ptr(reads.offsets), _ptr(reads.lengths), _ptr(status), _stream_ptr()),
              "sgk_sigtext_decode")
    return reads, status


class Slow5TextWriter:
    """sgk_slow5_text_measure + sgk_slow5_text_write over one resident batch, in the manner of TextWriter: row r is
    heads[r] | the samples of read r as decimal numbers joined by ',' | tails[r] (heads / tails: one bytes object per
    read, or None for all empty).  measure() and write() only enqueue; status() synchronises.  ws_bytes overrides the
    workspace size (tests)."""

    def __init__(self, b: DeviceReads, heads=None, tails=None, ws_bytes: Optional[int] = None):
        L = api.load_library()
        dev = b.samples.device
        self.b = b
        self._keep = []

        def ids(parts):
            if parts is None:
                return None
            raw = [bytes(p) for p in parts]
            assert len(raw) == b.n_reads
            offs = np.zeros(b.n_reads + 1, dtype=np.int64)
            np.cumsum([len(p) for p in raw], out=offs[1:])
            d_bytes = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
            d_offs = torch.from_numpy(offs.astype(np.uint32).view(np.int32)).to(dev)
            self._keep += [d_bytes, d_offs]
            return api.TextIds(_ptr(d_bytes), _ptr(d_offs))

        self.heads, self.tails = ids(heads), ids(tails)
        self.ws_bytes = int(L.sgk_slow5_text_workspace_bytes(b.n_reads, b.n_samples)) if ws_bytes is None else int(ws_bytes)
        self.ws = torch.zeros(self.ws_bytes + 16, dtype=torch.uint8, device=dev)
        self.row_offsets = torch.zeros(b.n_reads + 1, dtype=torch.int64, device=dev)

    def _rows(self):
        b = self.b
        return (_ptr(b.samples), _ptr(b.offsets), _ptr(b.lengths), b.n_reads,
                C.byref(self.heads) if self.heads is not None else None, C.byref(self.tails) if self.tails is not None else None)

    def measure(self) -> int:
        return int(api.load_library().sgk_slow5_text_measure(*self._rows(), _ptr(self.row_offsets), _ptr(self.ws),
                                                             self.ws_bytes, _stream_ptr()))

    def write(self, text: torch.Tensor, capacity: Optional[int] = None) -> int:
        """text: uint8 tensor (or a view of one starting at any byte); capacity defaults to its length"""
        return int(api.load_library().sgk_slow5_text_write(*self._rows(), _ptr(text),
                                                           int(text.numel() if capacity is None else capacity),
                                                           _ptr(self.ws), self.ws_bytes, _stream_ptr()))

    def status(self):
        """-> (return code of sgk_text_status: 0, api.SGK_ERR_CAPACITY or api.SGK_ERR_WORKSPACE; api.TextStatus); synchronises"""
        torch.cuda.synchronize()
        st = api.TextStatus()
        return int(api.load_library().sgk_text_status(_ptr(self.ws), C.byref(st))), st

    def run(self) -> bytes:
        """measure, allocate exactly, write -> the rows as bytes (and self.row_offsets_host)"""
        api.check(self.measure(), "sgk_slow5_text_measure")
        torch.cuda.synchronize()
        self.row_offsets_host = self.row_offsets.cpu().numpy().astype(np.uint64)
        total = int(self.row_offsets_host[-1])
        text = torch.zeros(max(total, 1), dtype=torch.uint8, device=self.b.samples.device)
        api.check(self.write(text, total), "sgk_slow5_text_write")
        rc, _ = self.status()
        api.check(rc, "sgk_slow5_text_write")
        return text[:total].cpu().numpy().tobytes()


# ---------------------------------------------------------------------- qts + svb-zd encode (device API)

def qts(b: DeviceReads, bits: int, method: int) -> None:
    """sgk_qts: quantise the samples of every read in place (method 0 floor, 1 round, 2 fill-ones)."""
    L = api.load_library()
    api.check(L.sgk_qts(_ptr(b.samples), _ptr(b.offsets), _ptr(b.lengths), b.n_reads, b.max_read_len, int(bits),
                        int(method), _stream_ptr()), "sgk_qts")


def svbzd_encode(b: DeviceReads, blob_leads=None, fill: int = 0, with_gaps: bool = False):
    """sgk_svbzd_size + sgk_svbzd_encode -> list of blobs (bytes), one per read.  Blob r starts on an 8-byte boundary of
    the output buffer, or with blob_leads (each 0, 4, 8 or 12) blob_leads[r] bytes behind a 16-byte boundary; the buffer
    is pre-filled with `fill`.  with_gaps: -> (blobs, gaps, lengths): gaps[0] the bytes in front of the first blob,
    gaps[r + 1] those between the end of blob r and the start of the next (the end of the buffer, 16 bytes or more, for
    the last), which no blob may write; lengths: what sgk_svbzd_size reported"""
    L = api.load_library()
    dev = b.samples.device
    n = b.n_reads
    blens = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    api.check(L.sgk_svbzd_size(_ptr(b.samples), _ptr(b.offsets), _ptr(b.lengths), n, _ptr(blens), _stream_ptr()),
              "sgk_svbzd_size")
    torch.cuda.synchronize()
    lens = blens[:n].cpu().numpy().astype(np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    if blob_leads is None:
        np.cumsum((lens + 7) // 8 * 8, out=offs[1:])
    else:
        lead = np.asarray(blob_leads, dtype=np.int64)
        assert lead.size == n and all(int(v) in (0, 4, 8, 12) for v in lead)
        pos = 0
        for r in range(n):
            offs[r] = (pos + 15) // 16 * 16 + int(lead[r])
            pos = int(offs[r]) + int(lens[r])
        offs[n] = pos
    size = max(int(offs[-1]), 8) + (16 if with_gaps else 0)
    blobs = torch.full((size,), int(fill), dtype=torch.uint8, device=dev)
    assert _ptr(blobs) % 16 == 0
    d_offs = torch.from_numpy(offs[:n].copy() if n else np.zeros(1, dtype=np.int64)).to(dev)
    api.check(L.sgk_svbzd_encode(_ptr(b.samples), _ptr(b.offsets), _ptr(b.lengths), n, _ptr(blobs), _ptr(d_offs),
                                 _ptr(blens), _stream_ptr()), "sgk_svbzd_encode")
    torch.cuda.synchronize()
    host = blobs.cpu().numpy()
    out = [host[int(offs[r]):int(offs[r]) + int(lens[r])].tobytes() for r in range(n)]
    if with_gaps:
        ends = [0] + [int(offs[r]) + int(lens[r]) for r in range(n)]
        starts = [int(offs[r]) for r in range(n)] + [size]
        return out, [host[e:s].tobytes() for e, s in zip(ends, starts)], lens
    return out


def inflate_input_offsets(streams, leads=None):
    """where inflate() puts every stream in its input buffer (whose start is 4-byte aligned) -> (byte offsets, total):
    at odd offsets on purpose, the kernel aligns its dword reads itself; leads[r] in 0 - 3 (None: any) asks for
    offset % 4 == leads[r], for streams built for one alignment of their first byte"""
    in_off = np.zeros(len(streams), dtype=np.uint64)
    pos = 0
    for r, s in enumerate(streams):
        if leads is not None and leads[r] is not None:
            pos += (int(leads[r]) - pos) & 3
        in_off[r] = pos
        pos += len(s) + (r % 3)
    return in_off, pos


def inflate(streams, caps=None, device: Optional[torch.device] = None, with_gaps: bool = False, leads=None):
    """sgk_inflate over a list of zlib streams (bytes) -> (list of inflated bytes as kept: the first caps[r] of each,
    out_lengths, status) -- the device-side replacement of slow5lib's per-record uncompress().  with_gaps: a fourth
    result, the bytes of the (zero-filled) output buffer between caps[r] and the next stream's 16-byte aligned area,
    which no stream may write; leads: see inflate_input_offsets"""
    L = api.load_library()
    dev = device or torch.device("cuda", 0)
    n = len(streams)
    in_len = np.asarray([len(s) for s in streams], dtype=np.uint32)
    in_off, pos = inflate_input_offsets(streams, leads)
    blob = np.zeros((pos + 7) // 4 * 4 + 4, dtype=np.uint8)
    for r, s in enumerate(streams):
        blob[int(in_off[r]):int(in_off[r]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    caps_a = np.asarray(caps if caps is not None else [1 << 20] * n, dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        out_off[1:] = np.cumsum((caps_a[:-1].astype(np.uint64) + 15) // 16 * 16)
    total = int(out_off[-1] + (int(caps_a[-1]) + 15) // 16 * 16) if n else 16
    d_in = torch.from_numpy(blob).to(dev)
    assert _ptr(d_in) % 4 == 0
    d_ioff = torch.from_numpy(in_off.view(np.int64)).to(dev)
    d_ilen = torch.from_numpy(in_len.view(np.int32)).to(dev)
    d_out = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
    d_ooff = torch.from_numpy(out_off.view(np.int64)).to(dev)
    d_caps = torch.from_numpy(caps_a.view(np.int32)).to(dev)
    d_olen = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    api.check(L.sgk_inflate(_ptr(d_in), _ptr(d_ioff), _ptr(d_ilen), n, _ptr(d_out), _ptr(d_ooff), _ptr(d_caps), _ptr(d_olen),
                            _ptr(d_st), _stream_ptr()), "sgk_inflate")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    olen = d_olen.cpu().numpy().view(np.uint32)[:n]
    st = d_st.cpu().numpy()[:n]
    kept = [out[int(out_off[r]):int(out_off[r]) + min(int(olen[r]), int(caps_a[r]))].tobytes() for r in range(n)]
    if with_gaps:
        ends = [int(out_off[r + 1]) if r + 1 < n else total for r in range(n)]
        return kept, olen, st, [out[int(out_off[r]) + int(caps_a[r]):ends[r]].tobytes() for r in range(n)]
    return kept, olen, st


def deflate_bound(n: int) -> int:
    """sgk_deflate_bound: bytes that always hold the zlib stream sgk_deflate writes for n input bytes (no GPU needed)"""
    return int(api.load_library().sgk_deflate_bound(int(n)))


def deflate(streams, caps=None, device: Optional[torch.device] = None, with_gaps: bool = False, fill: int = 0,
            in_shift=None):
    """sgk_deflate over a list of byte strings -> (list of zlib streams as written: out_lengths[r] bytes each, none for a
    stream with a non-zero status, out_lengths, status) -- the device-side replacement of compress2().  caps[r]: room
    for stream r (default: deflate_bound); the output buffer is pre-filled with `fill`.  with_gaps: a fourth result, per
    stream the bytes of the output buffer from out_lengths[r] (0 for a failed stream) up to the next stream's 16-byte
    aligned area, which the stream must have left alone, a fifth: the byte offset of caps[r] in that gap.  in_shift[r]
    (0 .. 15, default 0): stream r's input lies that many bytes behind a 16-byte boundary of the input buffer"""
    L = api.load_library()
    dev = device or torch.device("cuda", 0)
    n = len(streams)
    in_len = np.asarray([len(s) for s in streams], dtype=np.uint32)
    shift = np.asarray(in_shift if in_shift is not None else [0] * n, dtype=np.uint64)
    assert shift.size == n and (n == 0 or int(shift.max()) <= 15)
    in_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        in_off[1:] = np.cumsum((in_len[:-1].astype(np.uint64) + shift[:-1] + 15) // 16 * 16)
    in_off += shift
    pos = int(in_off[-1]) + int(in_len[-1]) if n else 0
    blob = np.zeros((pos + 19) // 16 * 16, dtype=np.uint8)
    for r, s in enumerate(streams):
        blob[int(in_off[r]):int(in_off[r]) + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    caps_a = np.asarray(caps if caps is not None else [deflate_bound(len(s)) for s in streams], dtype=np.uint32)
    gap = 48 if with_gaps else 0   # (room that belongs to no stream)
    out_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        out_off[1:] = np.cumsum((caps_a[:-1].astype(np.uint64) + 15) // 16 * 16 + gap)
    total = int(out_off[-1] + (int(caps_a[-1]) + 15) // 16 * 16 + gap) if n else 16
    d_in = torch.from_numpy(blob).to(dev)
    assert _ptr(d_in) % 16 == 0
    d_ioff = torch.from_numpy(in_off.view(np.int64)).to(dev)
    d_ilen = torch.from_numpy(in_len.view(np.int32)).to(dev)
    d_out = torch.full((max(total, 16),), fill, dtype=torch.uint8, device=dev)
    assert _ptr(d_out) % 16 == 0
    d_ooff = torch.from_numpy(out_off.view(np.int64)).to(dev)
    d_caps = torch.from_numpy(caps_a.view(np.int32)).to(dev)
    d_olen = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    api.check(L.sgk_deflate(_ptr(d_in), _ptr(d_ioff), _ptr(d_ilen), n, _ptr(d_out), _ptr(d_ooff), _ptr(d_caps), _ptr(d_olen),
                            _ptr(d_st), _stream_ptr()), "sgk_deflate")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    st = d_st.cpu().numpy()[:n]
    olen = d_olen.cpu().numpy().view(np.uint32)[:n].copy()
    kept = [out[int(out_off[r]):int(out_off[r]) + int(olen[r])].tobytes() if st[r] == 0 else None for r in range(n)]
    if with_gaps:
        ends = [int(out_off[r + 1]) if r + 1 < n else total for r in range(n)]
        used = [int(olen[r]) if st[r] == 0 else 0 for r in range(n)]
        return (kept, olen, st, [out[int(out_off[r]) + used[r]:ends[r]].tobytes() for r in range(n)],
                [int(caps_a[r]) - used[r] for r in range(n)])
    return kept, olen, st


def zstd_decompress(frames, caps=None, device: Optional[torch.device] = None, with_gaps: bool = False, leads=None,
                    fill: int = 0, guard: int = 0):
    """sgk_zstd_decompress over a list of zstd frames (bytes) -> (list of decoded bytes as kept, out_lengths, status) --
    the device-side replacement of slow5lib's per-record ZSTD_decompress().  caps, with_gaps and leads as inflate().
    The output buffer starts out as `fill` bytes, and `guard` more bytes (a multiple of 16) lie between a frame's room and
    the next frame's: with_gaps returns what is there after the launch, for tests that look for stray writes."""
    L = api.load_library()
    dev = device or torch.device("cuda", 0)
    n = len(frames)
    in_len = np.asarray([len(s) for s in frames], dtype=np.uint32)
    in_off, pos = inflate_input_offsets(frames, leads)
    blob = np.zeros((pos + 7) // 4 * 4 + 4, dtype=np.uint8)
    for r, s in enumerate(frames):
        blob[int(in_off[r]):int(in_off[r]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    caps_a = np.asarray(caps if caps is not None else [1 << 20] * n, dtype=np.uint32)
    assert guard % 16 == 0
    out_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        out_off[1:] = np.cumsum((caps_a[:-1].astype(np.uint64) + 15) // 16 * 16 + np.uint64(guard))
    total = int(out_off[-1]) + (int(caps_a[-1]) + 15) // 16 * 16 + guard if n else 16
    d_in = torch.from_numpy(blob).to(dev)
    assert _ptr(d_in) % 4 == 0
    d_ioff = torch.from_numpy(in_off.view(np.int64)).to(dev)
    d_ilen = torch.from_numpy(in_len.view(np.int32)).to(dev)
    d_out = torch.full((max(total, 16),), fill, dtype=torch.uint8, device=dev)
    d_ooff = torch.from_numpy(out_off.view(np.int64)).to(dev)
    d_caps = torch.from_numpy(caps_a.view(np.int32)).to(dev)
    d_olen = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    api.check(L.sgk_zstd_decompress(_ptr(d_in), _ptr(d_ioff), _ptr(d_ilen), n, _ptr(d_out), _ptr(d_ooff), _ptr(d_caps),
                                    _ptr(d_olen), _ptr(d_st), _stream_ptr()), "sgk_zstd_decompress")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    olen = d_olen.cpu().numpy().view(np.uint32)[:n]
    st = d_st.cpu().numpy()[:n]
    kept = [out[int(out_off[r]):int(out_off[r]) + min(int(olen[r]), int(caps_a[r]))].tobytes() for r in range(n)]
    if with_gaps:
        ends = [int(out_off[r + 1]) if r + 1 < n else total for r in range(n)]
        return kept, olen, st, [out[int(out_off[r]) + int(caps_a[r]):ends[r]].tobytes() for r in range(n)]
    return kept, olen, st


def zrec_tail_check(inflated: torch.Tensor, rec_offsets: torch.Tensor, rec_lengths: torch.Tensor,
                    tail_offsets: torch.Tensor, fields, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sgk_zrec_tail_check over torch buffers on one device: inflated uint8; rec_offsets int64 (uint64 bits);
    rec_lengths / tail_offsets int32 (uint32 bits), one entry per record; fields: the file's auxiliary columns
    (api.AuxField objects or (elem_bytes, is_array) pairs -- a host table).  -> status, int32 per record (enqueued on the
    current stream, not synchronised)"""
    L = api.load_library()
    n = int(rec_offsets.numel())
    assert inflated.dtype == torch.uint8 and rec_offsets.dtype == torch.int64
    assert rec_lengths.dtype == torch.int32 and tail_offsets.dtype == torch.int32
    assert int(rec_lengths.numel()) == n and int(tail_offsets.numel()) == n
    if status is None:
        status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=inflated.device)
    api.check(L.sgk_zrec_tail_check(_ptr(inflated), _ptr(rec_offsets), _ptr(rec_lengths), _ptr(tail_offsets), n,
                                    api.aux_table(fields), len(fields), _ptr(status), _stream_ptr()), "sgk_zrec_tail_check")
    return status


def sigraw_unit_samples() -> int:
    """sgk_sigraw_unit_samples: the samples one work unit of sigraw_gather moves (host arithmetic)"""
    return int(api.load_library().sgk_sigraw_unit_samples())


def sigraw_gather(records: torch.Tensor, rec_offsets: torch.Tensor, rec_lengths: torch.Tensor, sig_offsets: torch.Tensor,
                  samples: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, max_read_len: int,
                  rec_status: Optional[torch.Tensor] = None, n_samples: Optional[int] = None,
                  status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sgk_sigraw_gather over torch buffers on one device: records uint8 (16-byte aligned, readable to the next multiple
    of 16 behind every record); rec_offsets / offsets int64 (uint64 bits); rec_lengths / sig_offsets / lengths / rec_status
    int32 (uint32 bits), one entry per read; samples int16, written in place at offsets[r] (multiples of 8).  n_samples
    defaults to the arena's size.  -> status, int32 per read (enqueued on the current stream, not synchronised)"""
    L = api.load_library()
    n = int(rec_offsets.numel())
    assert records.dtype == torch.uint8 and samples.dtype == torch.int16
    assert rec_offsets.dtype == torch.int64 and offsets.dtype == torch.int64
    for t in (rec_lengths, sig_offsets, lengths) + ((rec_status,) if rec_status is not None else ()):
        assert t.dtype == torch.int32 and int(t.numel()) == n
    assert int(offsets.numel()) == n
    if status is None:
        status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=records.device)
    api.check(L.sgk_sigraw_gather(_ptr(records), _ptr(rec_offsets), _ptr(rec_lengths), _ptr(sig_offsets), _ptr(rec_status), n,
                                  _ptr(samples), _ptr(offsets), _ptr(lengths), int(max_read_len),
                                  int(samples.numel()) if n_samples is None else int(n_samples), _ptr(status), _stream_ptr()),
              "sgk_sigraw_gather")
    return status


# ---------------------------------------------------------------------- TSV rows written on the device (sgk_text_*)

class TextWriter:
    """sgk_text_measure + sgk_text_write over one resident batch: ids, workspace and row offsets on the device.

    kind: api.TEXT_PA (rows from the batch's int16 samples) or api.TEXT_EVENT / api.TEXT_EVENT_COMPACT (rows from the
    arena a device.event() call filled).  measure() and write() only enqueue; status() synchronises."""

    def __init__(self, b: DeviceReads, ids, kind: int, arena: Optional[EventArena] = None):
        L = api.load_library()
        dev = b.samples.device
        raw = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
        assert len(raw) == b.n_reads
        offs = np.zeros(b.n_reads + 1, dtype=np.int64)
        np.cumsum([len(i) for i in raw], out=offs[1:])
        blob = np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()
        self.b, self.kind, self.arena = b, int(kind), arena
        self.id_bytes = torch.from_numpy(blob).to(dev)
        self.id_offs = torch.from_numpy(offs.astype(np.int32)).to(dev)
        self.ids = api.TextIds(_ptr(self.id_bytes), _ptr(self.id_offs))
        items = b.n_samples if kind == api.TEXT_PA else arena.n_slots
        self.ws_bytes = int(L.sgk_text_workspace_bytes(self.kind, b.n_reads, items))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.row_offsets = torch.zeros(b.n_reads + 1, dtype=torch.int64, device=dev)

    def _arena_ptrs(self):
        a = self.arena
        return (_ptr(a.slots), _ptr(a.events), _ptr(a.n_events)) if a is not None else (None, None, None)

    def measure(self) -> None:
        view = self.b.view()
        api.check(api.load_library().sgk_text_measure(self.kind, C.byref(view), C.byref(self.ids), *self._arena_ptrs(),
                                                      _ptr(self.row_offsets), _ptr(self.ws), self.ws_bytes, _stream_ptr()),
                  "sgk_text_measure")

    def write(self, text: torch.Tensor, capacity: Optional[int] = None) -> None:
        """text: uint8 tensor (or a view of one starting at any byte); capacity defaults to its length"""
        view = self.b.view()
        api.check(api.load_library().sgk_text_write(self.kind, C.byref(view), C.byref(self.ids), *self._arena_ptrs(),
                                                    _ptr(text), int(text.numel() if capacity is None else capacity),
                                                    _ptr(self.ws), self.ws_bytes, _stream_ptr()), "sgk_text_write")

    def status(self):
        """-> (return code of sgk_text_status: 0 or api.SGK_ERR_CAPACITY, api.TextStatus); synchronises"""
        torch.cuda.synchronize()
        st = api.TextStatus()
        rc = api.load_library().sgk_text_status(_ptr(self.ws), C.byref(st))
        if rc not in (api.SGK_OK, api.SGK_ERR_CAPACITY):
            api.check(rc, "sgk_text_status")
        return rc, st

    def run(self) -> bytes:
        """measure, allocate exactly, write -> the rows as bytes (and self.row_offsets_host)"""
        self.measure()
        torch.cuda.synchronize()
        self.row_offsets_host = self.row_offsets.cpu().numpy().astype(np.uint64)
        total = int(self.row_offsets_host[-1])
        text = torch.zeros(max(total, 1), dtype=torch.uint8, device=self.b.samples.device)
        self.write(text, total)
        rc, _ = self.status()
        api.check(rc, "sgk_text_write")
        return text[:total].cpu().numpy().tobytes()


# ---------------------------------------------------------------------- sref: synthetic reference signal (sgk_sref_*)

class SrefBatch:
    """Sequences (bytes, as read from a FASTA file), their names and a pore model (`levels`: 4^k float32 by k-mer rank)
    on the device, with the spans api.sref_spans cuts their rows into (max_span / cuts force seams)."""

    def __init__(self, seqs, names, levels, k: int, rna: bool = False, max_span: Optional[int] = None, cuts=None,
                 table_in_lds: bool = False, device: Optional[torch.device] = None):
        dev = device or torch.device("cuda", torch.cuda.current_device())
        levels = np.ascontiguousarray(levels, dtype=np.float32)
        assert levels.size == 4 ** k, "the model must hold 4^k levels"
        seqs = [bytes(s) for s in seqs]
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        assert len(raw) == len(seqs)
        self.spans_host, self.row_of_span = api.sref_spans([len(s) for s in seqs], k, rna, max_span, cuts)
        self.n_spans = int(self.spans_host.size)
        self.n_positions = int(self.spans_host["count"].astype(np.int64).sum()) if self.n_spans else 0
        blob = np.frombuffer(b"".join(seqs) + b"\0" * 16, dtype=np.uint8).copy()
        self.n_bases = blob.size - 16
        self.bases = torch.from_numpy(blob).to(dev)
        self.spans = torch.from_numpy(np.frombuffer(self.spans_host.tobytes() + b"\0" * 40, dtype=np.uint8).copy()).to(dev)
        self.levels = torch.from_numpy(levels.view(np.int32).copy()).to(dev)
        offs = np.zeros(len(raw) + 1, dtype=np.int64)
        np.cumsum([len(n) for n in raw], out=offs[1:])
        self.name_bytes = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.name_offs = torch.from_numpy(offs.astype(np.int32)).to(dev)
        self.names = api.TextIds(_ptr(self.name_bytes), _ptr(self.name_offs))
        self.k, self.device, self.table_in_lds = int(k), dev, bool(table_in_lds)

    def view(self) -> api.SrefBatch:
        return api.SrefBatch(_ptr(self.bases), self.n_bases, _ptr(self.spans), self.n_spans, self.k, _ptr(self.levels),
                             int(self.table_in_lds), 0)


def sref_levels(seqs, levels, k: int, rna: bool = False, max_span: Optional[int] = None, cuts=None,
                device: Optional[torch.device] = None, batch: Optional[SrefBatch] = None, to_host: bool = True):
    """sgk_sref_levels -> one float32 array per row ('+' then, unless rna, '-' of every sequence), its spans joined;
    to_host=False: the device tensor of all rows back to back, not synchronised"""
    b = batch or SrefBatch(seqs, [b""] * len(seqs), levels, k, rna, max_span, cuts, device=device)
    counts = b.spans_host["count"].astype(np.int64) if b.n_spans else np.zeros(0, dtype=np.int64)
    offs = np.zeros(b.n_spans + 1, dtype=np.int64)
    np.cumsum(counts, out=offs[1:])
    d_offs = torch.from_numpy(offs).to(b.device)
    out = torch.zeros(max(int(offs[-1]), 1), dtype=torch.float32, device=b.device)
    view = b.view()
    api.check(api.load_library().sgk_sref_levels(C.byref(view), _ptr(d_offs), _ptr(out), _stream_ptr()), "sgk_sref_levels")
    if not to_host:
        return out
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    n_rows = int(b.row_of_span[-1]) + 1 if b.n_spans else 0
    row_lo = np.searchsorted(b.row_of_span, np.arange(n_rows), side="left")
    row_hi = np.searchsorted(b.row_of_span, np.arange(n_rows), side="right")
    return [flat[int(offs[lo]):int(offs[hi])].copy() for lo, hi in zip(row_lo, row_hi)]


class SrefText(SrefBatch):
    """sgk_sref_text_measure + sgk_sref_text_write over one resident batch of spans, in the manner of TextWriter:
    measure() and write() only enqueue; status() synchronises; row_offsets has n_spans + 1 entries."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        L = api.load_library()
        self.ws_bytes = int(L.sgk_sref_text_workspace_bytes(self.n_spans, self.n_positions))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.row_offsets = torch.zeros(self.n_spans + 1, dtype=torch.int64, device=self.device)

    def measure(self) -> None:
        view = self.view()
        api.check(api.load_library().sgk_sref_text_measure(C.byref(view), C.byref(self.names), _ptr(self.row_offsets),
                                                           _ptr(self.ws), self.ws_bytes, _stream_ptr()), "sgk_sref_text_measure")

    def write(self, text: torch.Tensor, capacity: Optional[int] = None) -> None:
        view = self.view()
        api.check(api.load_library().sgk_sref_text_write(C.byref(view), C.byref(self.names), _ptr(text),
                                                         int(text.numel() if capacity is None else capacity), _ptr(self.ws),
                                                         self.ws_bytes, _stream_ptr()), "sgk_sref_text_write")

    def status(self):
        """-> (return code of sgk_text_status: 0 or api.SGK_ERR_CAPACITY, api.TextStatus); synchronises"""
        torch.cuda.synchronize()
        st = api.TextStatus()
        rc = api.load_library().sgk_text_status(_ptr(self.ws), C.byref(st))
        if rc not in (api.SGK_OK, api.SGK_ERR_CAPACITY):
            api.check(rc, "sgk_text_status")
        return rc, st

    def run(self) -> bytes:
        """measure, allocate exactly, write -> the rows as bytes (and self.row_offsets_host)"""
        self.measure()
        torch.cuda.synchronize()
        self.row_offsets_host = self.row_offsets.cpu().numpy().astype(np.uint64)
        total = int(self.row_offsets_host[-1])
        text = torch.zeros(max(total, 1), dtype=torch.uint8, device=self.device)
        self.write(text, total)
        rc, _ = self.status()
        api.check(rc, "sgk_sref_text_write")
        return text[:total].cpu().numpy().tobytes()


# ---------------------------------------------------------------------- ss paf2tsv (sgk_ss_*)

SS_CANARY = 0x5a5a5a5a


class SsBatch:
    """Records of `ss paf2tsv` on the device.  A record is any object with the attributes rid, ss (bytes), start_raw,
    end_raw, st_k, end_k, tlen and rna (tests/ss_model.py: Record).  Its k-mer range is cut into spans by api.ss_spans
    (max_span / cuts), or `spans` gives them.  aligns[r] in 0..15: the byte alignment of string r in the buffer (default
    r % 16); the bytes between strings are digits, so a read outside a string would show.  gap: pair-table entries left
    between the spans' ranges and at both ends, filled with SS_CANARY; the ranges themselves are filled with -1."""

    def __init__(self, records, max_span: Optional[int] = None, cuts=None, spans=None, aligns=None, gap: int = 0,
                 device: Optional[torch.device] = None):
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.device, self.records = dev, list(records)
        n = len(self.records)
        rec = np.zeros(n, dtype=api.SS_RECORD_DTYPE)
        pos, chunks = 16, [b"7" * 16]
        for r, x in enumerate(self.records):
            al = int(aligns[r]) if aligns is not None else r % 16
            pad = (-pos) % 16 + al
            chunks.append(b"7" * pad)
            pos += pad
            rec[r] = (pos, len(x.ss), x.start_raw, x.end_raw, x.st_k, x.end_k, x.tlen, x.rna, r)
            chunks.append(bytes(x.ss))
            pos += len(x.ss)
        chunks.append(b"7" * ((-pos) % 16 + 16))
        blob = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        self.n_ss_bytes = blob.size - 16
        self.records_host = rec
        self.spans_host = np.asarray(spans, dtype=api.SS_SPAN_DTYPE) if spans is not None else \
            api.ss_spans([x.end_k - x.st_k for x in self.records], max_span, cuts)
        self.n_records, self.n_spans = n, int(self.spans_host.size)
        counts = self.spans_host["count"].astype(np.int64) if self.n_spans else np.zeros(0, dtype=np.int64)
        self.n_rows = int(counts.sum())
        self.offsets_host = np.zeros(self.n_spans, dtype=np.int64)
        pos = gap
        table = np.full((gap + self.n_rows + (self.n_spans + 1) * gap + 2, 2), SS_CANARY, dtype=np.int32)
        for s in range(self.n_spans):
            self.offsets_host[s] = pos
            table[pos:pos + int(counts[s])] = -1
            pos += int(counts[s]) + gap
        self.table_filled = table.copy()
        self.ss = torch.from_numpy(blob).to(dev)
        assert _ptr(self.ss) % 16 == 0
        self.recs = torch.from_numpy(np.frombuffer(rec.tobytes() + b"\0" * 40, dtype=np.uint8).copy()).to(dev)
        self.spans = torch.from_numpy(np.frombuffer(self.spans_host.tobytes() + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.offsets = torch.from_numpy(np.concatenate([self.offsets_host, [0]])).to(dev)
        self.pairs = torch.from_numpy(table).to(dev)
        self.status = torch.full((max(self.n_spans, 1),), -1, dtype=torch.int32, device=dev)
        self.ends = torch.full((max(self.n_spans, 1), 2), -7, dtype=torch.int32, device=dev)
        raw = [bytes(x.rid) for x in self.records]
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(i) for i in raw], out=offs[1:])
        self.id_bytes = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.id_offs = torch.from_numpy(offs.astype(np.int32)).to(dev)
        self.ids = api.TextIds(_ptr(self.id_bytes), _ptr(self.id_offs))

    def view(self) -> api.SsBatch:
        return api.SsBatch(_ptr(self.ss), self.n_ss_bytes, _ptr(self.recs), _ptr(self.spans), self.n_records, self.n_spans)

    def decode(self) -> None:
        """sgk_ss_decode over the spans (enqueued, not synchronised)"""
        view = self.view()
        api.check(api.load_library().sgk_ss_decode(C.byref(view), _ptr(self.offsets), _ptr(self.pairs), _ptr(self.status),
                                                   _ptr(self.ends), _stream_ptr()), "sgk_ss_decode")


def ss_decode(records, max_span: Optional[int] = None, cuts=None, spans=None, aligns=None, gap: int = 0,
              device: Optional[torch.device] = None, validate: bool = False):
    """sgk_ss_decode -> (pairs: one int32 array [count, 2] per span, status [n_spans] uint32, ends [n_spans, 2] int32,
    the SsBatch: .table_filled is the pair table as it was before the call, .table_after as it is now, .offsets_host where
    each span's range starts).  validate=True: the spans == NULL form, one result per record and nothing stored."""
    b = SsBatch(records, max_span, cuts, spans, aligns, gap, device)
    if validate:
        b.status = torch.full((max(b.n_records, 1),), -1, dtype=torch.int32, device=b.device)
        b.ends = torch.full((max(b.n_records, 1), 2), -7, dtype=torch.int32, device=b.device)
        view = api.SsBatch(_ptr(b.ss), b.n_ss_bytes, _ptr(b.recs), None, b.n_records, 0)
        api.check(api.load_library().sgk_ss_decode(C.byref(view), None, None, _ptr(b.status), _ptr(b.ends), _stream_ptr()),
                  "sgk_ss_decode")
        n_out = b.n_records
    else:
        b.decode()
        n_out = b.n_spans
    torch.cuda.synchronize()
    b.table_after = b.pairs.cpu().numpy()
    pairs = [b.table_after[int(o):int(o) + int(c)].copy() for o, c in zip(b.offsets_host, b.spans_host["count"])] \
        if b.n_spans else []
    return pairs, b.status.cpu().numpy().view(np.uint32)[:n_out], b.ends.cpu().numpy()[:n_out], b


class SsText(SsBatch):
    """sgk_ss_decode, then sgk_ss_text_measure + sgk_ss_text_write over one resident batch of spans, in the manner of
    SrefText: row_offsets has n_spans + 1 entries.  rows_capacity: what the workspace is sized for (default: the rows)."""

    def __init__(self, *args, rows_capacity: Optional[int] = None, **kw):
        super().__init__(*args, **kw)
        L = api.load_library()
        self.ws_bytes = int(L.sgk_ss_text_workspace_bytes(self.n_spans, self.n_rows if rows_capacity is None else rows_capacity))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.row_offsets = torch.zeros(self.n_spans + 1, dtype=torch.int64, device=self.device)
        self.decode()

    def measure(self) -> None:
        view = self.view()
        api.check(api.load_library().sgk_ss_text_measure(C.byref(view), _ptr(self.offsets), _ptr(self.pairs), C.byref(self.ids),
                                                         _ptr(self.row_offsets), _ptr(self.ws), self.ws_bytes, _stream_ptr()),
                  "sgk_ss_text_measure")

    def write(self, text: torch.Tensor, capacity: Optional[int] = None) -> None:
        view = self.view()
        api.check(api.load_library().sgk_ss_text_write(C.byref(view), _ptr(self.offsets), _ptr(self.pairs), C.byref(self.ids),
                                                       _ptr(text), int(text.numel() if capacity is None else capacity),
                                                       _ptr(self.ws), self.ws_bytes, _stream_ptr()), "sgk_ss_text_write")

    def status_text(self):
        """-> (return code of sgk_text_status: 0, api.SGK_ERR_CAPACITY or api.SGK_ERR_WORKSPACE; api.TextStatus); synchronises"""
        torch.cuda.synchronize()
        st = api.TextStatus()
        return api.load_library().sgk_text_status(_ptr(self.ws), C.byref(st)), st

    def run(self) -> bytes:
        """measure, allocate exactly, write -> the rows as bytes (and self.row_offsets_host)"""
        self.measure()
        torch.cuda.synchronize()
        self.row_offsets_host = self.row_offsets.cpu().numpy().astype(np.uint64)
        total = int(self.row_offsets_host[-1])
        text = torch.zeros(max(total, 1), dtype=torch.uint8, device=self.device)
        self.write(text, total)
        rc, _ = self.status_text()
        api.check(rc, "sgk_ss_text_write")
        return text[:total].cpu().numpy().tobytes()


def ss_text(records, max_span: Optional[int] = None, cuts=None, spans=None, aligns=None,
            device: Optional[torch.device] = None):
    """the rows of the spans written on the device -> (bytes, row_offsets [n_spans + 1] uint64)"""
    t = SsText(records, max_span, cuts, spans, aligns, device=device)
    text = t.run()
    return text, t.row_offsets_host


def text_numbers(values: np.ndarray):
    """sgk_text_numbers_f32 / _i64 (by dtype): printf("%f") / "%ld" of every value, made on the device
    -> (uint8 array [n, 48] of the slots, filled with '#' beforehand; uint8 array [n] of the byte counts)"""
    L = api.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    values = np.ascontiguousarray(values)
    n = values.size
    if values.dtype == np.float32:
        d_v = torch.from_numpy(values.view(np.int32)).to(dev)
        fn = L.sgk_text_numbers_f32
    else:
        d_v = torch.from_numpy(values.astype(np.int64)).to(dev)
        fn = L.sgk_text_numbers_i64
    slots = torch.full((max(n, 1) * 48,), 35, dtype=torch.uint8, device=dev)
    lens = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    api.check(fn(_ptr(d_v), n, _ptr(slots), _ptr(lens), _stream_ptr()), "sgk_text_numbers")
    torch.cuda.synchronize()
    return slots.cpu().numpy().reshape(-1, 48)[:n], lens.cpu().numpy()[:n]
