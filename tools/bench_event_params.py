#!/usr/bin/env python3
"""Time the generic event kernel (k_event_param: caller-supplied detector parameters) against the presets' own kernels
on the same device-resident batch, in one process: for each batch shape sgk_event_opt on both presets, k_event_param on
both presets (SGK_EVENT_PARAMS_GENERIC) and on two off-preset sets.  Every side is warmed up, then timed --steps times
with device events around one call each; the median is reported, with the ratio generic / preset and the workspace
bytes.  The generic kernel's events on the presets are compared with sgk_event_opt's (the counts of every read and
every record of every read's used slots) before anything is timed.  One JSON line per batch shape; what
profiles/event_params.md quotes.

The fast route (SGK_EVENT_PARAMS_PRESET_KERNELS: the presets' kernels with run-time thresholds) is timed beside them: per
preset its numbers moved by one ulp (the preset's work through the <.., RT = true> instances) and one tuned set, each
against k_event_param on the same set and batch -- after the two routes' counts and records have been compared.
--no-generic-grid leaves out the off-preset sets of the generic kernel.

    python tools/bench_event_params.py [--shapes 10000x100000,1000x100000] [--steps 5] [--warmup 1] [--no-generic-grid]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sigtk_amd import api, device

OFF_PRESET = [(5, 9, 1.4, 3.0, 0.2), (3, 20, 1.4, 2.0, 0.2)]
#: per preset: a tuned set of the fast domain (the preset's numbers moved by one ulp are formed from the preset)
TUNED = {0: (3, 6, 1.0, 9.0, 0.1), 1: (7, 14, 1.5, 12.0, 0.5)}


def one_ulp_off(rna):
    """the preset's thresholds and peak height, each one float up: another parameter set, the same work"""
    p = api.EventParams.preset(rna)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    return (p.window_length1, p.window_length2, up(p.threshold1), up(p.threshold2), up(p.peak_height))


def used_slots(arena):
    """mask over the arena's slots: slot s of read r is used when s - slots[r] < n_events[r]"""
    n = arena.slots.numel() - 1
    idx = torch.arange(arena.n_slots, device=arena.slots.device)
    read = torch.searchsorted(arena.slots, idx, right=True) - 1
    return (idx - arena.slots[read]) < arena.n_events[:n].to(torch.int64)[read]


def same_records(x, y, what):
    """every record of every read's used slots is the same in both arenas; otherwise: where they differ"""
    used = used_slots(x)
    bad = torch.nonzero((x.events != y.events).any(dim=1) & used).flatten()
    if bad.numel() == 0:
        return
    reads = torch.unique(torch.searchsorted(x.slots, bad, right=True) - 1)
    s = int(bad[0].item())
    raise AssertionError("%s: %d records of %d reads differ (reads %s ...); first at slot %d: %s against %s" % (
        what, bad.numel(), reads.numel(), reads[:8].tolist(), s, x.events[s].tolist(), y.events[s].tolist()))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x100000,1000x100000", help="READSxSAMPLES, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-generic-grid", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    api.load_library()
    for shape in a.shapes.split(","):
        n_reads, read_len = (int(x) for x in shape.split("x"))
        res = {"reads": n_reads, "read_len": read_len, "steps": a.steps, "warmup": a.warmup, "sides": {}}
        for rna in (0, 1):
            b = device.synth_reads(n_reads, read_len, seed=1, kind=rna, device=dev)
            arena = device.EventArena(b)
            p = api.EventParams.preset(rna).generic()
            garena = device.EventArena(b, params=p)
            device.event(b, arena, rna)
            device.event(b, garena, rna, params=p)
            torch.cuda.synchronize()
            assert torch.equal(arena.n_events, garena.n_events), "generic kernel: other event counts than the preset's"
            used = used_slots(arena)
            assert torch.equal(arena.events[used], garena.events[used]), "generic kernel: other records than the preset's"
            del used
            st, gst = arena.status(), garena.status()
            assert st.n_events_total == gst.n_events_total
            med, ms = timed(lambda: device.event(b, arena, rna), a.steps, a.warmup)
            gmed, gms = timed(lambda: device.event(b, garena, rna, params=p), a.steps, a.warmup)
            res["sides"]["preset%d" % rna] = {"ms": round(med, 3), "all_ms": [round(x, 3) for x in ms],
                                               "workspace_bytes": int(arena.ws_bytes), "events": int(st.n_events_total)}
            res["sides"]["generic_preset%d" % rna] = {"ms": round(gmed, 3), "all_ms": [round(x, 3) for x in gms],
                                                       "workspace_bytes": int(garena.param_workspace_bytes(b, p)),
                                                       "rerun_chunks": int(gst.n_rerun_passes),
                                                       "ratio_generic_over_preset": round(gmed / med, 2)}
            if rna == 0 and not a.no_generic_grid:
                for q in OFF_PRESET:
                    p2 = api.EventParams(*q)
                    a2 = device.EventArena(b, params=p2)
                    m2, ms2 = timed(lambda: device.event(b, a2, 0, params=p2), a.steps, a.warmup)
                    s2 = a2.status()
                    res["sides"]["generic_%d_%d_%g_%g_%g" % q] = {
                        "ms": round(m2, 3), "all_ms": [round(x, 3) for x in ms2],
                        "workspace_bytes": int(a2.param_workspace_bytes(b, p2)), "events": int(s2.n_events_total),
                        "rerun_chunks": int(s2.n_rerun_passes), "overflow": int(s2.n_capacity_overflow),
                        "samples_per_s": round(n_reads * read_len / (m2 * 1e-3), 0)}
                    del a2
            # the fast route against the generic kernel on the same set and batch
            for tag, q in (("ulp", one_ulp_off(rna)), ("tuned", TUNED[rna])):
                pf = api.EventParams(*q, api.SGK_EVENT_PARAMS_PRESET_KERNELS)
                pg = api.EventParams(*q, api.SGK_EVENT_PARAMS_GENERIC)
                assert pf.route() == api.SGK_EVENT_ROUTE_PRESET_WINDOWS and pg.route() == api.SGK_EVENT_ROUTE_GENERIC
                fa = device.EventArena(b, params=pf)
                device.event(b, fa, rna, params=pf)
                device.event(b, garena, rna, params=pg)
                torch.cuda.synchronize()
                assert torch.equal(fa.n_events, garena.n_events), "fast route: other event counts than the generic kernel's"
                same_records(fa, garena, "fast route (%s, preset %d) against the generic kernel" % (tag, rna))
                fmed, fms = timed(lambda: device.event(b, fa, rna, params=pf), a.steps, a.warmup)
                fst = fa.status()
                g2, gms2 = timed(lambda: device.event(b, garena, rna, params=pg), a.steps, a.warmup)
                res["sides"]["rt_%s%d" % (tag, rna)] = {
                    "params": list(q), "ms": round(fmed, 3), "all_ms": [round(x, 3) for x in fms],
                    "workspace_bytes": int(fa.param_workspace_bytes(b, pf)), "events": int(fst.n_events_total),
                    "fallback_reads": int(fst.n_fallback_reads), "rerun_chunks": int(fst.n_rerun_passes),
                    "rt_over_preset": round(fmed / med, 3), "generic_ms": round(g2, 3),
                    "generic_all_ms": [round(x, 3) for x in gms2], "generic_over_rt": round(g2 / fmed, 2)}
                del fa
            del arena, garena, b
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
