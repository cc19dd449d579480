#!/usr/bin/env python3
"""Times stat and jnn on batches of float (pA) signals (profiles/float_signals.md):

    python tools/bench_float_signals.py [--shapes 10000x100000,200000x5000] [--runs 5] [--sample 8] [--json out.json]

Per shape, on pA of the benchmark's synthetic DNA reads (made and converted on the device):
  1. sgk_stat_f32, sgk_jnn_f32 with the DNA preset, and sgk_jnn_f32 with a fixed-threshold set whose error >= corrector,
     which takes the literal loop (one read per lane); with the HBM bytes the passes move (passes x 4 B per value) and
     the share of the HBM peak (8 TB/s) that comes to;
  2. what a caller had before the batch entry points: the per-read shims in a loop (sgk_meanf + sgk_stdvf + sgk_medianf,
     sgk_jnn_pa) over `--sample` reads, wall clock, SCALED to the batch;
  3. as a yardstick, sgk_stat and sgk_jnn_param on the int16 reads the floats were made from.
HIP events around each call after one warm-up call, the median of `--runs` runs.

    python tools/bench_float_signals.py --shims 5000,100000,3000001 [--runs 5] [--calls 5] [--json out.json]

times the per-read float shims instead (profiles/float_shims.md): one pA read of each size, wall clock per call of
api.shim_stat_f32 (its three calls), api.shim_jnn_pa with the DNA preset and with the literal set of 1., each run the
mean of `--calls` calls after one warm-up call.  SIGTK_AMD_LIB selects the library, for a comparison of two builds."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see tests/conftest.py)

from sigtk_amd import api, device  # noqa: E402

HBM_PEAK = 8.0e12


def timed(call, runs):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def shims(a, dev):
    dna = api.JnnParam(0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0)
    rows = []
    for n in (int(v) for v in a.shims.split(",")):
        b = device.synth_reads(1, n, seed=11, kind=0, device=dev)
        pa = torch.empty(b.n_samples, dtype=torch.float32, device=dev)
        device.pa(b, pa)
        torch.cuda.synchronize()
        x = pa[int(b.offsets_host[0]):int(b.offsets_host[0]) + n].cpu().numpy()
        med = float(np.median(x))
        literal = api.JnnParam(-1.0, 4, 50, 150, 1.0, 5, med + 8.0, med - 8.0)   # error >= corrector
        res = {"n": n, "library": api.LIB_PATH}
        for name, call in (("shim_stat_f32", lambda: api.shim_stat_f32(x)), ("shim_jnn_pa_dna", lambda: api.shim_jnn_pa(x, dna)),
                           ("shim_jnn_pa_literal", lambda: api.shim_jnn_pa(x, literal))):
            call()
            ms = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                ms.append((time.perf_counter() - t0) / a.calls * 1e3)
            res[name] = {"ms_per_call": ms}
        rows.append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="10000x100000,200000x5000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8, help="reads the shim loop is timed on")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shims", default=None, help="N1,N2,..: time the per-read float shims on one read of each size instead")
    ap.add_argument("--calls", type=int, default=5, help="--shims: calls per run")
    a = ap.parse_args()
    L = api._float_lib()
    dev = torch.device("cuda", 0)
    if a.shims:
        return shims(a, dev)
    stream = lambda: int(torch.cuda.current_stream().cuda_stream)
    dna = api.JnnParam(0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0)
    rows = []
    for shape in a.shapes.split(","):
        nr, ln = (int(v) for v in shape.split("x"))
        b = device.synth_reads(nr, ln, seed=11, kind=0, device=dev)
        pa = torch.empty(b.n_samples, dtype=torch.float32, device=dev)
        device.pa(b, pa)
        torch.cuda.synchronize()
        fb = device.float_reads(pa, b.offsets_host.astype(np.int64), b.lengths_host.astype(np.int64))
        values = nr * ln
        med = float(pa[int(b.offsets_host[0]):int(b.offsets_host[0]) + ln].median())
        literal = api.JnnParam(-1.0, 4, 50, 150, 1.0, 5, med + 8.0, med - 8.0)   # error >= corrector
        # ---- 1. the float batch
        out = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
        ws = device._float_workspace(fb, "sgk_stat_f32_workspace_bytes")
        arena = device.FloatSegArena(fb)

        def stat_f32():
            api.check(L.sgk_stat_f32(*fb.view(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream()), "sgk_stat_f32")

        res = {"shape": shape, "values": values}
        t = timed(stat_f32, a.runs)
        res["stat_f32"] = {"ms": t, "bytes": 3 * 4 * values}
        t = timed(lambda: device.jnn_f32(fb, arena, dna), a.runs)
        res["jnn_f32_dna"] = {"ms": t, "bytes": (3 * 4 + 2 / 8) * values}   # two sums, the mask sweep; masks written and read
        t = timed(lambda: device.jnn_f32(fb, arena, literal), a.runs)
        res["jnn_f32_literal"] = {"ms": t, "bytes": 4 * values}
        for k in ("stat_f32", "jnn_f32_dna", "jnn_f32_literal"):
            res[k]["hbm_share"] = res[k]["bytes"] / (res[k]["ms"][0] * 1e-3) / HBM_PEAK
        # ---- 2. the shim loop, scaled
        host = [pa[int(o):int(o) + ln].cpu().numpy() for o in b.offsets_host[:a.sample]]
        api.shim_stat_f32(host[0]); api.shim_jnn_pa(host[0], dna)
        t0 = time.perf_counter()
        for x in host:
            api.shim_stat_f32(x)
        t1 = time.perf_counter()
        for x in host:
            api.shim_jnn_pa(x, dna)
        t2 = time.perf_counter()
        res["shim_stat_scaled_ms"] = (t1 - t0) / len(host) * nr * 1e3
        res["shim_jnn_scaled_ms"] = (t2 - t1) / len(host) * nr * 1e3
        res["shim_sample"] = len(host)
        # ---- 3. the int16 yardstick
        res["stat_i16"] = {"ms": timed(lambda: device.stat(b), a.runs)}
        seg = device.SegArena(b)
        res["jnn_i16_dna"] = {"ms": timed(lambda: device.jnn(b, seg, 0, params=dna), a.runs)}
        rows.append(res)
        print(json.dumps(res), flush=True)
        del b, pa, fb, out, ws, arena, seg
        torch.cuda.empty_cache()
    print("| shape | call | median ms (min - max) | HBM bytes | share of 8 TB/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        for k in ("stat_f32", "jnn_f32_dna", "jnn_f32_literal"):
            m = r[k]["ms"]
            print("| %s | %s | %.2f (%.2f - %.2f) | %.2f GB | %.0f %% |" % (r["shape"], k, m[0], m[1], m[2], r[k]["bytes"] / 1e9,
                                                                      100 * r[k]["hbm_share"]))
        print("| %s | shim loop stat, SCALED from %d reads | %.0f | | |" % (r["shape"], r["shim_sample"], r["shim_stat_scaled_ms"]))
        print("| %s | shim loop jnn_pa, SCALED from %d reads | %.0f | | |" % (r["shape"], r["shim_sample"], r["shim_jnn_scaled_ms"]))
        for k in ("stat_i16", "jnn_i16_dna"):
            m = r[k]["ms"]
            print("| %s | %s (int16 yardstick) | %.2f (%.2f - %.2f) | | |" % (r["shape"], k, m[0], m[1], m[2]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
