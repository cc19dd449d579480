#!/usr/bin/env python3
"""Times sgk_normalise_f32 on batches of float (pA) signals (profiles/normalise.md):

    python tools/bench_normalise.py [--shapes 10000x100000,200000x5000] [--runs 5] [--json out.json]

Per shape, on pA of the benchmark's synthetic DNA reads (made and converted on the device), in one process:
  1. sgk_normalise_f32 with both methods, out of place, with the HBM bytes the algorithm moves -- z-score: the three
     sweeps of sgk_stat_f32 and the write sweep's read, plus one write (5 x 4 B per value); med-MAD: three counting sweeps
     more (8 x 4 B per value) -- and the share of the HBM peak (8 TB/s) that comes to (the count assumes that no read
     has a mean that is not finite: such a read gets one more read-only sweep, which looks for a NaN or an infinity; the
     synthetic pA signal has none);
  2. sgk_stat_f32 on the same batch, the yardstick, and its ratio to each method;
  3. what a caller could do before the entry point existed: sgk_stat_f32, a torch elementwise abs(x - median) into a
     temporary, sgk_stat_f32 on that, a torch elementwise (x - shift) / scale (med-MAD), or sgk_stat_f32 and the last
     step alone (z-score).  torch's elementwise kernels work on a [reads, length] view of the batch, the cheapest form a
     caller has; their quotient is torch's, not the definition's.
HIP events around each call after one warm-up call, the median of `--runs` runs (min - max beside it).

    python tools/bench_normalise.py --stat-only [--shapes ...] [--runs 5] [--json out.json]

times sgk_stat_f32 alone and binds nothing else: SIGTK_AMD_LIB selects the library, so that two builds -- one of them
from before sgk_normalise_f32 existed -- can be run alternately on one box."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see tests/conftest.py)

from sigtk_amd import api, device  # noqa: E402

HBM_PEAK = 8.0e12
SWEEPS = {"zscore": 4 + 1, "medmad": 7 + 1}   # reads + the write, 4 B per value each


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


def stat_binding():
    """sgk_stat_f32 and its size function, bound by hand: all a build from before the normalise calls has"""
    L = api.load_library()
    L.sgk_stat_f32_workspace_bytes.restype = C.c_size_t
    L.sgk_stat_f32_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    L.sgk_stat_f32.restype = C.c_int
    L.sgk_stat_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="10000x100000,200000x5000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--stat-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no GPU: nothing here can be timed without one"
    L = stat_binding()
    dev = torch.device("cuda", 0)
    stream = lambda: int(torch.cuda.current_stream().cuda_stream)
    rows = []
    for shape in a.shapes.split(","):
        nr, ln = (int(v) for v in shape.split("x"))
        b = device.synth_reads(nr, ln, seed=11, kind=0, device=dev)
        pa = torch.empty(b.n_samples, dtype=torch.float32, device=dev)
        device.pa(b, pa)
        torch.cuda.synchronize()
        fb = device.float_reads(pa, b.offsets_host.astype(np.int64), b.lengths_host.astype(np.int64))
        values = nr * ln
        res = {"shape": shape, "values": values, "library": api.LIB_PATH}

        def stat_call(batch, out, ws):
            api.check(L.sgk_stat_f32(*batch.view(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream()), "sgk_stat_f32")

        def stat_buffers(batch):
            n = int(L.sgk_stat_f32_workspace_bytes(batch.n_reads, batch.n_values, batch.max_read_len))
            return (torch.zeros(nr * 16, dtype=torch.uint8, device=dev), torch.zeros(max(n, 64), dtype=torch.uint8, device=dev))

        out_x, ws_x = stat_buffers(fb)
        res["stat_f32"] = {"ms": timed(lambda: stat_call(fb, out_x, ws_x), a.runs), "bytes": 3 * 4 * values}
        if not a.stat_only:
            # ---- 1. the library's call
            y = torch.zeros_like(pa)
            ws = device._float_workspace(fb, "sgk_normalise_f32_workspace_bytes")
            for name, method in api.NORM_METHODS.items():
                t = timed(lambda: fb.normalise_f32(method, y=y, ws=ws), a.runs)
                res[name] = {"ms": t, "bytes": SWEEPS[name] * 4 * values}
                res[name]["bytes_per_s"] = res[name]["bytes"] / (t[0] * 1e-3)
                res[name]["hbm_share"] = res[name]["bytes_per_s"] / HBM_PEAK
                res[name]["stat_f32_ratio"] = t[0] / res["stat_f32"]["ms"][0]
            # ---- 3. the composition a caller had: the reads as rows of one strided view (alloc_reads pads every read alike)
            stride = int(b.offsets_host[1] - b.offsets_host[0]) if nr > 1 else ln
            first = int(b.offsets_host[0])
            xv = pa[first:first + nr * stride].view(nr, stride)[:, :ln]
            yv = y[first:first + nr * stride].view(nr, stride)[:, :ln]
            tmp = torch.empty((nr, ln), dtype=torch.float32, device=dev)
            ft = device.float_reads(tmp.view(-1), np.arange(nr, dtype=np.int64) * ln, np.full(nr, ln, dtype=np.int64))
            out_t, ws_t = stat_buffers(ft)
            rec_x, rec_t = out_x.view(torch.float32).view(nr, 4), out_t.view(torch.float32).view(nr, 4)

            def compose_medmad():
                stat_call(fb, out_x, ws_x)
                med = rec_x[:, 2:3]
                torch.sub(xv, med, out=tmp)
                tmp.abs_()
                stat_call(ft, out_t, ws_t)
                scale = rec_t[:, 2:3] * 1.4826
                torch.sub(xv, med, out=yv)
                yv.div_(scale)

            def compose_zscore():
                stat_call(fb, out_x, ws_x)
                torch.sub(xv, rec_x[:, 0:1], out=yv)
                yv.div_(rec_x[:, 1:2])

            for name, call in (("zscore", compose_zscore), ("medmad", compose_medmad)):
                t = timed(call, a.runs)
                res["compose_" + name] = {"ms": t, "library_ratio": res[name]["ms"][0] / t[0]}
            del y, ws, tmp, ft, out_t, ws_t
        rows.append(res)
        print(json.dumps(res), flush=True)
        del b, pa, fb, out_x, ws_x
        torch.cuda.empty_cache()
    print("| shape | call | median ms (min - max) | HBM bytes | bytes / s | share of 8 TB/s | time / sgk_stat_f32 | library / composition |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        m = r["stat_f32"]["ms"]
        print("| %s | sgk_stat_f32 | %.2f (%.2f - %.2f) | %.2f GB | | | 1 | |" % (r["shape"], m[0], m[1], m[2], r["stat_f32"]["bytes"] / 1e9))
        for k in ("zscore", "medmad"):
            if k not in r:
                continue
            m, c = r[k]["ms"], r["compose_" + k]
            print("| %s | sgk_normalise_f32 %s | %.2f (%.2f - %.2f) | %.2f GB | %.2f TB/s | %.0f %% | %.2f | %.2f |" % (
                r["shape"], k, m[0], m[1], m[2], r[k]["bytes"] / 1e9, r[k]["bytes_per_s"] / 1e12, 100 * r[k]["hbm_share"],
                r[k]["stat_f32_ratio"], c["library_ratio"]))
            print("| %s | composition %s | %.2f (%.2f - %.2f) | | | | | |" % (r["shape"], k, c["ms"][0], c["ms"][1], c["ms"][2]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
