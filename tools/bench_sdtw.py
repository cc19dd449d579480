#!/usr/bin/env python3
"""Times sgk_sdtw_f32 (profiles/sdtw.md):

    python tools/bench_sdtw.py [--shapes 10000x250,1000x1024,1000x4096] [--targets 2x30000] [--runs 5] [--json out.json]

Per shape (n_queries x query length, Gaussian values, against n_targets x target length), with and without
SGK_SDTW_NO_START, in one process: HIP events around the call after one warm-up call, the median of `--runs` runs
(min - max beside it); cells per second (cells = n_queries x n_targets x m x n); and the yardstick: the vector
instructions per cell of the kernel the shape runs on (VALU_PER_CELL below: counted in the step loop of the compiled ISA,
the one executed case of the row switch included, the steps' own instructions shared among the lane's R cells), the time
those take at full issue -- one wave64 vector instruction per 2 cycles on each of 1 024 SIMDs at 2.4 GHz -- and the
fraction of that the call achieves.  The pipeline's fill (63 steps per pass) and the rows of the last lanes that lie past
the query are in the measured time and not in the cell count.
With --c and tools/sdtw_c built (sigtk_amd/build.py: build_tools), the single-threaded C restatement on 20 x 250 against
the same targets, for context."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see tests/conftest.py)

from sigtk_amd import api, device  # noqa: E402

SIMDS, HZ, CYCLES_PER_VALU = 1024, 2.4e9, 2
# rows per lane -> vector instructions per cell (with start, SGK_SDTW_NO_START); "passes": the multi-pass kernel
VALU_PER_CELL = {1: (20.0, 12.0), 2: (16.25, 9.25), 4: (12.0, 6.5), 8: (10.0, 5.25), 16: (9.0, 4.625), "passes": (9.06, 4.69)}


def kernel_of(m):
    if m > 1024:
        return "passes"
    return next(r for r in (1, 2, 4, 8, 16) if m <= 64 * r)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="10000x250,1000x1024,1000x4096")
    ap.add_argument("--targets", default="2x30000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--c", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no GPU: nothing here can be timed without one"
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(5)
    nt, n = (int(v) for v in a.targets.split("x"))
    tb = device.upload_float_reads([rs.normal(size=n).astype(np.float32) for _ in range(nt)], dev)
    rows = []
    for shape in a.shapes.split(","):
        nq, m = (int(v) for v in shape.split("x"))
        qx = torch.from_numpy(rs.normal(size=nq * m).astype(np.float32)).to(dev)
        qb = device.float_reads(qx, np.arange(nq, dtype=np.int64) * m, np.full(nq, m, dtype=np.int64))
        ws = device.sdtw_workspace(qb, tb)
        cells = float(nq) * nt * m * n
        k = kernel_of(m)
        res = {"shape": shape, "targets": a.targets, "cells": cells, "kernel": "k_sdtw R=%s" % k, "workspace_bytes": int(ws.numel()),
               "library": os.path.relpath(api.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}
        for name, options, per_cell in (("start", 0, VALU_PER_CELL[k][0]), ("no_start", api.SDTW_NO_START, VALU_PER_CELL[k][1])):
            t = timed(lambda: device.sdtw_f32(qb, tb, options, ws=ws), a.runs)
            full_issue_ms = cells * per_cell / 64.0 * CYCLES_PER_VALU / (SIMDS * HZ) * 1e3
            res[name] = {"ms": t, "cells_per_s": cells / (t[0] * 1e-3), "valu_per_cell": per_cell, "full_issue_ms": full_issue_ms,
                         "fraction_of_full_issue": full_issue_ms / t[0]}
        recs = device.sdtw_f32(qb, tb, 0, ws=ws)
        torch.cuda.synchronize()
        r = recs.cpu().numpy().view(api.SDTW_DTYPE)
        res["records"] = {"flags_or": int(np.bitwise_or.reduce(r["flags"])), "score_mean": float(r["score"].mean())}
        rows.append(res)
        print(json.dumps(res), flush=True)
        del qx, qb, ws, recs
        torch.cuda.empty_cache()
    c_line = None
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sdtw_c")
    if a.c and os.path.exists(exe):
        c_line = json.loads(subprocess.check_output([exe, "20", "250", str(nt), str(n)]).decode())
        print(json.dumps(c_line), flush=True)
    print("| queries | targets | kernel | option | median ms (min - max) | cells / s | vector instructions / cell | ms at full issue | fraction |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for name in ("start", "no_start"):
            v = r[name]
            print("| %s | %s | %s | %s | %.2f (%.2f - %.2f) | %.3g | %.2f | %.2f | %.0f %% |" % (
                r["shape"], r["targets"], r["kernel"], "" if name == "start" else "SGK_SDTW_NO_START", v["ms"][0], v["ms"][1],
                v["ms"][2], v["cells_per_s"], v["valu_per_cell"], v["full_issue_ms"], 100 * v["fraction_of_full_issue"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rows": rows, "c": c_line}, f, indent=1)


if __name__ == "__main__":
    main()
