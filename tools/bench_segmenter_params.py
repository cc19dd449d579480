#!/usr/bin/env python3
"""Times `prefix` with caller-supplied segmenter parameters against the preset route (profiles/segmenter_params.md):

    python tools/bench_segmenter_params.py [--reads 50000] [--len 100000] [--runs 7] [--windows 1000,4096] [--json out.json]

Synthetic RNA reads made on the device; every route is called once to warm up, then `--runs` times.  Per route: the
median, smallest and largest time of the whole call (two events around sgk_prefix_opt / sgk_prefix_param, with the
library's per-kernel profile on, which serialises the launches) and of the adaptor kernel by that profile.  For the
figure of another commit, build that commit's library and select it with SIGTK_AMD_LIB=<path>: a library without
sgk_prefix_param runs the preset route only."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the library: see tests/conftest.py)

from sigtk_amd import api, device  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--len", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--windows", default="1000,4096")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = api.load_library()
    dev = torch.device("cuda", 0)
    b = device.synth_reads(a.reads, a.len, seed=11, kind=1, device=dev)
    torch.cuda.synchronize()
    new = hasattr(L, "sgk_prefix_param")
    cases = [("preset", None)]
    if new:
        g = api.PrefixParams.preset(1, 0)
        g.flags = api.PREFIX_PARAMS_GENERIC
        cases.append(("generic_2000", g))
        for w in [int(x) for x in a.windows.split(",") if x]:
            p = api.PrefixParams.preset(1, 0)
            p.adaptor.window = w
            cases.append(("window_%d" % w, p))
        cases.append(("preset_again", None))
    res = {"lib": api.LIB_PATH, "reads": a.reads, "samples_per_read": a.len, "runs": a.runs}
    for name, p in cases:
        call = (lambda: device.prefix(b, 1, 0, params=p)) if new else (lambda: device.prefix(b, 1, 0))
        call()
        torch.cuda.synchronize()
        whole, kern = [], []
        for _ in range(a.runs):
            L.sgk_profile_enable(1)
            L.sgk_profile_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            whole.append(e0.elapsed_time(e1))
            kern.append({k: v[0] for k, v in api.profile_read().items() if "adaptor" in k or "long_chains" in k})
            L.sgk_profile_enable(0)
        names = sorted({k for d in kern for k in d})
        res[name] = {"whole_ms": [statistics.median(whole), min(whole), max(whole)],
                     "kernel_ms": {k: [statistics.median([d.get(k, 0.0) for d in kern]), min(d.get(k, 0.0) for d in kern),
                                       max(d.get(k, 0.0) for d in kern)] for k in names}}
        print(name, json.dumps(res[name]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
