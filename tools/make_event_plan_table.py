#!/usr/bin/env python3
"""What the built library answers for the host-side plan of `event` over a grid of batches -> tests/golden/event_plan_table.npz.

    python tools/make_event_plan_table.py [OUT.npz]

No GPU work: sgk_event_plan_opt and the three workspace queries (without a GPU the plan assumes 256 CUs, the MI355X's
count).  The table is recorded ONCE, from the library whose plan is to be kept, and tests/test_event_plan_table.py
recomputes every row from the library it is given with answers() below: run this again only when a planning rule is
meant to change.

The table: `inputs` (n_reads, n_samples, max_read_len, rna, row of `options`), `options` (the six fields of
sgk_event_options_t in front of `reserved`), `params` (window_length1, window_length2, threshold1, threshold2,
peak_height, flags: a generic-route set and a preset-windows set for the presets' kernels) and `outputs`, per input the
columns of COLUMNS."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_READS = (1, 7, 160, 1000, 1023, 1024, 1600, 1800, 3072, 3800, 3900, 9300, 10000, 30000, 200000)
MEANS = (100, 4000, 5000, 16383, 16384, 20000, 32767, 32768, 65536, 100000, 131072, 262143, 300000)
# max_read_len = ceil(mean * r): 5/4 and 81/64 sit on either side of the ragged predicate
RATIOS = ((1, 1), (5, 4), (81, 64), (3, 1), (30, 1))
OPTION_FIELDS = ("segment_len", "long_min", "warmup", "lanes_per_short_read", "short_max", "tail_split")
OPTIONS = ({}, {"tail_split": -1}, {"tail_split": 50}, {"lanes_per_short_read": -1}, {"lanes_per_short_read": 8},
           {"short_max": 4096}, {"segment_len": 4096, "long_min": 10000}, {"warmup": 64})
PARAMS = ((5, 9, 1.4, 9.0, 0.2, 0),    # generic route
          (3, 6, 2.0, 9.5, 0.3, 4))    # the presets' windows with SGK_EVENT_PARAMS_PRESET_KERNELS
PLAN_FIELDS = ("segment_len", "long_min", "max_segments", "max_long_reads", "short_max", "lanes_per_short_read",
               "warmup_override", "tail_split_from", "tail_segment_len")
COLUMNS = PLAN_FIELDS + ("workspace_bytes_opt", "workspace_bytes_param_generic", "workspace_bytes_param_preset_kernels")


def grid():
    rows = []
    for n in N_READS:
        for mean in MEANS:
            for num, den in RATIOS:
                if n == 1:
                    num, den = 1, 1
                for rna in (0, 1):
                    for o in range(len(OPTIONS)):
                        rows.append((n, n * ((mean + 7) // 8 * 8), (mean * num + den - 1) // den, rna, o))
    inputs = np.array(rows, dtype=np.uint64)
    options = np.array([[o.get(f, 0) for f in OPTION_FIELDS] for o in OPTIONS], dtype=np.int64)
    return inputs, options, np.array(PARAMS, dtype=np.float64)


def answers(lib, inputs, options, params):
    """the COLUMNS of every row of `inputs`, asked of `lib` (sigtk_amd.api.load_library())"""
    from sigtk_amd import api
    opts = []
    for row in options:
        o = api.EventOptions()
        for f, v in zip(OPTION_FIELDS, row):
            setattr(o, f, int(v))
        opts.append(o)
    prm = [api.EventParams(int(p[0]), int(p[1]), p[2], p[3], p[4], int(p[5])) for p in params]
    out = np.zeros((len(inputs), len(COLUMNS)), dtype=np.uint64)
    plan = api.EventPlan()
    for i, (n, ns, ml, rna, o) in enumerate(inputs.tolist()):
        opt = C.byref(opts[o])
        assert lib.sgk_event_plan_opt(n, ns, ml, rna, opt, C.byref(plan)) == 0
        out[i, :9] = [getattr(plan, f) for f in PLAN_FIELDS]
        out[i, 9] = lib.sgk_event_workspace_bytes_opt(n, ns, ml, opt)
        out[i, 10] = lib.sgk_event_workspace_bytes_param(n, ns, ml, opt, C.byref(prm[0]))
        out[i, 11] = lib.sgk_event_workspace_bytes_param(n, ns, ml, opt, C.byref(prm[1]))
    return out


if __name__ == "__main__":
    from sigtk_amd import api
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "event_plan_table.npz")
    inputs, options, params = grid()
    outputs = answers(api.load_library(), inputs, options, params)
    np.savez_compressed(out_path, inputs=inputs, options=options, params=params, outputs=outputs)
    c = {k: outputs[:, COLUMNS.index(k)] for k in COLUMNS}
    print("%d rows -> %s (%d bytes): tail split in %d, packing in %d, segment lists in %d, %d distinct long_min, lanes %s"
          % (len(inputs), out_path, os.path.getsize(out_path), int((c["tail_segment_len"] > 0).sum()),
             int((c["lanes_per_short_read"] > 0).sum()), int((c["max_segments"] > 0).sum()),
             len(set(c["long_min"].tolist())), sorted(set(c["lanes_per_short_read"].tolist()))))
