"""development: time sgk_event on a device-resident synthetic batch with the library SIGTK_AMD_LIB points to
(tools/build_variant.sh); prints the ms of every event kernel and the status counters."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sigtk_amd import api, device

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10000)
ap.add_argument("--read-len", type=int, default=100000)
ap.add_argument("--rna", type=int, default=0)
ap.add_argument("--kind", type=int, default=None)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--ragged", type=float, default=0.0, help="sigma of log-normal read lengths with mean --read-len, as bench.py --ragged")
a = ap.parse_args()
dev = torch.device("cuda", 0)
L = api.load_library()
lens = None
if a.ragged > 0:
    lens = a.read_len * np.exp(np.random.RandomState(5).normal(-0.5 * a.ragged ** 2, a.ragged, size=a.reads))
    lens = np.clip(lens, 200, 16 * a.read_len).astype(np.int64)
b = device.synth_reads(a.reads, a.read_len, seed=1, kind=a.rna if a.kind is None else a.kind, device=dev, lengths=lens)
arena = device.EventArena(b)
device.event(b, arena, a.rna)
torch.cuda.synchronize()
L.sgk_profile_enable(1)
for _ in range(a.steps):
    device.event(b, arena, a.rna)
torch.cuda.synchronize()
prof = api.profile_read()
st = arena.status()
res = {"lib": os.environ.get("SIGTK_AMD_LIB", "default"), "reads": a.reads, "read_len": a.read_len, "ragged": a.ragged, "rna": a.rna,
       "ms": {k: round(v[0] / max(v[1], 1), 4) for k, v in prof.items()},
       "events": int(st.n_events_total), "fallback": int(st.n_fallback_reads), "rerun": int(st.n_rerun_passes),
       "replays": int(st.n_long_replays)}
print(json.dumps(res))
