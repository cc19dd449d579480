#!/usr/bin/env python3
"""Device-resident measure + write of the three row grammars (sgk_text_*: pa, event, event -c) on a batch of
BASELINE config 2's shape (--reads x --read-len synthetic DNA reads; config 2 itself is --reads 10000) and on the
log-normal batch of the same mean (--ragged 0.8, lengths as bench.py draws them).

One JSON line per kind and batch: kernel milliseconds from the library's per-kernel events (sgk_profile_*), the text
bytes, and the HBM bytes computed FROM SHAPES -- what the passes must read and write if every byte moves once:
    pa        2 B/sample read in each pass + the text written
    event     16 B/event read in each pass (+ the ids of the long form, from cache) + the text written
"GBps" is those bytes over the measured time; it is not a counter reading."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--ragged", type=float, default=0.8, help="sigma of the log-normal batch (0: skip it)")
    ap.add_argument("--kinds", default="pa,event,event_c")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import torch
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    L = api.load_library()
    kinds = {"pa": api.TEXT_PA, "event": api.TEXT_EVENT, "event_c": api.TEXT_EVENT_COMPACT}
    batches = [("uniform", None)]
    if a.ragged > 0:
        rs = np.random.RandomState(5)
        lens = a.read_len * np.exp(rs.normal(-0.5 * a.ragged ** 2, a.ragged, size=a.reads))
        batches.append(("log-normal(sigma %.2f)" % a.ragged, np.clip(lens, 200, 16 * a.read_len).astype(np.int64)))
    for bname, lens in batches:
        b = device.synth_reads(a.reads, a.read_len, 11, 0, dev, lengths=lens)
        S = b.total_samples
        ids = [("%08x-dd92-4aad-be1d-59a33545ab1d" % r).encode() for r in range(b.n_reads)]   # 36 bytes, as real ids
        arena = None
        for name in a.kinds.split(","):
            kind = kinds[name]
            if kind != api.TEXT_PA and arena is None:
                arena = device.EventArena(b)
                device.event(b, arena, 0)
                torch.cuda.synchronize()
            w = device.TextWriter(b, ids, kind, arena if kind != api.TEXT_PA else None)
            w.measure()
            torch.cuda.synchronize()
            total = int(w.row_offsets.cpu().numpy().astype(np.uint64)[-1])
            text = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            w.write(text, total)
            rc, st = w.status()
            api.check(rc, "sgk_text_write")
            L.sgk_profile_reset(); L.sgk_profile_enable(1)
            for _ in range(a.iters):
                w.measure()
                w.write(text, total)
            torch.cuda.synchronize(); L.sgk_profile_enable(0)
            pr = {k: v[0] / v[1] for k, v in api.profile_read().items()}
            ms_measure = sum(v for k, v in pr.items() if k.startswith("k_text_measure"))
            ms_write = sum(v for k, v in pr.items() if k.startswith("k_text_write"))
            ms_scan = pr.get("k_text_tiles", 0.0) + pr.get("k_text_scan", 0.0)
            items = S if kind == api.TEXT_PA else int(arena.status().n_events_total)
            item_bytes = 2 if kind == api.TEXT_PA else 16
            hbm_measure, hbm_write = items * item_bytes, items * item_bytes + total
            ms = ms_measure + ms_scan + ms_write
            print(json.dumps({
                "kind": name, "batch": bname, "reads": b.n_reads, "samples": S, "items": items, "tiles": int(st.n_tiles),
                "text_bytes": total, "text_bytes_per_item": round(total / max(items, 1), 2),
                "ms": {"measure": round(ms_measure, 4), "tiles+scan": round(ms_scan, 4), "write": round(ms_write, 4),
                       "total": round(ms, 4)},
                "hbm_bytes_from_shapes": {"measure": hbm_measure, "write": hbm_write},
                "GBps_from_shapes": {"measure": round(hbm_measure / max(ms_measure, 1e-9) / 1e6, 1),
                                     "write": round(hbm_write / max(ms_write, 1e-9) / 1e6, 1)},
                "samples_per_s": round(S / ms * 1e3, 1), "text_GBps": round(total / ms / 1e6, 1)}), flush=True)
            del text, w


if __name__ == "__main__":
    main()
