#!/usr/bin/env python3
"""ss paf2tsv on the device and end to end (profiles/ss.md).

  kernels   one resident batch of --records x --kmers rows (tools/make_paf.py's records): milliseconds of k_ss_decode and of
            tiles + measure + scan + write, from the library's per-kernel events (sgk_profile_*), means over --iters runs
            after one warm-up; string bytes / s, rows / s and text GB / s with bytes FROM SHAPES
  one       a single record of --one-kmers k-mers (10^6: a 3 MB string): the serial case of one wavefront per record
  --e2e     a PAF of --records records to a temporary file; wall seconds, stdout to /dev/null, medians of three alternating
            runs of `sigtk-amd ss paf2tsv`, the same with --host-decode, and oracle/_ref/sigtk_ref when it has been built

One JSON line per measurement."""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import make_paf

CLI = os.path.join(ROOT, "sigtk_amd", "sigtk-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")


class Rec:
    def __init__(self, rid, ss, start_raw, end_raw, start_kmer, end_kmer, tlen):
        self.rid, self.ss, self.start_raw, self.end_raw, self.tlen = rid, ss, start_raw, end_raw, tlen
        self.rna = int(start_kmer > end_kmer)
        self.st_k, self.end_k = min(start_kmer, end_kmer), max(start_kmer, end_kmer)


def kernels(what, n_records, n_kmers, iters):
    import torch
    from sigtk_amd import api, device
    L = api.load_library()
    recs = [Rec(*r) for r in make_paf.records(n_records, n_kmers)]
    ss_bytes = sum(len(r.ss) for r in recs)
    t = device.SsText(recs)
    t.measure()
    torch.cuda.synchronize()
    st = t.status.cpu().numpy()
    assert not st[:t.n_spans].any(), "the generated strings must decode"
    total = int(t.row_offsets.cpu().numpy().astype(np.uint64)[-1])
    text = torch.empty(total + 64, dtype=torch.uint8, device=t.device)
    t.write(text, total)
    rc, _ = t.status_text()
    api.check(rc, "sgk_ss_text_write")
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    for _ in range(iters):
        t.decode()
        t.measure()
        t.write(text, total)
    torch.cuda.synchronize(); L.sgk_profile_enable(0)
    pr = {k: v[0] / v[1] for k, v in api.profile_read().items()}
    ms = {"decode": pr.get("k_ss_decode", 0.0), "tiles+scan": pr.get("k_ss_tiles", 0.0) + pr.get("k_ss_scan", 0.0),
          "measure": pr.get("k_ss_measure", 0.0), "write": pr.get("k_ss_write", 0.0)}
    rows = t.n_rows
    t_text = ms["tiles+scan"] + ms["measure"] + ms["write"]
    print(json.dumps({"what": what, "records": n_records, "kmers_per_record": n_kmers, "rows": rows, "ss_bytes": ss_bytes,
                      "text_bytes": total, "iters": iters, "ms": {k: round(v, 4) for k, v in ms.items()},
                      "decode_string_MB_per_s": round(ss_bytes / max(ms["decode"], 1e-9) / 1e3, 1),
                      "text_rows_per_s": round(rows / max(t_text, 1e-9) * 1e3, 1),
                      "write_GBps_from_shapes": round((8 * rows + total) / max(ms["write"], 1e-9) / 1e6, 1),
                      "text_GBps_all_three": round(total / max(t_text, 1e-9) / 1e6, 1)}), flush=True)


def wall(cmd):
    t0 = time.time()
    with open(os.devnull, "wb") as null:
        rc = subprocess.run(cmd, stdout=null, stderr=null).returncode
    return time.time() - t0, rc


def e2e(n_records, n_kmers):
    with tempfile.TemporaryDirectory() as d:
        paf = os.path.join(d, "bench.paf")
        ss_bytes, rows = make_paf.write(paf, n_records, n_kmers)
        cmds = {"sigtk-amd (GPU)": [CLI, "ss", "paf2tsv", paf], "sigtk-amd --host-decode": [CLI, "ss", "paf2tsv", "--host-decode", paf]}
        if os.path.exists(REF):
            cmds["reference"] = [REF, "ss", "paf2tsv", paf]
        times = {k: [] for k in cmds}
        for rep in range(4):          # the first round warms the page cache and is dropped
            for k, c in cmds.items():
                t, rc = wall(c)
                assert rc == 0, (k, rc)
                if rep:
                    times[k].append(round(t, 3))
        print(json.dumps({"what": "e2e", "records": n_records, "rows": rows, "paf_bytes": os.path.getsize(paf),
                          "wall_s": times, "median_s": {k: statistics.median(v) for k, v in times.items()},
                          "Mrows_per_s": {k: round(rows / statistics.median(v) / 1e6, 2) for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--kmers", type=int, default=10000)
    ap.add_argument("--one-kmers", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    if not a.no_kernels:
        kernels("kernels", a.records, a.kmers, a.iters)
        kernels("one record", 1, a.one_kmers, a.iters)
    if a.e2e:
        e2e(a.records, a.kmers)


if __name__ == "__main__":
    main()
