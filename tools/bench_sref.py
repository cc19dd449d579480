#!/usr/bin/env python3
"""sref on the device and end to end.

  kernels   per size N (bases of one random sequence; '+' and '-' rows, 2 (N - 5) positions): milliseconds of the table
            build, tiles + scan, measure and write (sgk_sref_text_*, table in global memory and in LDS) and of
            sgk_sref_levels, from the library's per-kernel events (sgk_profile_*); bytes FROM SHAPES next to them
  --cli     `sigtk-amd sref` on a generated FASTA of --cli-bases bases to /dev/null, wall seconds
  --ref     the CPU baseline, oracle/_ref/sigtk_ref sref, on 1e6 bases in one sequence and in 1 000 sequences, and the CLI on
            the same two files

One JSON line per measurement.  The model is random (any 4 096 levels cost the same); it is written to a temporary file."""
import argparse, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "sigtk_amd", "sigtk-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")


def write_fasta(path, lens, rs):
    with open(path, "wb") as f:
        for i, n in enumerate(lens):
            s = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
            f.write(b">seq%d\n" % i)
            full = n // 80
            body = np.empty((full, 81), dtype=np.uint8)
            body[:, :80] = s[:full * 80].reshape(full, 80)
            body[:, 80] = 10
            f.write(body.tobytes())
            if n % 80:
                f.write(s[full * 80:].tobytes() + b"\n")


def write_model(path, levels):
    with open(path, "w") as f:
        f.write("#k\t6\nkmer\tlevel_mean\n")
        for r, v in enumerate(levels):
            f.write("%s\t%f\n" % ("".join("ACGT"[(r >> (2 * (5 - m))) & 3] for m in range(6)), v))


def wall(cmd):
    t0 = time.time()
    with open(os.devnull, "wb") as null:
        rc = subprocess.run(cmd, stdout=null, stderr=null).returncode
    return time.time() - t0, rc


def kernels(n, iters, levels):
    import torch
    from sigtk_amd import api, device
    L = api.load_library()
    rs = np.random.RandomState(1)
    seq = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()
    for lds in (False, True):
        w = device.SrefText([seq], [b"chr1"], levels, 6, table_in_lds=lds)
        w.measure()
        torch.cuda.synchronize()
        total = int(w.row_offsets.cpu().numpy().astype(np.uint64)[-1])
        text = torch.empty(total + 64, dtype=torch.uint8, device=w.device)
        w.write(text, total)
        rc, st = w.status()
        api.check(rc, "sgk_sref_text_write")
        L.sgk_profile_reset(); L.sgk_profile_enable(1)
        for _ in range(iters):
            w.measure()
            w.write(text, total)
        torch.cuda.synchronize(); L.sgk_profile_enable(0)
        pr = {k: v[0] / v[1] for k, v in api.profile_read().items()}
        sfx = "_lds" if lds else ""
        ms = {"table": pr.get("k_sref_table", 0.0), "tiles+scan": pr.get("k_sref_tiles", 0.0) + pr.get("k_sref_scan", 0.0),
              "measure": pr.get("k_sref_measure" + sfx, 0.0), "write": pr.get("k_sref_write" + sfx, 0.0)}
        pos = w.n_positions
        print(json.dumps({"what": "text", "table": "lds" if lds else "global", "bases": n, "positions": pos,
                          "tiles": int(st.n_tiles), "text_bytes": total, "ms": {k: round(v, 4) for k, v in ms.items()},
                          "bytes_from_shapes": {"measure": pos, "write": pos + total},
                          "GBps_from_shapes": {"measure": round(pos / max(ms["measure"], 1e-9) / 1e6, 1),
                                               "write": round((pos + total) / max(ms["write"], 1e-9) / 1e6, 1)},
                          "positions_per_s": round(pos / sum(ms.values()) * 1e3, 1)}), flush=True)
        if not lds:
            L.sgk_profile_reset(); L.sgk_profile_enable(1)
            for _ in range(iters):
                device.sref_levels(None, None, 6, batch=w, to_host=False)
            L.sgk_profile_enable(0)
            pr = {k: v[0] / v[1] for k, v in api.profile_read().items()}
            t = pr.get("k_sref_levels", 0.0)
            print(json.dumps({"what": "levels", "bases": n, "positions": pos, "ms": round(t, 4),
                              "bytes_from_shapes": 5 * pos, "GBps_from_shapes": round(5 * pos / max(t, 1e-9) / 1e6, 1)}), flush=True)
        del text, w
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000000,100000000")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-bases", type=int, default=100000000)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    rs = np.random.RandomState(3)
    levels = (60 + 70 * rs.rand(4096)).astype(np.float32)
    if not a.no_kernels:
        for n in [int(x) for x in a.sizes.split(",") if x]:
            kernels(n, a.iters, levels)
    with tempfile.TemporaryDirectory() as d:
        model = os.path.join(d, "k6.model")
        write_model(model, levels)
        if a.cli:
            fa = os.path.join(d, "big.fa")
            write_fasta(fa, [a.cli_bases], rs)
            for rep in range(2):
                t, rc = wall([CLI, "sref", "--kmer-model", model, fa])
                print(json.dumps({"what": "cli", "bases": a.cli_bases, "run": rep, "wall_s": round(t, 3), "rc": rc,
                                  "Mbases_per_s": round(a.cli_bases / t / 1e6, 2)}), flush=True)
        if a.ref:
            for name, lens in (("1e6 bases, 1 sequence", [1000000]), ("1e6 bases, 1000 sequences", [1000] * 1000)):
                fa = os.path.join(d, "ref.fa")
                write_fasta(fa, lens, rs)
                t_cli, rc_cli = wall([CLI, "sref", "--kmer-model", model, fa])
                row = {"what": "cpu baseline", "input": name, "sigtk_amd_wall_s": round(t_cli, 3), "sigtk_amd_rc": rc_cli}
                if os.path.exists(REF):
                    t_ref, rc_ref = wall([REF, "sref", fa])
                    row.update({"reference_wall_s": round(t_ref, 3), "reference_rc": rc_ref})
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
