#!/usr/bin/env python3
"""`sigtk-amd` with and without --gpu-text on the same file, alternating, in one session: the A/B behind
profiles/cli_gpu_text.json.  The run without the option is exactly the parent behaviour (the host formatters).

    python tools/cli_gpu_text_ab.py [--base-reads 1000] [--threads 16] [--runs 2] [--dir /tmp] \\
        [--cases "event -c:100;event:20;pa:10"]          # subtool : copies of the base file

Per subtool the large file is `copies` concatenations of a base file's records (tools/cli_steady.py: replicate), sized
so that the output stays within what the sink takes: the sink is /dev/null for the timed runs, and both variants'
stdout goes through md5 once more ("identical")."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sigtk_amd import api, blow5, build  # noqa: E402
from cli_steady import replicate, stages  # noqa: E402


def md5_of(cmd):
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    h, n = hashlib.md5(), 0
    while True:
        chunk = p.stdout.read(1 << 24)
        if not chunk:
            break
        h.update(chunk)
        n += len(chunk)
    if p.wait() != 0:
        raise SystemExit("%s failed" % cmd)
    return h.hexdigest(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-reads", type=int, default=1000)
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--cases", default="event -c:100;event:20;pa:10")
    a = ap.parse_args()
    base = os.path.join(a.dir, "ab_base_%d.blow5" % a.base_reads)
    if not os.path.exists(base):
        reads, dig, off, rng = api.synth_reads_host(a.base_reads, a.read_len, 77, 0)
        recs = [blow5.Read("synth-%08d" % i, 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0, reads[i])
                for i in range(a.base_reads)]
        blow5.write_blow5(base, recs, {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"})
    env = dict(os.environ, SGK_CLI_TIMING="1")
    out = {"base_reads": a.base_reads, "read_len": a.read_len, "threads": a.threads, "sink": "/dev/null", "cases": {}}
    for case in a.cases.split(";"):
        tool, copies = case.rsplit(":", 1)
        tool, copies = tool.split(), int(copies)
        big = os.path.join(a.dir, "ab_big_%d_x%d.blow5" % (a.base_reads, copies))
        if not os.path.exists(big):
            replicate(base, big, copies)
        samples = a.base_reads * copies * a.read_len
        rec = {"samples": samples, "file_bytes": os.path.getsize(big), "host": [], "gpu_text": []}
        for _ in range(a.runs):                       # alternating: host, gpu-text, host, gpu-text
            for key, extra in (("host", []), ("gpu_text", ["--gpu-text"])):
                t0 = time.perf_counter()
                with open(os.devnull, "wb") as nul:
                    p = subprocess.run([build.CLI, *tool, "-t", str(a.threads), *extra, big], stdout=nul,
                                       stderr=subprocess.PIPE, env=env)
                w = time.perf_counter() - t0
                if p.returncode != 0:
                    raise SystemExit("%s %s failed: %s" % (tool, extra, p.stderr[-400:]))
                st = stages(p.stderr)
                rec[key].append({"wall_s": round(w, 3), "samples_per_s": round(samples / w),
                                 "stages_s": {k: st.get(k) for k in ("wait-for-GPU", "format", "write", "stage+submit")},
                                 "text_bytes_over_pcie": st.get("text_bytes_over_pcie")})
        ha, na = md5_of([build.CLI, *tool, "-t", str(a.threads), big])
        hb, nb = md5_of([build.CLI, *tool, "-t", str(a.threads), "--gpu-text", big])
        rec["stdout_bytes"] = na
        rec["identical"] = ha == hb and na == nb
        best = {k: min(r["wall_s"] for r in rec[k]) for k in ("host", "gpu_text")}
        rec["best_wall_s"] = best
        rec["gpu_text_speedup"] = round(best["host"] / best["gpu_text"], 3)
        out["cases"][" ".join(tool)] = rec
        print(" ".join(tool), json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
