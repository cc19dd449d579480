#!/usr/bin/env python3
"""development: wall time of `qts -b 1` with --gpu-inflate (records inflated, rewritten and deflated on the GPU) against
--gpu-deflate (records inflated and parsed on the host threads), on the synthetic file of tools/bench_deflate.py --cli
(64 reads of 100 000 samples, their records repeated) and on the same reads written with ONT's six auxiliary columns.
Medians of three runs, the variants taken in turn; the CLI's own stage split (SGK_CLI_TIMING) of the median run.
--parent-cli names a `sigtk-amd` built from the parent commit: its --gpu-deflate is the line to beat.
    python tools/bench_qts_inflate.py [--reads 3968] [--parent-cli PATH] > profiles/<name>.json"""
import argparse, json, os, re, statistics, struct, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sigtk_amd import api, blow5, build

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=3968)
ap.add_argument("--read-len", type=int, default=100000)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--parent-cli", default="")
a = ap.parse_args()
NB = 64
reads, dig, off, rng = api.synth_reads_host(NB, a.read_len, 9, 0)
ONT_AUX = [("start_time", "uint64_t"), ("read_number", "int32_t"), ("start_mux", "uint8_t"), ("median_before", "double"),
           ("end_reason", "enum{unknown,partial,mux_change,unblock_mux_change,data_service_unblock_mux_change,signal_positive,signal_negative}"),
           ("channel_number", "char*")]


def make_file(path, aux):
    """64 distinct reads, their records written over and over (qts does not mind equal ids)"""
    rs = [blow5.Read("synth-%08d" % i, 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0, reads[i],
                     aux=(4000 * i, i, 1 + i % 4, 200.0 + (i % 97) * 0.25, i % 7, str(1 + i % 512)) if aux else None)
          for i in range(NB)]
    blow5.write_blow5(path, rs, {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"}, aux_types=ONT_AUX if aux else None)
    buf = open(path, "rb").read()
    (hsize,) = struct.unpack_from("<I", buf, 64)
    body = buf[68 + hsize:-5]
    with open(path, "wb") as fh:
        fh.write(buf[:68 + hsize])
        for _ in range(a.reads // NB):
            fh.write(body)
        fh.write(b"5WOLB")


def stages(stderr):
    s = stderr.decode(errors="replace")
    m = re.search(r"read ([\d.]+) s, inflate\+parse ([\d.]+) s, stage\+submit ([\d.]+) s \| wait-for-GPU ([\d.]+) s, "
                  r"format ([\d.]+) s, write ([\d.]+) s \| HIP init ([\d.]+) s, job create ([\d.]+) s", s)
    out = dict(zip(("read", "parse", "stage", "wait", "format", "write", "hip_init", "job_create"), map(float, m.groups()))) if m else {}
    m = re.search(r"records decompressed on the GPU: (\d+) of (\d+); batches redone on the host: (\d+)", s)
    if m:
        out["on_gpu"], out["records"], out["redone"] = (int(x) for x in m.groups())
    return out


out = {"reads": a.reads // NB * NB, "samples": a.reads // NB * NB * a.read_len, "threads": a.threads, "runs": a.runs}
with tempfile.TemporaryDirectory() as tmp:
    for name, aux in (("no_aux", False), ("six_columns", True)):
        f = os.path.join(tmp, name + ".blow5")
        make_file(f, aux)
        variants = []
        if a.parent_cli:
            variants.append(("parent_gpu_deflate", a.parent_cli, ["--gpu-deflate"]))
        variants.append(("gpu_deflate", build.CLI, ["--gpu-deflate"]))
        for mb in (16, 64, 128):
            variants.append(("gpu_inflate_%dM" % mb, build.CLI, ["--gpu-inflate", "--batch-samples", str(mb << 20)]))
        walls = {v[0]: [] for v in variants}
        errs = {v[0]: [] for v in variants}
        env = dict(os.environ, SGK_CLI_TIMING="1")
        # one untimed run first: the file into the page cache, the code objects loaded once
        subprocess.run([build.CLI, "qts", "--gpu-deflate", "-b", "1", "-t", str(a.threads), f, "-o", os.path.join(tmp, "warm.blow5")],
                       capture_output=True, env=env, timeout=300, check=True)
        for _ in range(a.runs):
            for tag, cli, extra in variants:
                o = os.path.join(tmp, tag + ".blow5")
                t0 = time.perf_counter()
                p = subprocess.run([cli, "qts", *extra, "-b", "1", "-t", str(a.threads), f, "-o", o], capture_output=True, env=env,
                                   timeout=300)
                walls[tag].append(time.perf_counter() - t0)
                errs[tag].append(p.stderr)
                if p.returncode != 0:
                    raise SystemExit("%s: %s" % (tag, p.stderr[-400:]))
        res = {"input_mb": round(os.path.getsize(f) / 1e6, 1)}
        base = open(os.path.join(tmp, "gpu_deflate.blow5"), "rb").read()
        for tag, _, _ in variants:
            w = walls[tag]
            k = w.index(statistics.median(w)) if len(w) % 2 else 0
            # (HIP initialisation is 0.06 - 0.25 s of a run and varies from run to run more than the paths differ)
            less = [x - stages(e).get("hip_init", 0.0) for x, e in zip(w, errs[tag])]
            res[tag] = {"wall_s_median": round(statistics.median(w), 3), "wall_s": [round(x, 3) for x in w],
                        "wall_less_hip_init_s_median": round(statistics.median(less), 3),
                        "wall_less_hip_init_s": [round(x, 3) for x in less],
                        "stages_s": stages(errs[tag][k]),
                        "output_equals_gpu_deflate": open(os.path.join(tmp, tag + ".blow5"), "rb").read() == base}
        out[name] = res
        print(name, json.dumps(res), file=sys.stderr)
print(json.dumps(out, indent=1))
