#!/usr/bin/env python3
"""Throughput of the device writer of text SLOW5 signal columns (sgk_slow5_text_*: k_slow5_text_measure,
k_slow5_text_write) on synthetic reads, beside the `pa` text writer (k_text_measure_pa / k_text_write_pa) on the same
batch -- and, with --cli FILE, wall-clock times of `sigtk-amd qts FILE -o out.slow5` beside the reference binary
(oracle/_ref/sigtk_ref, when it is built) on the same file.  profiles/sigtext_encode.md holds what was measured."""
import argparse, hashlib, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def kernels(a):
    import torch
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    L = api.load_library()
    b = device.synth_reads(a.reads, a.read_len, 9, 0, dev)
    heads = [b"synth-%08d\t0\t8192\t3\t1402.882324\t4000\t%d\t" % (r, a.read_len) for r in range(a.reads)]
    tails = [b"\n"] * a.reads
    w = device.Slow5TextWriter(b, heads if a.frames else None, tails if a.frames else None)
    api.check(w.measure(), "sgk_slow5_text_measure")
    torch.cuda.synchronize()
    ro = w.row_offsets.cpu().numpy().astype(np.int64)
    total = int(ro[-1])
    text = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    api.check(w.write(text, total), "sgk_slow5_text_write")
    rc, st = w.status()
    api.check(rc, "sgk_text_status")
    for r in (0, a.reads // 2, a.reads - 1):      # a few rows against the host's join
        o = int(b.offsets_host[r])
        x = b.samples[o:o + a.read_len].cpu().numpy()
        want = (heads[r] if a.frames else b"") + b",".join(b"%d" % int(v) for v in x.tolist()) + (tails[r] if a.frames else b"")
        assert text[int(ro[r]):int(ro[r + 1])].cpu().numpy().tobytes() == want, r
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    for _ in range(a.iters):
        api.check(w.measure(), "sgk_slow5_text_measure")
        api.check(w.write(text, total), "sgk_slow5_text_write")
    torch.cuda.synchronize(); L.sgk_profile_enable(0)
    ms = {k: v[0] / v[1] for k, v in api.profile_read().items()}
    S = a.reads * a.read_len
    out = {"reads": a.reads, "samples": S, "frames": bool(a.frames), "text_bytes_per_sample": round(total / S, 3), "kernels": {}}
    for name, byts in (("k_slow5_text_tiles", 0), ("k_slow5_text_measure", 2 * S), ("k_slow5_text_scan", 0),
                       ("k_slow5_text_write", 2 * S + total)):
        out["kernels"][name] = {"ms": round(ms[name], 4), "samples_per_s": round(S / ms[name] * 1e3, 1),
                                "GBps": round(byts / ms[name] / 1e6, 1), "hbm_frac": round(byts / ms[name] / 1e6 / 8000.0, 4)}
    both = ms["k_slow5_text_measure"] + ms["k_slow5_text_write"] + ms["k_slow5_text_tiles"] + ms["k_slow5_text_scan"]
    out["measure_plus_write_ms"] = round(both, 4)
    out["samples_per_s"] = round(S / both * 1e3, 1)
    del text, w
    if a.pa:
        b.dig[:] = 8192.0; b.off[:] = 3.0; b.rng[:] = 1402.882324
        tw = device.TextWriter(b, [h.split(b"\t")[0] for h in heads], api.TEXT_PA)
        tw.measure(); torch.cuda.synchronize()
        ptotal = int(tw.row_offsets.cpu().numpy().astype(np.int64)[-1])
        ptext = torch.zeros(ptotal + 16, dtype=torch.uint8, device=dev)
        tw.write(ptext, ptotal); torch.cuda.synchronize()
        L.sgk_profile_reset(); L.sgk_profile_enable(1)
        for _ in range(a.iters):
            tw.measure(); tw.write(ptext, ptotal)
        torch.cuda.synchronize(); L.sgk_profile_enable(0)
        pms = {k: v[0] / v[1] for k, v in api.profile_read().items()}
        out["pa_text"] = {"text_bytes_per_sample": round(ptotal / S, 3),
                          "measure_ms": round(pms["k_text_measure_pa"], 4), "write_ms": round(pms["k_text_write_pa"], 4),
                          "write_GBps": round((2 * S + ptotal) / pms["k_text_write_pa"] / 1e6, 1),
                          "samples_per_s": round(S / (pms["k_text_measure_pa"] + pms["k_text_write_pa"]) * 1e3, 1)}
    print(json.dumps(out))


def cli(a):
    from sigtk_amd import build
    ref = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
    progs = {"sigtk-amd": [build.CLI, "qts", "-b", "3", "-t", str(a.threads)]}
    if os.path.exists(ref):
        progs["reference"] = [ref, "qts", "-b", "3"]
    times = {k: [] for k in progs}
    digest = {}
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        for rnd in range(1 + a.runs):          # one warm-up round (page cache, code objects), then alternating runs
            for name, cmd in progs.items():
                outp = os.path.join(d, name + ".slow5")
                t0 = time.perf_counter()
                subprocess.run([*cmd, a.cli, "-o", outp], check=True, capture_output=True)
                dt = time.perf_counter() - t0
                if rnd:
                    times[name].append(round(dt, 3))
                elif not a.no_digest:
                    h = hashlib.sha256()
                    with open(outp, "rb") as fh:
                        for chunk in iter(lambda: fh.read(1 << 24), b""):
                            h.update(chunk)
                    digest[name] = h.hexdigest()
                os.remove(outp)
    print(json.dumps({"file": os.path.basename(a.cli), "bytes": os.path.getsize(a.cli), "wall_s": times,
                      "median_s": {k: sorted(v)[len(v) // 2] for k, v in times.items()},
                      "outputs_identical": len(set(digest.values())) == 1 if len(digest) > 1 else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1, help="0: bare columns; 1: whole lines (a head and a newline per read)")
    ap.add_argument("--pa", type=int, default=1, help="time the pa text writer on the same batch too")
    ap.add_argument("--cli", help="a text SLOW5 file: time `qts` end to end instead of the kernels")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--no-digest", action="store_true")
    a = ap.parse_args()
    cli(a) if a.cli else kernels(a)


if __name__ == "__main__":
    main()
