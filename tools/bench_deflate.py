#!/usr/bin/env python3
"""development: k_deflate on N rewritten records of 100 000-sample reads (82 bytes of head + the svb-zd blob of the signal
after `qts -b 1 -m round`, about 125 KB): ms per launch, input GB/s, size against zlib level 6; k_inflate on the streams it
wrote against k_inflate on zlib's own; k_qts_assemble through a record-mode job; and with --cli the wall time of
`qts -b 1` over one synthetic file, host path against --gpu-deflate.
    python tools/bench_deflate.py [--reads 20000] [--cli 4000] > profiles/<name>.json"""
import argparse, json, os, statistics, struct, subprocess, sys, tempfile, time, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sigtk_amd import api, blow5, build, device
from sigtk_amd.device import _ptr, _stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, nargs="+", default=[20000, 1280])
ap.add_argument("--read-len", type=int, default=100000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--cli", type=int, default=0, help="reads of the synthetic file for the CLI wall times (0: skip)")
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
L = api.load_library()
dev = torch.device("cuda", 0)
NB = 64
reads, dig, off, rng = api.synth_reads_host(NB, a.read_len, 9, 0)


def quantise(raw):   # -b 1 -m round
    x = raw.astype(np.int64)
    return np.where((x & 1) < 1, x & ~1, (x & ~1) + 2).astype(np.int16)


def record(i, raw):
    blob = blow5.svb_zd_encode(raw)
    rid = b"synth-%08d" % i
    return struct.pack("<H", len(rid)) + rid + struct.pack("<IddddQ", 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0,
                                                           len(blob)) + blob + bytes(24)


recs = [record(i, quantise(reads[i])) for i in range(NB)]
z6 = [zlib.compress(r) for r in recs]
ours, _, st = device.deflate(recs)
assert not st.any() and all(zlib.decompress(z) == r for z, r in zip(ours, recs))
out = {"record_bytes": round(sum(map(len, recs)) / NB), "zlib6_ratio": round(sum(map(len, z6)) / sum(map(len, recs)), 4),
       "gpu_ratio": round(sum(map(len, ours)) / sum(map(len, recs)), 4),
       "gpu_over_zlib6": round(sum(map(len, ours)) / sum(map(len, z6)), 4)}


def tiled(items, n, align):
    """n items (cycling through `items`) in a device buffer built from one tile -> (buffer, offsets, lengths)"""
    ln = np.asarray([len(s) for s in items], dtype=np.uint32)
    o = np.zeros(len(items), dtype=np.uint64)
    o[1:] = np.cumsum((ln[:-1].astype(np.uint64) + align - 1) // align * align)
    tile_bytes = int((int(o[-1]) + int(ln[-1]) + 63) // 64 * 64)
    tile = np.zeros(tile_bytes, dtype=np.uint8)
    for r, s in enumerate(items):
        tile[int(o[r]):int(o[r]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    reps = (n + len(items) - 1) // len(items)
    buf = torch.from_numpy(tile).to(dev).repeat(reps)
    idx = np.arange(n)
    offs = (idx // len(items)).astype(np.uint64) * np.uint64(tile_bytes) + o[idx % len(items)]
    return buf, offs, ln[idx % len(items)]


t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)


def kernel_ms(name, fn, steps):
    fn(); torch.cuda.synchronize()
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    ms = api.profile_read()[name]
    L.sgk_profile_enable(0)
    return ms[0] / ms[1]


def inflate_ms(streams, raw_len, n):
    d_in, in_off, in_len = tiled(streams, n, 4)
    caps = np.asarray([raw_len[i % NB] for i in range(n)], dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64); out_off[1:] = np.cumsum((caps[:-1].astype(np.uint64) + 15) // 16 * 16)
    d_out = torch.zeros(int(out_off[-1]) + int(caps[-1]) + 16, dtype=torch.uint8, device=dev)
    d = [t(in_off, np.int64), t(in_len, np.int32), t(out_off, np.int64), t(caps, np.int32),
         torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
    ms = kernel_ms("k_inflate", lambda: api.check(L.sgk_inflate(_ptr(d_in), _ptr(d[0]), _ptr(d[1]), n, _ptr(d_out), _ptr(d[2]), _ptr(d[3]),
                                                                 _ptr(d[4]), _ptr(d[5]), _stream_ptr()), "sgk_inflate"), a.steps)
    assert int(d[5].abs().sum().item()) == 0
    return ms, float(caps.sum())


for n in a.reads:
    d_in, in_off, in_len = tiled(recs, n, 16)
    caps = np.asarray([device.deflate_bound(int(x)) for x in in_len], dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64); out_off[1:] = np.cumsum((caps[:-1].astype(np.uint64) + 15) // 16 * 16)
    d_out = torch.zeros(int(out_off[-1]) + int(caps[-1]) + 16, dtype=torch.uint8, device=dev)
    d = [t(in_off, np.int64), t(in_len, np.int32), t(out_off, np.int64), t(caps, np.int32),
         torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
    ms = kernel_ms("k_deflate", lambda: api.check(L.sgk_deflate(_ptr(d_in), _ptr(d[0]), _ptr(d[1]), n, _ptr(d_out), _ptr(d[2]), _ptr(d[3]),
                                                                 _ptr(d[4]), _ptr(d[5]), _stream_ptr()), "sgk_deflate"), a.steps)
    assert int(d[5].abs().sum().item()) == 0
    tot = float(in_len.astype(np.float64).sum())
    rec = {"input_mb": round(tot / 1e6, 1), "k_deflate_ms": round(ms, 3), "input_GB_per_s": round(tot / ms / 1e6, 2),
           "samples_per_s": round(n * a.read_len / ms * 1e3)}
    del d_in, d_out
    raw_len = [len(r) for r in recs]
    ms_o, tot_o = inflate_ms(ours, raw_len, n)
    ms_z, _ = inflate_ms(z6, raw_len, n)
    rec["k_inflate_on_gpu_streams_GB_per_s"] = round(tot_o / ms_o / 1e6, 2)
    rec["k_inflate_on_zlib6_streams_GB_per_s"] = round(tot_o / ms_z / 1e6, 2)
    out["reads_%d" % n] = rec
    print(n, rec, file=sys.stderr)

# k_qts_assemble: a record-mode job over 1 280 reads
n = 1280
job = api.Job(0)
sig = [reads[i % NB] for i in range(n)]
job.stage(sig, [dig[i % NB] for i in range(n)], [off[i % NB] for i in range(n)], [rng[i % NB] for i in range(n)])
job.set_record_frames([recs[i % NB][:46] + bytes(24) for i in range(n)], [46] * n)
job.launch_qts(1, 1, True, records=True); res = job.wait()
assert zlib.decompress(res["records"][5])[:46] == recs[5][:46]
L.sgk_profile_reset(); L.sgk_profile_enable(1)
for _ in range(a.steps):
    job.launch_qts(1, 1, True, records=True); job.wait()
prof = api.profile_read()
L.sgk_profile_enable(0)
job.close()
out["job_1280_reads_ms"] = {k: round(prof[k][0] / prof[k][1], 3) for k in
                            ("k_qts", "k_svbzd_size", "k_svbzd_encode", "k_qts_assemble", "k_deflate", "k_bytes_gather") if k in prof}

if a.cli:
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "in.blow5")
        # (64 distinct reads, their records written over and over: qts does not mind equal ids, and the file is there in
        # a second instead of the minutes write_blow5 takes for 4e8 samples)
        blow5.write_blow5(f, [blow5.Read("synth-%08d" % i, 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0, reads[i])
                              for i in range(NB)], {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"})
        buf = open(f, "rb").read()
        (hsize,) = struct.unpack_from("<I", buf, 64)
        body = buf[68 + hsize:-5]
        with open(f, "wb") as fh:
            fh.write(buf[:68 + hsize])
            for _ in range(a.cli // NB):
                fh.write(body)
            fh.write(b"5WOLB")
        cli = {"reads": a.cli // NB * NB, "samples": a.cli // NB * NB * a.read_len, "threads": a.threads,
               "input_mb": round(os.path.getsize(f) / 1e6, 1)}
        for tag, extra in (("host", []), ("gpu_deflate", ["--gpu-deflate"])):
            walls = []
            o = os.path.join(tmp, tag + ".blow5")
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([build.CLI, "qts", *extra, "-b", "1", "-t", str(a.threads), f, "-o", o], capture_output=True)
                walls.append(time.perf_counter() - t0)
                if p.returncode != 0:
                    raise SystemExit(p.stderr[-400:])
            cli[tag] = {"wall_s_median": round(statistics.median(walls), 3), "wall_s": [round(w, 3) for w in walls],
                        "output_mb": round(os.path.getsize(o) / 1e6, 1)}
        cli["output_size_gpu_over_host"] = round(cli["gpu_deflate"]["output_mb"] / cli["host"]["output_mb"], 4)
        a_, b_ = (subprocess.run([build.CLI, "stat", os.path.join(tmp, k + ".blow5")], capture_output=True).stdout
                  for k in ("host", "gpu_deflate"))
        cli["stat_of_both_outputs_identical"] = bool(a_ == b_ and len(a_) > 0)
        out["cli_qts_b1"] = cli
print(json.dumps(out, indent=1))
