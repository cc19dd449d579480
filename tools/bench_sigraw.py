#!/usr/bin/env python3
"""k_sigraw_gather against a device-to-device copy of the same bytes, and k_inflate on records with an uncompressed signal
(profiles/zrec_raw.md).

    python tools/bench_sigraw.py [--reads 20000] [--read-len 100000] [--launches 20] [--records 1000] > zrec_raw_kernel.json

Kernel: `reads` records of `read-len` plain int16 samples behind a 48-byte head, every record on a 16-byte boundary and
its signal at byte residue 0, 1, 2 or 15 of 16 (one layout per residue), gathered into an arena laid out as
sgk_job_begin lays it out (reads on 64-sample boundaries).  HIP events around `launches` launches after 3 warm-up ones.
The yardstick is hipMemcpyAsync device to device (through torch's Tensor.copy_) of reads x read-len x 2 bytes between the
same two buffers, in the same process, timed the same way: both read and write every sample once.  Rates are bytes of
samples moved per second (count them twice for the memory traffic).

Inflate: `records` synthetic reads as records with ONT's six auxiliary columns and plain samples, zlib-compressed
(level 6, as slow5lib writes them), staged with Job.stage_zrec(signal_format=SIGNAL_INT16) and run through `stat`;
k_inflate's and k_sigraw_gather's times come from sgk_profile_* (HIP events around each launch)."""
import argparse
import json
import os
import struct
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sigtk_amd import api, blow5, device  # noqa: E402

HEAD = 48


def timed(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e-3


def kernel_bench(a, dev):
    n, ln = a.reads, a.read_len
    stride = (HEAD + 15 + 2 * ln + 15) // 16 * 16
    src = torch.randint(0, 256, (n * stride + 32,), dtype=torch.uint8, device=dev)
    dstride = (ln + 63) // 64 * 64
    arena = torch.zeros(256 + n * dstride + 64, dtype=torch.int16, device=dev)
    i32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.uint32).view(np.int32)).to(dev)
    i64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.uint64).view(np.int64)).to(dev)
    rec_off = i64(np.arange(n, dtype=np.uint64) * stride)
    offs = i64(256 + np.arange(n, dtype=np.uint64) * dstride)
    lens = i32(np.full(n, ln))
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    nbytes = n * ln * 2
    dst_bytes, src_bytes = arena.view(torch.uint8)[:nbytes], src[:nbytes]

    def copy():     # Tensor.copy_ between contiguous views of one dtype on one device is one hipMemcpyAsync, device to device
        dst_bytes.copy_(src_bytes)
    t_copy = timed(copy, a.launches)
    out = {"reads": n, "read_len": ln, "sample_bytes": nbytes, "launches": a.launches,
           "unit_samples": device.sigraw_unit_samples(),
           "memcpy_d2d": {"s": t_copy, "bytes_per_s": nbytes / t_copy}, "residues": {}}
    for res in (0, 1, 2, 15):
        sig_off = i32(np.full(n, HEAD + res))
        rec_len = i32(np.full(n, HEAD + res + 2 * ln))
        run = lambda: device.sigraw_gather(src, rec_off, rec_len, sig_off, arena, offs, lens, ln, status=status)
        t = timed(run, a.launches)
        assert int(status.abs().sum()) == 0
        for r in (0, n // 2, n - 1):     # the bytes are the source's
            o = r * stride + HEAD + res
            want = src[o:o + 2 * ln].cpu().numpy().view("<i2")
            got = arena[256 + r * dstride:256 + r * dstride + ln].cpu().numpy()
            assert np.array_equal(got, want), (res, r)
        out["residues"][str(res)] = {"s": t, "bytes_per_s": nbytes / t, "of_memcpy": t_copy / t}
    t_copy2 = timed(copy, a.launches)    # the yardstick once more, after the kernel: drift shows here
    out["memcpy_d2d_again"] = {"s": t_copy2, "bytes_per_s": nbytes / t_copy2}
    return out


ONT_AUX = [("start_time", "uint64_t"), ("read_number", "int32_t"), ("start_mux", "uint8_t"), ("median_before", "double"),
           ("end_reason", "enum{unknown,partial,mux_change,unblock_mux_change,data_service_unblock_mux_change,signal_positive,signal_negative}"),
           ("channel_number", "char*")]
TABLE = [(8, 0), (4, 0), (1, 0), (8, 0), (1, 0), (1, 1)]


def inflate_bench(a):
    n = a.records
    reads, dig, off, rng = api.synth_reads_host(n, a.read_len, 77, 0)
    plain, sig_off = [], []
    for i in range(n):
        rid = b"synth-%08d" % i
        raw = np.ascontiguousarray(reads[i], dtype="<i2")
        rec = struct.pack("<H", len(rid)) + rid + struct.pack("<IddddQ", 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0, raw.size)
        sig_off.append(len(rec))
        rec += raw.tobytes() + b"".join(blow5.aux_field_bytes(t, v) for (_, t), v in
                                        zip(ONT_AUX, (4000 * i, i, 1 + i % 4, 200.0 + (i % 97) * 0.25, i % 7, str(1 + i % 512))))
        plain.append(rec)
    recs = [zlib.compress(p) for p in plain]
    lengths = [a.read_len] * n
    room = [o + 2 * a.read_len + 22 + 8 + 256 for o in sig_off]
    job = api.Job(0)
    L = api.load_library()
    job.stage_zrec(recs, lengths, sig_off, [2 * a.read_len] * n, room, dig, off, rng, aux=TABLE, signal_format=api.SIGNAL_INT16)
    job.launch(api.TOOL_STAT)
    got = job.wait()["stat"].tobytes()
    ref = api.Job(0)
    ref.stage(reads, dig, off, rng)
    ref.launch(api.TOOL_STAT)
    assert got == ref.wait()["stat"].tobytes()
    ref.close()
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    for _ in range(a.launches):
        job.launch(api.TOOL_STAT)
        job.wait()
    L.sgk_profile_enable(0)
    prof = api.profile_read()
    job.close()
    zbytes, pbytes = sum(len(r) for r in recs), sum(len(p) for p in plain)
    out = {"records": n, "read_len": a.read_len, "compressed_bytes": zbytes, "inflated_bytes": pbytes, "launches": a.launches}
    for k in ("k_inflate", "k_sigraw_gather", "k_zrec_tail"):
        if k in prof:
            ms, calls = prof[k]
            out[k] = {"ms_per_launch": ms / calls, "calls": calls,
                      "inflated_bytes_per_s": pbytes / (ms / calls * 1e-3) if k != "k_zrec_tail" else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--records", type=int, default=1000)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    api.load_library()
    out = {"device": torch.cuda.get_device_name(0), "kernel": kernel_bench(a, dev)}
    torch.cuda.empty_cache()
    out["inflate"] = inflate_bench(a)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
