#!/usr/bin/env python3
"""development: k_zstd on N zstd-compressed (level 1) BLOW5 records of 100 000-sample reads with an svb-zd signal, and
k_inflate on the same records compressed with zlib level 6, in one run: median ms per launch (events around each
launch), compressed and decompressed bytes/s, samples/s.

    python tools/bench_zstd.py [--reads 2560] [--records FILE.npz] [--make-records FILE.npz]

The records need a compressor: libzstd through ctypes where the machine has one; otherwise --records takes a file that
--make-records wrote on a machine that has (64 records, replicated to --reads)."""
import argparse, ctypes, json, os, sys, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2560)
ap.add_argument("--read-len", type=int, default=100000)
ap.add_argument("--launches", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--records")
ap.add_argument("--make-records")
a = ap.parse_args()


def zstd_level1(data):
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    cap = z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    size = z.ZSTD_compress(out, cap, data, len(data), 1)   # (before out.raw is read: that is a copy)
    return out.raw[:size]


def signal(rs, n):
    """a nanopore-like signal: levels that hold for a few samples, noise on top (deltas of one byte, mostly)"""
    levels = rs.randint(350, 750, size=n // 8 + 2)
    return (np.repeat(levels, 8)[:n] + rs.randint(-12, 13, size=n)).astype(np.int16)


if a.records:
    z = np.load(a.records)
    offs, lens = z["offsets"], z["raw_lengths"]
    frames = [z["frames"][int(offs[k]):int(offs[k + 1])].tobytes() for k in range(len(lens))]
    plain = None
    a.read_len = int(z["read_len"])   # the samples of a record are those of the file's records, not --read-len
else:
    from sigtk_amd import blow5
    rs = np.random.RandomState(9)
    plain = [b"\x24\x00" + b"x" * 36 + bytes(44) + blow5.svb_zd_encode(signal(rs, a.read_len)) for _ in range(64)]
    frames = [zstd_level1(p) for p in plain]
    lens = np.asarray([len(p) for p in plain], dtype=np.int64)
if a.make_records:
    offs = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    np.savez(a.make_records, frames=np.frombuffer(b"".join(frames), dtype=np.uint8), offsets=offs, raw_lengths=lens,
             read_len=np.int64(a.read_len))
    print("wrote", a.make_records)
    sys.exit(0)

import torch
from sigtk_amd import api, device
from sigtk_amd.device import _ptr, _stream_ptr

L = api.load_library()
dev = torch.device("cuda", 0)
n = a.reads
if plain is None:   # the zlib twins are made from what the zstd kernel decodes
    got, olen, st = device.zstd_decompress(frames, caps=[int(x) for x in lens])
    assert (st == 0).all()
    plain = got
zl = [zlib.compress(p, 6) for p in plain]


def stage(streams):
    sel = [streams[i % len(streams)] for i in range(n)]
    raw = np.asarray([int(lens[i % len(streams)]) for i in range(n)], dtype=np.uint32)
    in_len = np.asarray([len(s) for s in sel], dtype=np.uint32)
    in_off = np.zeros(n, dtype=np.uint64)
    in_off[1:] = np.cumsum((in_len[:-1].astype(np.uint64) + 3) // 4 * 4)
    blob = np.zeros(int(in_off[-1]) + int(in_len[-1]) + 8, dtype=np.uint8)
    for r, s in enumerate(sel):
        blob[int(in_off[r]):int(in_off[r]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out_off = np.zeros(n, dtype=np.uint64)
    out_off[1:] = np.cumsum((raw[:-1].astype(np.uint64) + 15) // 16 * 16)
    t = lambda x, dt: torch.from_numpy(x.view(dt)).to(dev)
    return dict(d_in=torch.from_numpy(blob).to(dev), d_ioff=t(in_off, np.int64), d_ilen=t(in_len, np.int32),
                d_out=torch.zeros(int(out_off[-1]) + int(raw[-1]) + 16, dtype=torch.uint8, device=dev), d_ooff=t(out_off, np.int64),
                d_caps=t(raw, np.int32), d_olen=torch.zeros(n, dtype=torch.int32, device=dev),
                d_st=torch.zeros(n, dtype=torch.int32, device=dev), compressed=int(in_len.sum()), raw=int(raw.sum()))


def measure(fn, name, s):
    def run():
        api.check(fn(_ptr(s["d_in"]), _ptr(s["d_ioff"]), _ptr(s["d_ilen"]), n, _ptr(s["d_out"]), _ptr(s["d_ooff"]), _ptr(s["d_caps"]),
                     _ptr(s["d_olen"]), _ptr(s["d_st"]), _stream_ptr()), name)
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    assert int(s["d_st"].abs().sum().item()) == 0, name
    ms = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "compressed_MB": round(s["compressed"] / 1e6, 1), "decompressed_MB": round(s["raw"] / 1e6, 1),
            "compressed_GB_per_s": round(s["compressed"] / med / 1e6, 2), "decompressed_GB_per_s": round(s["raw"] / med / 1e6, 2),
            "samples_per_s": round(n * a.read_len / med * 1e3)}


res = {"reads": n, "read_len": a.read_len, "launches": a.launches}
sz, si = stage(frames), stage(zl)
# interleaved: zstd, inflate, zstd, inflate (two rounds each, the second reported)
for rnd in range(2):
    res["k_zstd (zstd level 1)"] = measure(L.sgk_zstd_decompress, "sgk_zstd_decompress", sz)
    res["k_inflate (zlib level 6)"] = measure(L.sgk_inflate, "sgk_inflate", si)
print(json.dumps(res))
