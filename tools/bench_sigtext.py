#!/usr/bin/env python3
"""Throughput of the device parser of text SLOW5 signal columns (k_sigtext_decode) on synthetic reads
(bytes in: the text, bytes out: 2 B/sample).  The distinct reads are turned into text once on the host and the block
of their columns is replicated on the device to enlarge the batch."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200, help="distinct reads")
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--replicate", type=int, default=100, help="replicate the block of text columns to enlarge the batch")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import torch
    from sigtk_amd import api, blow5, device
    dev = torch.device("cuda", 0)
    L = api.load_library()
    reads, _, _, _ = api.synth_reads_host(a.reads, a.read_len, 9, 0)
    texts = [blow5.slow5_signal_text(r) for r in reads]
    # correctness of the API path on the distinct reads first
    out1, st1 = device.sigtext_decode(texts, [a.read_len] * a.reads, dev)
    torch.cuda.synchronize()
    assert int((st1[:a.reads] != 0).sum().item()) == 0
    o = int(out1.offsets_host[5]); assert np.array_equal(out1.samples[o:o + a.read_len].cpu().numpy(), reads[5])
    del out1
    # one block of 16-byte aligned columns, replicated on the device; 16 bytes of padding at both ends
    tlens = np.array([len(t) for t in texts], dtype=np.int64)
    toffs = np.zeros(a.reads, dtype=np.int64)
    toffs[1:] = np.cumsum((tlens[:-1] + 15) // 16 * 16)
    block = int(toffs[-1] + (tlens[-1] + 15) // 16 * 16)
    host = np.zeros(block, dtype=np.uint8)
    for i, t in enumerate(texts):
        host[int(toffs[i]):int(toffs[i]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    n = a.reads * a.replicate
    pad = torch.zeros(16, dtype=torch.uint8, device=dev)
    d_text = torch.cat([pad, torch.from_numpy(host).to(dev).repeat(a.replicate), pad])
    all_offs = (16 + toffs[None, :] + block * np.arange(a.replicate, dtype=np.int64)[:, None]).reshape(-1)
    all_lens = np.tile(tlens, a.replicate)
    d_toffs = torch.from_numpy(all_offs).to(dev)
    d_tlens = torch.from_numpy(all_lens.astype(np.int32)).to(dev)
    out = device.alloc_reads(np.full(n, a.read_len, dtype=np.int64), dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def run():
        api.check(L.sgk_sigtext_decode(d_text.data_ptr(), d_toffs.data_ptr(), d_tlens.data_ptr(), n, out.samples.data_ptr(),
                                       out.offsets.data_ptr(), out.lengths.data_ptr(), status.data_ptr(), stream))
    run(); torch.cuda.synchronize()
    assert int((status != 0).sum().item()) == 0
    k = n - 3
    o = int(out.offsets_host[k]); assert np.array_equal(out.samples[o:o + a.read_len].cpu().numpy(), reads[k % a.reads])
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    for _ in range(a.iters): run()
    torch.cuda.synchronize(); L.sgk_profile_enable(0)
    ms = {k_: v[0] / v[1] for k_, v in api.profile_read().items()}["k_sigtext_decode"]
    S = n * a.read_len
    tbytes = int(all_lens.sum())
    byts = tbytes + 2 * S
    print(json.dumps({"kernel": "k_sigtext_decode", "reads": n, "samples": S, "text_bytes_per_sample": round(tbytes / S, 3),
                      "ms": round(ms, 4), "samples_per_s": round(S / ms * 1e3, 1), "GBps": round(byts / ms / 1e6, 1),
                      "hbm_frac": round(byts / ms / 1e6 / 8000.0, 4)}))


if __name__ == "__main__":
    main()
