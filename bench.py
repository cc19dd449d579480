#!/usr/bin/env python3
"""bench.py -- headline benchmark: `sigtk event` throughput (raw samples/s, reads/s) on MI355X.

Default workload (BASELINE.json configs[1], `--config 2`): 10 000 synthetic DNA reads x 100 000 samples per GPU
(S = 1e9 int16 samples, 2.0 GB), DNA detector parameters, seed 1; inputs and outputs are resident in HBM when the
timed region starts.  One "step" = one pass of the path over the whole batch.  With --gpus N every rank processes
its own batch of the same size (reads shard embarrassingly; no data-path collective) -> weak scaling.

Other BASELINE configurations (secondary lines, same JSON contract):
  --config 3   `event` with RNA parameters + `prefix` on 50 000 RNA-like reads x 100 000 samples
  --config 4   fused `stat` + `pa` on 125 000 DNA reads x 100 000 samples per GPU (the per-GPU shard of 1 M reads)
  --config 5   the pa / event / stat pipeline over a resident pool of 125 000 DNA reads per GPU: one fused stat+pa pass
               (the per-read statistics and the pA array), then event on the raw samples (it scales on the fly)
  --ragged S   (config 2) log-normal read lengths, sigma S, same mean: the mixed-length line

Prints ONE JSON line on rank 0 (see the driver contract): value = total samples/s over all ranks, ms_per_step = the
wall time of one timed step.  A plain run does only that: set up, warm up, time --steps steps, write the outputs
(--dump-outputs) and print the line.

--full adds the secondary figures, each of which costs time of its own:
  `roofline`           algorithmic HBM bytes of one step over the duration of the path's kernels, measured
                       with HIP events recorded around every launch of the timed steps
  `parity_spot_check`  three reads of the benched output against the oracle, bit for bit
  `cpu_baseline`       the real reference (oracle/_ref/libsigtk_ref.so, kind "reference") or the oracle restatement
                       (kind "port") timed single-threaded on a bounded subsample of the same reads on this host
The oracle is used only there (rank 0, N=1).

--dump-outputs DIR writes what the last timed step computed on rank 0 as DIR/<name>.npy (float32 / float64):
per-read arrays (event counts, stat / prefix records) for every read, and the complete events / pA of a fixed,
seeded sample of reads (at most DUMP_SAMPLE_SAMPLES raw samples).  Inputs are seeded: the same arguments give the
same inputs in every run, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
HBM_ACHIEVABLE_GBS = 6300.0  # what a copy kernel reaches (same guide)
# --dump-outputs: raw samples of the sampled reads whose events / pA are written whole (an event covers >= 2 samples,
# so <= 24 MB of events and 8 MB of pA), and the reads the per-read arrays cover (<= 72 bytes each): under 64 MB
DUMP_SAMPLE_SAMPLES = 2000000
DUMP_MAX_READS = 250000

CONFIGS = {
    2: dict(name="sigtk event (DNA params)", reads=10000, kind=0, rna=0, seed=1),
    3: dict(name="sigtk event (RNA params) + prefix", reads=50000, kind=1, rna=1, seed=2),
    4: dict(name="sigtk stat + pa (fused)", reads=125000, kind=0, rna=0, seed=3),
    5: dict(name="sigtk pa -> event -> stat", reads=125000, kind=0, rna=0, seed=4),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS), help="BASELINE.json configuration")
    ap.add_argument("--reads", type=int, default=0, help="reads per GPU (0: the configuration's)")
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--ragged", type=float, default=0.0, help="sigma of log-normal read lengths with mean --read-len")
    ap.add_argument("--rna", type=int, default=-1, help="detector preset (default: the configuration's)")
    ap.add_argument("--cpu-reads", type=int, default=-1, help="reads in the CPU baseline subsample (0 = skip)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs the configuration's reads (default); strong: ONE population of that "
                         "size is split over the ranks in contiguous ranges balanced by cumulative samples")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for the barrier / MAX-reduce "
                    "(nccl = RCCL; 'gloo' lets several ranks share one GPU for testing)")
    ap.add_argument("--inflight", type=int, default=1,
                    help="(config 2; NOT the contract line) batches in flight: step i runs on stream i %% N with output "
                         "arena i %% N, as the CLI's jobs do -- the next batch's first waves fill the slots the last "
                         "waves of this one leave empty.  The default, 1, is what the driver measures.")
    ap.add_argument("--full", action="store_true",
                    help="also measure the secondary figures: per-kernel times and roofline, the parity spot check "
                         "against the oracle and the single-thread CPU baseline (off by default)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    cfg = dict(CONFIGS[args.config])
    if args.reads:
        cfg["reads"] = args.reads
    if args.rna >= 0:
        cfg["rna"] = args.rna
        cfg["kind"] = args.rna
        if args.config == 2:
            cfg["name"] = "sigtk event (%s params)" % ("RNA" if args.rna else "DNA")
    rna = cfg["rna"]

    import torch
    import torch.distributed as dist
    from sigtk_amd import api, device

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d" % args.gpus)
    ndev = torch.cuda.device_count()
    dev_index = local_rank if args.backend == "nccl" else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=args.backend)

    L = api.load_library()  # raises if the HIP extension is missing: no fallback
    R = cfg["reads"]
    first_read = rank * R  # weak scaling: every rank generates a different slice of the read population
    lens = None
    if args.ragged > 0:
        rs = np.random.RandomState(5 + (rank if args.scaling == "weak" else 0))
        lens = args.read_len * np.exp(rs.normal(-0.5 * args.ragged ** 2, args.ragged, size=R))
        lens = np.clip(lens, 200, 16 * args.read_len).astype(np.int64)
    if args.scaling == "strong" and world > 1:
        # one population of R reads: rank g takes the g-th contiguous range of near-equal cumulative samples
        from sigtk_amd import shard
        all_lens = lens if lens is not None else np.full(R, args.read_len, dtype=np.int64)
        lo, hi = shard.partition_by_samples(all_lens, world)[rank]
        first_read, R = lo, hi - lo
        lens = all_lens[lo:hi] if lens is not None else None
    batch = device.synth_reads(R, args.read_len, seed=cfg["seed"], kind=cfg["kind"], device=dev,
                               first_read=first_read, lengths=lens)
    S = batch.total_samples
    arena = device.EventArena(batch) if args.config in (2, 3, 5) else None
    pa_out = torch.empty(batch.n_samples, dtype=torch.float32, device=dev) if args.config in (4, 5) else None
    stat_out = torch.zeros(max(batch.n_reads, 1) * api.STAT_DTYPE.itemsize, dtype=torch.uint8, device=dev) if args.config == 5 else None

    inflight = max(1, args.inflight) if args.config == 2 else 1
    lanes = [(torch.cuda.Stream(device=dev), device.EventArena(batch)) for _ in range(inflight - 1)]
    step_no = [0]

    def step():
        """enqueue one step; -> the outputs a caller of the path receives from it"""
        if args.config == 2 and inflight > 1:
            k = step_no[0] % inflight
            step_no[0] += 1
            if k == 0:
                device.event(batch, arena, rna)
                return {"arena": arena}
            st_k, ar_k = lanes[k - 1]
            with torch.cuda.stream(st_k):
                device.event(batch, ar_k, rna)
            return {"arena": ar_k}
        if args.config == 2:
            device.event(batch, arena, rna)
            return {"arena": arena}
        elif args.config == 3:
            device.event(batch, arena, rna)
            return {"arena": arena, "prefix": device.prefix(batch, rna, 0)}
        elif args.config == 4:
            stat_rec, _ = device.stat_pa(batch, pa_out)
            return {"stat": stat_rec, "pa": pa_out}
        else:
            # one call (sgk_pipeline): the fused stat + pA pass, then event on the raw samples (it scales on the fly)
            device.pipeline(batch, arena, rna, pa_out, stat_out)
            return {"arena": arena, "stat": stat_out, "pa": pa_out}

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warmup (untimed)
    for _ in range(max(args.warmup, 1)):
        step()
    torch.cuda.synchronize()
    st = arena.status() if arena is not None else None
    E = int(st.n_events_total) if st is not None else 0
    parity = None
    # ---- timed region: exactly K steps (--full: with HIP events around every kernel launch, for `roofline`)
    if args.full:
        L.sgk_profile_reset()
        L.sgk_profile_enable(1)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    t1 = time.perf_counter()
    if args.full:
        L.sgk_profile_enable(0)
    elapsed = t1 - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # units all ranks processed in one step (weak: S per rank; strong: the ranks' shares of one population)
    S_all, R_all = float(S), float(R)
    if world > 1:
        t = torch.tensor([S_all, R_all], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        S_all, R_all = float(t[0].item()), float(t[1].item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, batch, last)

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = S_all / (elapsed / args.steps)
        out = {
            "metric": "event_raw_samples_per_sec" if args.config in (2, 3) else "raw_samples_per_sec",
            "value": round(value, 1),
            "unit": "samples/s",
            "reads_per_sec": round(R_all / (elapsed / args.steps), 1),
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32+f64",
            "data": "synthetic",
            "config": {"workload": "%s on %d synthetic reads x %s samples per GPU (BASELINE configs[%d]), "
                                   "device-resident" % (cfg["name"], R,
                                                        ("log-normal(sigma %.2f, mean %d)" % (args.ragged, args.read_len))
                                                        if args.ragged else str(args.read_len), args.config - 1),
                       "reads_per_gpu": R, "samples_per_read": args.read_len, "samples_per_gpu": int(S),
                       "events_per_step_rank0": E,
                       "fallback_reads": int(st.n_fallback_reads) if st is not None else None,
                       "rerun_chunks": int(st.n_rerun_passes) if st is not None else None,
                       "long_detector_replays": int(st.n_long_replays) if st is not None else None,
                       "long_detector_replay_indices": int(st.n_replay_indices) if st is not None else None,
                       "split_reads": int(st.n_split_reads) if st is not None else None,
                       "batches_in_flight": inflight,
                       "parallelism": "reads sharded across ranks, no collective"},
        }
    if args.full:
        prof = api.profile_read()
        L.sgk_profile_reset()

    if rank == 0 and args.full:
        # per-step device time of each kernel (HIP events on the stream it was launched on, summed over its launches
        # in a step); "path:*" entries bracket a whole subtool (first launch -> last kernel done)
        kern = {k: v[0] / args.steps for k, v in prof.items() if not k.startswith("path:")}
        paths = {k: v[0] / args.steps for k, v in prof.items() if k.startswith("path:")}
        path_ms = sum(paths.values()) if paths else sum(kern.values())
        if args.config in (3, 4, 5):
            # prefix / stat / pa launch without a path bracket: the step's device time is the sum of its kernels
            # (config 3 counts the prefix kernels' bytes in `alg`, so their time belongs in the denominator too)
            path_ms = sum(kern.values())
        dominant = max(kern, key=kern.get) if kern else None
        alg = {2: 2 * S + 16 * E + 40 * R,
               3: (2 * S + 16 * E + 40 * R) + (2 * S + 48 * R),
               4: 6 * S + 32 * R,
               5: 2 * S + 16 * E + 72 * R + 4 * S}[args.config]
        achieved = alg / (path_ms * 1e-3) / 1e9 if path_ms > 0 else 0.0
        # HBM traffic and VALU counters cannot be collected inside this process (rocprofv3 --pmc passes of this same
        # command, tools/refresh_profiles.sh): the live line carries `traffic: null`; what was recorded for the
        # committed build is quoted under `recorded_pmc` with its source, for N = 1 and the default shape only
        recorded = None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if world == 1 and args.config == 2 and not rna and R == 10000 and args.read_len == 100000 and not args.ragged \
                and os.path.exists(tpath):
            try:
                pmc = json.load(open(tpath))
                recorded = {"hbm_bytes_per_step": pmc.get("hbm_bytes_per_step"),
                            "valu_wave_instructions_per_step": pmc.get("valu_wave_instructions_per_step"),
                            "valu_busy_fraction": pmc.get("valu_busy_fraction"),
                            "recorded_for": pmc.get("recorded_for"), "source": "profiles/pmc_traffic.json"}
            except (OSError, ValueError):
                recorded = None
        roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "frac_of_achievable": round(achieved / HBM_ACHIEVABLE_GBS, 4),
                    "traffic": None, "algorithmic_bytes": alg,
                    # what the PMC passes of profiles/ show for the dominant kernel of each configuration
                    "limiter": {2: "vector instruction issue (bit-exact f64/f32 expression tree; DESIGN.md 3.1), not "
                                   "HBM: `bound` names the roofline the contract prices against",
                                3: "vector instruction issue (k_event, RNA parameters: 2 waves per SIMD)",
                                4: "HBM (k_stat_wave with pA output: 100 GB in 19.7 ms = 5.1 TB/s, 0.76 VALU busy)",
                                5: "vector instruction issue (k_event) after the HBM-bound stat+pa pass"}[args.config],
                    "kernels_ms": {k: round(v, 4) for k, v in kern.items()},
                    "dominant_kernel": dominant, "path_ms": round(path_ms, 4), "recorded_pmc": recorded}

        cpu = None
        cpu_reads = args.cpu_reads if args.cpu_reads >= 0 else (2000 if args.config in (2, 3) else 300)
        if cpu_reads > 0 and world == 1:
            cpu, parity = cpu_leg(args, cfg, batch, last.get("arena"), cpu_reads, rna)
        out.update({"parity_spot_check": parity, "roofline": roofline, "cpu_baseline": cpu})

    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(out_dir, batch, outs):
    """What one step computed, as float32 / float64 .npy files under `out_dir` (rank 0's batch).
    n_events / stat_* / prefix_*: one entry per read (all reads, or the first DUMP_MAX_READS of a seeded permutation,
    in read order: `per_read_reads`); event_* / pa: the complete output of the reads listed in `sample_reads` (a seeded
    choice of reads, taken by their lengths alone), concatenated in read order."""
    import torch
    from sigtk_amd import api
    os.makedirs(out_dir, exist_ok=True)
    n = batch.n_reads
    lens = batch.lengths_host.astype(np.int64)
    order = np.random.RandomState(20261016).permutation(n)
    per_read = np.sort(order[:DUMP_MAX_READS])
    fits = np.cumsum(lens[order]) <= DUMP_SAMPLE_SAMPLES
    sample = np.sort(order[:int(np.argmin(fits)) if not fits.all() else n])
    arrays = {"per_read_reads": per_read.astype(np.float64), "sample_reads": sample.astype(np.float64)}
    dev = batch.samples.device

    def ranges(starts, counts):
        """device index tensor of the concatenated ranges [starts[i], starts[i] + counts[i])"""
        counts = counts.astype(np.int64)
        idx = np.repeat(starts.astype(np.int64) - np.cumsum(counts) + counts, counts) + np.arange(int(counts.sum()))
        return torch.from_numpy(idx).to(dev)

    def records(rec_bytes, dtype, prefix):
        rec = rec_bytes.cpu().numpy().view(dtype)[:n][per_read]
        for f in dtype.names:
            if f != "reserved":
                arrays[prefix + f] = rec[f] if rec[f].dtype == np.float32 else rec[f].astype(np.float64)

    arena = outs.get("arena")
    if arena is not None:
        n_ev = arena.n_events[:n].cpu().numpy().astype(np.int64)
        arrays["n_events"] = n_ev[per_read].astype(np.float64)
        rec = arena.events[ranges(arena.slots_host[sample], n_ev[sample])].cpu().numpy()
        arrays["event_start"] = rec[:, 0].view(np.uint32).astype(np.float64)
        arrays["event_length"] = rec[:, 1].view(np.uint32).astype(np.float64)
        arrays["event_mean"] = rec[:, 2].view(np.float32).copy()
        arrays["event_stdv"] = rec[:, 3].view(np.float32).copy()
    if "stat" in outs:
        records(outs["stat"], api.STAT_DTYPE, "stat_")
    if "prefix" in outs:
        records(outs["prefix"], api.PREFIX_DTYPE, "prefix_")
    if "pa" in outs:
        arrays["pa"] = outs["pa"][ranges(batch.offsets_host[sample], lens[sample])].cpu().numpy()
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_leg(args, cfg, batch, arena, nb, rna):
    """The only place the oracle is touched: first as the checker of the benched output (three reads, bit for bit),
    then as the timed single-thread baseline on the first `nb` reads of the benched batch."""
    from oracle.oracle import Oracle, RefLib
    nb = min(nb, batch.n_reads)
    lens = batch.lengths_host[:nb].astype(np.int64)
    o_end = int(batch.offsets_host[nb - 1]) + int(lens[nb - 1])
    samples = batch.samples[:o_end].cpu().numpy()
    # the oracle/reference helpers take CSR offsets: reads here are padded, so hand them a compacted copy
    comp = np.concatenate([samples[int(batch.offsets_host[r]):int(batch.offsets_host[r]) + int(lens[r])]
                           for r in range(nb)])
    coffs = np.zeros(nb + 1, dtype=np.uint64)
    np.cumsum(lens, out=coffs[1:])
    dig = batch.dig[:nb].cpu().numpy(); off = batch.off[:nb].cpu().numpy(); rng = batch.rng[:nb].cpu().numpy()
    orc = Oracle()
    parity = None
    if arena is not None:
        ok = True
        for r in (0, nb // 2, nb - 1):
            o = int(batch.offsets_host[r]); n = int(batch.lengths_host[r])
            raw = batch.samples[o:o + n].cpu().numpy()
            exp = orc.event_raw(raw, float(batch.dig[r]), float(batch.off[r]), float(batch.rng[r]), rna)
            got = arena.read_events(r)
            ok &= (got.start.size == exp.start.size and np.array_equal(got.start.astype(np.uint64), exp.start)
                   and np.array_equal(got.mean.view(np.uint32), exp.mean.view(np.uint32))
                   and np.array_equal(got.stdv.view(np.uint32), exp.stdv.view(np.uint32)))
        parity = bool(ok)
        if not ok:
            raise SystemExit("bench: GPU event output differs from the oracle -- the timing above is void")
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except OSError:
        pass
    use_ref = RefLib.available()
    lib = RefLib() if use_ref else orc
    kind_s = "reference" if use_ref else "port"
    tc0 = time.perf_counter()
    note = ""
    if args.config in (2, 3, 5):
        ne = lib.event_batch_count(comp, coffs, dig, off, rng, rna) if use_ref else \
            lib.event_batch_count(comp, coffs, dig, off, rng, rna, faithful=1)
        note = "%d events" % ne
    if args.config in (3, 4, 5):
        for r in range(nb):
            raw = comp[int(coffs[r]):int(coffs[r + 1])]
            if args.config == 3:
                lib.find_adaptor(raw, 0)
            else:
                lib.stat(raw, dig[r], off[r], rng[r])
                lib.pa(raw, dig[r], off[r], rng[r])
    tc = time.perf_counter() - tc0
    cpu = {"value": round(int(lens.sum()) / tc, 1), "unit": "samples/s", "cores": 1, "kind": kind_s,
           "sample": "first %d reads of the benched batch (%d samples%s), %.1f s, 1 thread of %d host cpus"
                     % (nb, int(lens.sum()), (", " + note) if note else "", tc, os.cpu_count())}
    return cpu, parity


if __name__ == "__main__":
    main()
