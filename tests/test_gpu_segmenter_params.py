"""GPU: jnn and prefix with caller-supplied segmenter parameters (sgk_jnn_param, sgk_prefix_param, k_adaptor_param, the
parametrised polyA kernels, the jobs).

The yardstick is tests/segmenter_params_model.py (tests/test_segmenter_params_cpu.py pins it to the reference's recorded
answers and to the reference itself); everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import prefix_cases as P
import segmenter_params_model as M
from test_gpu_stat import _check_prefix

pytestmark = pytest.mark.gpu

FILL = 12345   # what lies between and around the reads


def _load(reads, leads=None, scal=None):
    import torch
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    b = device.alloc_reads(np.array([r.size for r in reads], dtype=np.int64), dev, leads=leads)
    host = np.full(b.n_samples, FILL, dtype=np.int16)
    for r, raw in enumerate(reads):
        o = int(b.offsets_host[r])
        host[o:o + raw.size] = raw
    b.samples.copy_(torch.from_numpy(host).to(dev))
    n = len(reads)
    dig, off, rng = scal if scal is not None else (np.full(n, P.DIG), np.full(n, P.OFF), np.full(n, P.RNG))
    b.dig[:n].copy_(torch.from_numpy(np.asarray(dig, dtype=np.float64)).to(dev))
    b.off[:n].copy_(torch.from_numpy(np.asarray(off, dtype=np.float64)).to(dev))
    b.rng[:n].copy_(torch.from_numpy(np.asarray(rng, dtype=np.float64)).to(dev))
    return b


def _prefix(gpu, b, rna, params=None, pore=0):
    import torch
    from sigtk_amd import device
    out = device.prefix(b, rna, pore, params=params)
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=gpu.PREFIX_DTYPE)[:b.n_reads]


def _params(gpu, ap: M.AdaptW = None, q: M.PolyW = None, flags=0):
    p = gpu.PrefixParams.preset(1, 0)
    if ap is not None:
        p.adaptor = gpu.Jnnv2Param(ap.std_scale, ap.seg_dist, ap.window, 0.0, ap.hi, ap.lo)
    if q is not None:
        p.polya = gpu.JnnParam(-1.0, q.corrector, q.seg_dist, q.window, q.stall_len, q.error, 0.0, 0.0)
        p.shift, p.band = q.shift, q.band
    p.flags = flags
    return p


# ---------------------------------------------------------------- 1. the window grid
@pytest.fixture(scope="module")
def gold():
    return M.load_golden()


@pytest.mark.parametrize("w", M.WINDOWS)
def test_window_grid(gpu, gold, w):
    """every grid window: reads of W + 1 .. W + 3000 samples at every 16-byte residue of the arena, parameter sets on the
    edges of the reads' own runs; positions against the model, which the CPU test pins to the reference's answers"""
    reads = M.grid_reads(gold, w)
    raws = [M.gen_read(*r) for r in reads]
    fls = [M.flags(raw, w, gold["std_scale"]) for raw in raws]
    failures, n_real = [], 0
    for k, v in enumerate(M.grid_variants(gold, w)):
        leads = [(r + k) % 8 for r in range(len(raws))]   # (8 samples: every 2-byte position of a 16-byte line)
        b = _load(raws, leads=leads)
        got = _prefix(gpu, b, 0, _params(gpu, v))
        for r, (raw, fl) in enumerate(zip(raws, fls)):
            want, _ = M.jnnv2_model(raw, v, fl)
            n_real += 0 if M.trivial(want) else 1
            g = (int(got[r]["adapt_x"]), int(got[r]["adapt_y"]))
            if g != want or int(got[r]["n"]) != raw.size or (int(got[r]["polya_x"]), int(got[r]["polya_y"])) != (-1, -1):
                failures.append("W %d %s read %s lead %d: gpu %s model %s" % (w, v, reads[r], leads[r], g, want))
    assert not failures, "\n".join(failures[:20])
    assert n_real > 0


def test_window_grid_per_read_call(gpu, gold):
    """sgk_jnnv2_param, one read per call: the first set of every window on its longest read; a read of W samples"""
    for w in M.WINDOWS:
        r = max(M.grid_reads(gold, w), key=lambda x: x.extra)
        raw = M.gen_read(*r)
        v = M.grid_variants(gold, w)[0]
        p = gpu.Jnnv2Param(v.std_scale, v.seg_dist, v.window, 0.0, v.hi, v.lo)
        assert gpu.shim_jnnv2_param(raw, p) == (M.jnnv2_model(raw, v)[0], 0), w
        assert gpu.shim_jnnv2_param(raw[:w], p) == ((-1, -1), 0), w
    # sgk_jnnv2 keeps refusing everything but 2000
    assert gpu.shim_jnnv2(raw, gpu.Jnnv2Param(0.5, 1500, 1999, 0.0, 200000, 2000)) == ((-1, -1), gpu.SGK_ERR_ARG)


# ---------------------------------------------------------------- 2. the generic kernel on the presets
@pytest.mark.parametrize("pore", [0, 2])
def test_generic_kernel_equals_the_preset_kernels(gpu, oracle, pore):
    """SGK_PREFIX_PARAMS_GENERIC with a preset over the whole catalogue of tests/prefix_cases.py: the records of the
    preset kernels, byte for byte, and the oracle's.  The existing goldens (tests/golden/prefix_cases_*.prefix_stat.tsv)
    are what the reference's CLI printed; the command line cannot set SGK_PREFIX_PARAMS_GENERIC, so the generic kernel
    reaches them through the preset kernels' records, which tests/test_gpu_prefix_cases.py holds to those files."""
    cat = P.catalogue()
    reads = [k.raw for k in cat]
    scal = tuple(np.array([getattr(k, f) for k in cat]) for f in ("dig", "off", "rng"))
    b = _load(reads, leads=[r % 8 for r in range(len(reads))], scal=scal)
    gen = gpu.PrefixParams.preset(1, pore)
    gen.flags = gpu.PREFIX_PARAMS_GENERIC
    assert gen.route() == gpu.PREFIX_ROUTE_ADAPTOR_PARAM
    for rna in (0, 1):
        want = _prefix(gpu, b, rna, None, pore)
        got = _prefix(gpu, b, rna, gen)
        same = _prefix(gpu, b, rna, gpu.PrefixParams.preset(1, pore))    # the preset route of sgk_prefix_param
        assert got.tobytes() == want.tobytes(), [k.name for k, g, w in zip(cat, got, want) if g.tobytes() != w.tobytes()]
        assert same.tobytes() == want.tobytes()
        with np.errstate(all="ignore"):
            _check_prefix(oracle, reads, scal[0], scal[1], scal[2], rna, pore, got)


# ---------------------------------------------------------------- 3. the division
@pytest.mark.parametrize("w", M.WINDOWS)
def test_quotient_of_every_total(gpu, w):
    """the kernel's own t = tot / W for every tot in [0, 1200 W] against IEEE float32 division: no mismatch"""
    import torch
    n = 1200 * w + 1
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    gpu.check(gpu._param_lib().sgk_debug_roll_means(w, n, out.data_ptr(), None), "sgk_debug_roll_means")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = np.arange(n, dtype=np.float32) / np.float32(w)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print("W %d: %d totals, %d mismatches" % (w, n, bad.size))
    assert bad.size == 0, (w, bad[:5], got[bad[:5]], want[bad[:5]])


# ---------------------------------------------------------------- 4. polyA
def _rna_reads():
    return M.polya_reads()


def test_polya_sets_on_both_routes(gpu, oracle):
    """parameter sets for the wave route and for the lane route in one batch of reads each: against the model on the same
    reads, and the two routes against each other where the wave route applies"""
    cat = _rna_reads()
    reads = [k.raw for k in cat]
    scal = tuple(np.array([getattr(k, f) for k in cat]) for f in ("dig", "off", "rng"))
    b = _load(reads, leads=[(3 * r) % 8 for r in range(len(reads))], scal=scal)
    ap = M.POLYA_ADAPTOR
    routes, n_found, failures = set(), 0, []
    sets = M.polya_sets(cat)
    assert len(sets) >= 13     # (the on-sample bands were found)
    adaptors = [M.jnnv2_model(k.raw, ap)[0] for k in cat]
    for q in sets:
        p = _params(gpu, None, q)
        route = p.route()
        routes.add(route)
        wave_ok = q.stall_len == 1.0 and q.error < q.corrector
        assert route == (gpu.PREFIX_ROUTE_POLYA_WAVE_PARAM if wave_ok else gpu.PREFIX_ROUTE_POLYA_LANE_PARAM), q
        got = _prefix(gpu, b, 1, p)
        gpu.stat_configure(1, 0)      # one read per lane: the parametrised k_polya (and k_adaptor)
        try:
            lane = _prefix(gpu, b, 1, p)
        finally:
            gpu.stat_configure(0, 0)
        for r, k in enumerate(cat):
            with np.errstate(all="ignore"):
                wa, wp = M.prefix_model(oracle, k.raw, k.dig, k.off, k.rng, 1, ap, q, adaptors[r])
            n_found += 1 if wp[1] > 0 else 0
            for name, g in (("routed", got[r]), ("lanes", lane[r])):
                ga, gp = (int(g["adapt_x"]), int(g["adapt_y"])), (int(g["polya_x"]), int(g["polya_y"]))
                if ga != wa or gp != wp:
                    failures.append("%s %s %s: gpu %s %s model %s %s" % (name, q, k.name, ga, gp, wa, wp))
        assert got.tobytes() == lane.tobytes(), q
    assert not failures, "\n".join(failures[:20])
    assert routes == {gpu.PREFIX_ROUTE_POLYA_WAVE_PARAM, gpu.PREFIX_ROUTE_POLYA_LANE_PARAM}
    assert n_found >= len(sets)     # the sets find polyA tails


def test_find_polya_param_per_read(gpu, oracle):
    for k in P.pa_cases():
        for q in (M.POLYA_PRESET, M.POLYA_PRESET._replace(stall_len=0.5, error=50, window=100)):
            p = gpu.JnnParam(-1.0, q.corrector, q.seg_dist, q.window, q.stall_len, q.error, 0.0, 0.0)
            assert gpu.shim_find_polya_param(k.pa, k.top, k.bot, p) == M.polya_first(oracle, k.pa, k.top, k.bot, q), k.name


# ---------------------------------------------------------------- 5. jnn
JNN_SETS = M.JNN_SETS


@pytest.mark.parametrize("kernels", [1, 2])
def test_jnn_param(gpu, oracle, kernels):
    import torch
    from sigtk_amd import device
    reads = M.jnn_reads()     # (the CPU test pins the oracle on these reads and sets to the reference's recorded answers)
    b = _load(reads, leads=[(5 * r) % 8 for r in range(len(reads))])
    gpu.stat_configure(kernels, 0)
    try:
        for kw in JNN_SETS:
            po = oracle.jnn_param(**kw)
            pg = gpu.JnnParam(po.std_scale, po.corrector, po.seg_dist, po.window, po.stall_len, po.error, po.top, po.bot)
            arena = device.SegArena(b)
            device.jnn(b, arena, 0, params=pg)
            torch.cuda.synchronize()
            assert int(arena.ws[:4].cpu().numpy().view(np.uint32)[0]) == 0      # no read overflowed its slots
            ns, xs, ys = arena.n_segs.cpu().numpy(), arena.x.cpu().numpy(), arena.y.cpu().numpy()
            for r, raw in enumerate(reads):
                ex, ey = oracle.jnn_raw_param(raw, po)
                s0 = int(arena.slots_host[r])
                assert int(ns[r]) == ex.size, (kw, r)
                assert np.array_equal(xs[s0:s0 + ex.size], ex) and np.array_equal(ys[s0:s0 + ex.size], ey), (kw, r)
    finally:
        gpu.stat_configure(0, 0)


# ---------------------------------------------------------------- 6. jobs
def test_job_prefix_params(gpu, oracle):
    """preset-equal parameters give the option-less job's bytes; an off-preset set the model's positions"""
    cat = _rna_reads()
    reads = [k.raw for k in cat]
    dig, off, rng = (np.array([getattr(k, f) for k in cat]) for f in ("dig", "off", "rng"))
    ap, q = M.AdaptW(0.6, 900, 1000, 50000, 300), M.POLYA_PRESET._replace(stall_len=0.5, band=25.0)
    job = gpu.Job(0)
    try:
        def run():
            job.stage(reads, dig, off, rng, None)
            job.launch(gpu.TOOL_PREFIX, rna=1, pore=0)
            return job.wait()["prefix"].copy()
        plain = run()
        job.set_prefix_params(gpu.PrefixParams.preset(1, 0))
        assert run().tobytes() == plain.tobytes()
        job.set_prefix_params(_params(gpu, ap, q))
        got = run()
        job.set_prefix_params(None)
        assert run().tobytes() == plain.tobytes()
    finally:
        job.close()
    n_real = 0
    for r, k in enumerate(cat):
        with np.errstate(all="ignore"):
            wa, wp = M.prefix_model(oracle, k.raw, k.dig, k.off, k.rng, 1, ap, q)
        n_real += 0 if M.trivial(wa) else 1
        assert (int(got[r]["adapt_x"]), int(got[r]["adapt_y"])) == wa, k.name
        assert (int(got[r]["polya_x"]), int(got[r]["polya_y"])) == wp, k.name
    assert n_real > 0


def test_job_jnn_params(gpu, oracle):
    reads = gpu.synth_reads_host(4, [3000, 20011, 40000, 9000], seed=7, kind=1)[0]
    dig, off, rng = np.full(4, P.DIG), np.full(4, P.OFF), np.full(4, P.RNG)
    job = gpu.Job(0)
    try:
        def run():
            job.stage(reads, dig, off, rng, None)
            job.launch(gpu.TOOL_JNN, rna=1)
            return [(x.copy(), y.copy()) for x, y in job.wait()["segs"]]
        same = lambda a, b: all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a, b))
        plain = run()
        kw = JNN_SETS[1]     # the dRNA preset: what rna=1 runs
        job.set_jnn_params(gpu.JnnParam(kw["std_scale"], kw["corrector"], kw["seg_dist"], kw["window"], kw["stall_len"], kw["error"], 0, 0))
        assert same(run(), plain)
        po = oracle.jnn_param(**JNN_SETS[4])
        job.set_jnn_params(gpu.JnnParam(po.std_scale, po.corrector, po.seg_dist, po.window, po.stall_len, po.error, po.top, po.bot))
        got = run()
        job.set_jnn_params(None)
        assert same(run(), plain)
    finally:
        job.close()
    assert same(got, [oracle.jnn_raw_param(raw, po) for raw in reads])
    assert sum(x.size for x, _ in got) > 0


# ---------------------------------------------------------------- 6. the command line
def _cli(*args):
    import subprocess
    from sigtk_amd import build
    p = subprocess.run([build.CLI, *args], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.fixture(scope="module")
def rna_file(tmp_path_factory):
    from sigtk_amd import blow5
    cat = _rna_reads()
    path = str(tmp_path_factory.mktemp("segparams") / "rna.blow5")
    blow5.write_blow5(path, [blow5.Read(k.name, 0, k.dig, k.off, k.rng, 4000.0, k.raw) for k in cat],
                      {"experiment_type": "rna", "sequencing_kit": "sqk-rna002"})
    return path, cat


def test_cli_presets_as_options_change_no_byte(gpu, rna_file):
    import os
    from conftest import GOLDEN
    sp1 = os.path.join(GOLDEN, "sp1_dna.blow5")
    rna = rna_file[0]
    ids = [k.name for k in rna_file[1][:3]]
    for path, seg in ((sp1, "0.75,50,50,150,0.25,5"), (rna, "0.75,50,50,1000,1,5")):
        for extra in ([], ["--gpus", "1", "--batch-samples", "30000"]):
            assert _cli("jnn", "--segmenter", seg, *extra, path).stdout == _cli("jnn", *extra, path).stdout
            want = _cli("prefix", "--print-stat", *extra, path).stdout
            assert _cli("prefix", "--print-stat", "--adaptor", "0.5,1500,2000,200000,2000", "--polya", "50,200,250,1,30,30,20",
                        *extra, path).stdout == want
            assert _cli("prefix", "--print-stat", "--polya", "50,200,250,1,30,30,20", *extra, path).stdout == want
    # read-id mode
    assert _cli("jnn", "--segmenter", "0.75,50,50,1000,1,5", rna, *ids).stdout == _cli("jnn", rna, *ids).stdout
    assert _cli("prefix", "--adaptor", "0.5,1500,2000,200000,2000", rna, *ids).stdout == _cli("prefix", rna, *ids).stdout


def test_cli_off_preset_rows_are_the_model_s(gpu, oracle, rna_file):
    path, cat = rna_file
    ap, q = M.AdaptW(0.6, 900, 1000, 50000, 300), M.POLYA_PRESET._replace(stall_len=0.5, band=25.0)
    rows, n_real = [], 0
    for k in cat:
        with np.errstate(all="ignore"):
            (ax, ay), (px, py) = M.prefix_model(oracle, k.raw, k.dig, k.off, k.rng, 1, ap, q)
        n_real += 1 if ay > 0 else 0
        cols = [str(ax), str(ay)] + ([str(px + ay), str(py + ay)] if py > 0 else [".", "."]) if ay > 0 else ["."] * 4
        rows.append("\t".join([k.name, str(k.raw.size)] + cols))
    want = ("read_id\tlen_raw_signal\tadapt_start\tadapt_end\tpolya_start\tpolya_end\n" + "\n".join(rows) + "\n").encode()
    assert n_real > 0
    p = _cli("prefix", "-v", "4", "--adaptor", "0.6,900,1000,50000,300", "--polya", "50,200,250,0.5,30,30,25", path)
    assert p.stdout == want
    assert b"adaptor route: generic; polyA route: lane, parameters" in p.stderr
    ids = [k.name for k in cat[5:9]]
    p = _cli("prefix", "-n", "--adaptor", "0.6,900,1000,50000,300", "--polya", "50,200,250,0.5,30,30,25", path, *ids)
    assert p.stdout == ("\n".join(rows[5:9]) + "\n").encode()
    # jnn: an in-domain set outside the wave kernel
    po = oracle.jnn_param(**JNN_SETS[4])
    jrows = []
    for k in cat:
        ex, ey = oracle.jnn_raw_param(k.raw, po)
        jrows.append((k.name, ex.size, ex.tolist(), ey.tolist()))
    out = _cli("jnn", "-n", "--segmenter", "0.6,17,30,32,0.5,40", path).stdout.decode().splitlines()
    assert len(out) == len(cat)
    for line, (name, n, ex, ey) in zip(out, jrows):
        f = line.split("\t")
        assert f[0] == name and int(f[2]) == n, line[:200]
        nums = [int(v) for v in f[3].replace(";", ",").replace("\t", ",").split(",") if v.strip(". ")] if len(f) > 3 else []
        assert nums == [v for pair in zip(ex, ey) for v in pair], name
