"""GPU: every read of the median catalogue (tests/median_cases.py) on every form of the median, bit for bit against what
the real reference returned (tests/golden/median_cases.json): the wave kernel's window, the same window merged from the
workgroups of the long path, k_moments + k_median, the 32 bins of k_moments_median, the fused stat + pA under both
implementations, the region medians of prefix, the float and int16 shims, and the CLI on two small text SLOW5 files.
A NaN needs the reference's sign bit.  No case is skipped on any form."""
import json
import os
import subprocess

import numpy as np
import pytest

import median_cases as mc
from sigtk_amd import build

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 12345
FIELDS = ("raw_mean", "pa_mean", "raw_std", "pa_std", "pa_median")


@pytest.fixture(scope="module")
def cases():
    return mc.cases()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "median_cases.json")))


def same_bits(got, want_bits):
    gb = int(np.float32(got).view(np.uint32))
    if gb == want_bits:
        return True
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000  # noqa: E731
    return nan(gb) and nan(want_bits) and (gb >> 31) == (want_bits >> 31)


def _place(cases, n_fill=0):
    """the reads at their leads, `n_fill` 8-sample fillers behind them, the gaps full of a sentinel"""
    import torch
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(5)
    fill = rs.randint(480, 520, size=(n_fill, 8)).astype(np.int16)
    lens = np.array([c.raw.size for c in cases] + [8] * n_fill, dtype=np.int64)
    leads = np.array([c.lead for c in cases] + [0] * n_fill, dtype=np.int64)
    b = device.alloc_reads(lens, dev, leads=leads)
    host = np.full(b.n_samples, SENTINEL, dtype=np.int16)
    for r, c in enumerate(cases):
        o = int(b.offsets_host[r])
        host[o:o + c.raw.size] = c.raw
    if n_fill:
        o = b.offsets_host[len(cases):].astype(np.int64)
        host[(o[:, None] + np.arange(8)[None, :]).ravel()] = fill.ravel()
    b.samples.copy_(torch.from_numpy(host).to(dev))
    n = len(cases)
    for name, t, dflt in (("dig", b.dig, mc.DIG), ("off", b.off, mc.OFF), ("rng", b.rng, mc.RNG)):
        v = np.full(n + n_fill, dflt, dtype=np.float64)
        v[:n] = [getattr(c, name) for c in cases]
        t[:b.n_reads] = torch.from_numpy(v).to(dev)
    return b, host, fill


def _wrong(cases, golden, rec):
    bad = []
    for r, c in enumerate(cases):
        g = golden["stat"][c.name]
        what = [f for f, bts in zip(FIELDS, g["bits"]) if not same_bits(rec[f][r], bts)]
        if int(rec["raw_median"][r]) != g["raw_median"]:
            what.append("raw_median")
        if int(rec["n"][r]) != g["n"]:
            what.append("n")
        if int(rec["reserved"][r]) != 0:
            what.append("reserved")
        if what:
            bad.append("%s: %s" % (c.name, ",".join(what)))
    return bad


def _stat(gpu, b):
    from sigtk_amd import device
    return device.stat(b).cpu().numpy().view(gpu.STAT_DTYPE)


@pytest.fixture
def configure(gpu):
    yield gpu.stat_configure
    gpu.stat_configure(0, 0)


def test_wave(gpu, configure, cases, golden):
    """k_stat_wave's 2048-bin window, k_median for what it flags"""
    configure(2, -1)
    b, _, _ = _place(cases)
    bad = _wrong(cases, golden, _stat(gpu, b))
    assert not bad, "\n".join(bad)


def test_long(gpu, configure, cases, golden):
    """reads of 8192 samples and more on k_long_chains (the window merged from its workgroups), the rest on the wave"""
    from sigtk_amd import device
    configure(2, 8192)
    b, _, _ = _place(cases)
    rec = _stat(gpu, b)
    st = device.long_status(b, "stat")
    assert st.n_long_reads == sum(1 for c in cases if c.raw.size >= 8192) and st.n_long_reads > 40
    assert st.n_timeouts == 0
    bad = _wrong(cases, golden, rec)
    assert not bad, "\n".join(bad)


def test_lane_small_batch(gpu, configure, cases, golden):
    """k_moments + k_median on every read (2048 / 8192 bins, the two-level select behind them)"""
    configure(1, 0)
    b, _, _ = _place(cases)
    assert b.n_reads < 81920
    bad = _wrong(cases, golden, _stat(gpu, b))
    assert not bad, "\n".join(bad)


def test_lane_32_bins(gpu, configure, cases, golden):
    """the same reads in a batch of 81 920 and more: the medians out of k_moments' 32 bins per lane"""
    configure(1, 0)
    n_fill = 81920 + 64 - len(cases)
    b, _, fill = _place(cases, n_fill)
    rules = [r for r in gpu.stat_lane_rules() if r[0] == 0]
    assert b.n_reads >= max(r[1] for r in rules) == 81920     # the row from which k_moments_median is launched
    assert gpu.stat_plan("stat", b.n_reads, b.n_samples, b.max_read_len).kernels == 1
    assert b.total_samples < 4000000
    L = gpu.load_library()
    L.sgk_profile_reset(); L.sgk_profile_enable(1)
    try:
        rec = _stat(gpu, b)
    finally:
        L.sgk_profile_enable(0)
    launched = set(gpu.profile_read())
    L.sgk_profile_reset()
    assert {"k_moments_median", "k_median_flagged", "k_median_literal"} <= launched and "k_median" not in launched, launched
    bad = _wrong(cases, golden, rec[:len(cases)])
    assert not bad, "\n".join(bad)
    f = rec[len(cases):]
    assert np.array_equal(f["raw_median"], np.sort(fill, axis=1)[:, 4]) and not f["reserved"].any()


@pytest.mark.parametrize("kernels", [1, 2])
def test_fused_stat_pa(gpu, oracle, configure, cases, golden, kernels):
    """stat + pA: the records as above, every pA sample the oracle's, the gaps between the reads untouched"""
    import torch
    from sigtk_amd import device
    configure(kernels, -1)
    b, host, _ = _place(cases)
    pa0 = torch.full((b.n_samples,), float(SENTINEL), dtype=torch.float32, device=b.samples.device)
    rec, pa = device.stat_pa(b, pa0)
    rec, pa = rec.cpu().numpy().view(gpu.STAT_DTYPE), pa.cpu().numpy()
    bad = _wrong(cases, golden, rec)
    assert not bad, "\n".join(bad)
    want = np.full(b.n_samples, float(SENTINEL), dtype=np.float32)
    with np.errstate(all="ignore"):
        for r, c in enumerate(cases):
            o = int(b.offsets_host[r])
            want[o:o + c.raw.size] = oracle.pa(c.raw, c.dig, c.off, c.rng)
    gv, wv = pa.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(pa) & np.isnan(want) & ((gv >> 31) == (wv >> 31))
    diff = np.flatnonzero((gv != wv) & ~nan)
    assert diff.size == 0, (diff[:8], pa[diff[:8]], want[diff[:8]])


def _prefix_wrong(gpu, rg, golden, pre):
    bad = []
    for r, k in enumerate(rg):
        g = golden["region"][k.name]
        what = []
        if (int(pre["adapt_x"][r]), int(pre["adapt_y"][r])) != tuple(g["adapt"]):
            what.append("adapt")
        if (int(pre["polya_x"][r]), int(pre["polya_y"][r])) != tuple(g["polya"]):
            what.append("polya")
        for f, bts in zip(("adapt_mean", "adapt_std", "adapt_median"), g["adapt_bits"]):
            if not same_bits(pre[f][r], bts):
                what.append(f)
        if g["polya"][1] > 0:
            for f, bts in zip(("polya_mean", "polya_std", "polya_median"), g["polya_bits"]):
                if not same_bits(pre[f][r], bts):
                    what.append(f)
        if int(pre["reserved"][r]) != 0:
            what.append("reserved")
        if what:
            bad.append("%s: %s" % (k.name, ",".join(what)))
    return bad


@pytest.mark.parametrize("kernels,n_fill", [(1, 0), (2, 0), (0, 49152)])
def test_regions(gpu, configure, golden, kernels, n_fill):
    """the region medians of prefix under both implementations, and in a batch of 49 152 reads and more, where the wave
    finders hand their regions to the lane kernels (lane_regions && !lanes)"""
    from sigtk_amd import device
    rg = mc.region_cases()
    configure(kernels, 0)
    b, _, _ = _place(rg, n_fill)
    if n_fill:
        assert gpu.stat_plan("prefix", b.n_reads, b.n_samples, b.max_read_len).kernels == 2
        assert [r for r in gpu.stat_lane_rules() if r[0] == 4][0][1] <= b.n_reads
    pre = device.prefix(b, 1, mc.REGION_PORE).cpu().numpy().view(gpu.PREFIX_DTYPE)
    bad = _prefix_wrong(gpu, rg, golden, pre)
    assert not bad, "\n".join(bad)
    assert (pre["adapt_y"][len(rg):] <= 0).all()     # (the fillers are too short for an adaptor)


# ---- the workspace decides whether a pick can be redone: a smaller one must never give a silently different median
def _is_pick(c, raw=None):
    """what k_median_literal redoes: pA(raw order statistic) is a zero, or the unit or offset is not finite"""
    raw = c.raw if raw is None else raw
    with np.errstate(all="ignore"):
        rule = mc.pa_rule(c._replace(raw=raw))
        fin = np.isfinite(mc.unit_of(c.dig, c.rng)) and np.isfinite(np.float32(c.off))
    return raw.size >= 1 and (rule == 0 or not fin)


def _rule_bits_ok(got, c, raw=None):
    """pA(raw order statistic), bit for bit; where that is a NaN (0 * inf) any NaN: which sign the GPU's own multiplication
    gives it is not the reference's business on this path, which the record marks as inexact"""
    with np.errstate(all="ignore"):
        rule = mc.pa_rule(c._replace(raw=c.raw if raw is None else raw))
    return (np.isnan(rule) and np.isnan(got)) or np.float32(got).view(np.uint32) == np.float32(rule).view(np.uint32)


def _ws_sizes(gpu, b, tool):
    """(0.2.3 size: order + long reads, no scratch row; that + three rows; the full size)"""
    import torch
    L = gpu.load_library()
    base = int(L.sgk_jnn_workspace_bytes(b.n_reads, b.n_samples, b.max_read_len))   # the same two parts, and nothing else
    full = int(getattr(L, "sgk_%s_workspace_bytes" % tool)(b.n_reads, b.n_samples, b.max_read_len))
    row = 2 * ((b.max_read_len + 7) // 8 * 8)
    assert full == base + min(b.n_reads, 1024) * row      # (under the byte cap of SGK_LITERAL_MAX_BYTES)
    return [("none", base), ("three", base + 3 * row + 5), ("full", full)], torch


def _literal_status(gpu, ws, n_reads):
    import ctypes as C
    import torch
    torch.cuda.synchronize()
    st = gpu.LiteralStatus()
    gpu.check(gpu.load_library().sgk_stat_literal_status(C.c_void_p(ws.data_ptr()), ws.numel(), n_reads, C.byref(st)), "status")
    return st.n_literal, st.n_inexact


@pytest.mark.parametrize("kernels", [1, 2])
def test_stat_with_smaller_workspaces(gpu, configure, cases, golden, kernels):
    """sgk_stat_opt with no scratch row (the 0.2.3 workspace), with three rows and with all of them"""
    import ctypes as C
    configure(kernels, 0)
    b, _, _ = _place(cases)
    picks = [r for r, c in enumerate(cases) if _is_pick(c)]
    assert len(picks) >= 60 and any(cases[r].raw.size == 1 for r in picks)
    sizes, torch = _ws_sizes(gpu, b, "stat")
    L, view = gpu.load_library(), b.view()
    for label, nbytes in sizes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=b.samples.device)
        out = torch.zeros(b.n_reads * gpu.STAT_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
        gpu.check(L.sgk_stat_opt(C.byref(view), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), None,
                                 C.byref(gpu.STAT_OPTIONS)), "sgk_stat_opt")
        n_lit, n_inexact = _literal_status(gpu, ws, b.n_reads)
        rec = out.cpu().numpy().view(gpu.STAT_DTYPE).copy()
        if label == "none":
            assert (n_lit, n_inexact) == (0, len(picks)), label
            flagged = np.flatnonzero(rec["reserved"]).tolist()
            assert flagged == picks and (rec["reserved"][picks] == 4).all()          # SGK_MEDIAN_INEXACT
            wrong = [cases[r].name for r in picks if not _rule_bits_ok(rec["pa_median"][r], cases[r])]
            assert not wrong, wrong
            for r in picks:          # (everything else in those records is the reference's)
                rec["pa_median"][r] = np.uint32(golden["stat"][cases[r].name]["bits"][4]).view(np.float32)
            rec["reserved"][picks] = 0
        else:
            assert (n_lit, n_inexact) == (len(picks), 0), label
        bad = _wrong(cases, golden, rec)
        assert not bad, label + "\n" + "\n".join(bad)


def test_prefix_with_smaller_workspaces(gpu, configure, golden):
    """sgk_prefix_opt likewise: the adaptor picks keep SGK_MEDIAN_INEXACT, the polyA pick SGK_MEDIAN_INEXACT_POLYA"""
    import ctypes as C
    configure(2, 0)
    rg = mc.region_cases()
    b, _, _ = _place(rg)
    regs = {}
    for r, k in enumerate(rg):
        g = golden["region"][k.name]
        (ax, ay), (px, py) = g["adapt"], g["polya"]
        regs[r] = (k.raw[ax:ay], k.raw[ay + px:ay + py] if py > 0 else None)
    a_picks = [r for r, k in enumerate(rg) if _is_pick(k, regs[r][0])]
    p_picks = [r for r, k in enumerate(rg) if regs[r][1] is not None and _is_pick(k, regs[r][1])]
    assert len(a_picks) >= 5 and [rg[r].name for r in p_picks] == ["region_polya_zero"]
    sizes, torch = _ws_sizes(gpu, b, "prefix")
    L, view = gpu.load_library(), b.view()
    for label, nbytes in sizes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=b.samples.device)
        out = torch.zeros(b.n_reads * gpu.PREFIX_DTYPE.itemsize, dtype=torch.uint8, device=b.samples.device)
        gpu.check(L.sgk_prefix_opt(C.byref(view), 1, mc.REGION_PORE, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                   ws.numel(), None, C.byref(gpu.STAT_OPTIONS)), "sgk_prefix_opt")
        n_lit, n_inexact = _literal_status(gpu, ws, b.n_reads)
        pre = out.cpu().numpy().view(gpu.PREFIX_DTYPE).copy()
        if label == "none":
            assert (n_lit, n_inexact) == (0, len(a_picks) + len(p_picks)), label
            want = np.zeros(b.n_reads, dtype=np.uint32)
            want[a_picks] |= 4          # SGK_MEDIAN_INEXACT
            want[p_picks] |= 8          # SGK_MEDIAN_INEXACT_POLYA
            assert np.array_equal(pre["reserved"], want), (pre["reserved"], want)
            for r in a_picks:
                assert _rule_bits_ok(pre["adapt_median"][r], rg[r], regs[r][0]), rg[r].name
                pre["adapt_median"][r] = np.uint32(golden["region"][rg[r].name]["adapt_bits"][2]).view(np.float32)
            for r in p_picks:
                assert _rule_bits_ok(pre["polya_median"][r], rg[r], regs[r][1]), rg[r].name
                pre["polya_median"][r] = np.uint32(golden["region"][rg[r].name]["polya_bits"][2]).view(np.float32)
            pre["reserved"][:] = 0
        else:
            assert (n_lit, n_inexact) == (len(a_picks) + len(p_picks), 0), label
        bad = _prefix_wrong(gpu, rg, golden, pre)
        assert not bad, label + "\n" + "\n".join(bad)


def test_the_scratch_rows_are_capped(gpu):
    """one very long read among many: the rows stop at SGK_LITERAL_MAX_BYTES, and one read alone always gets its row"""
    L = gpu.load_library()
    base = int(L.sgk_jnn_workspace_bytes(2000, 10 ** 9, 3000000))
    assert int(L.sgk_stat_workspace_bytes(2000, 10 ** 9, 3000000)) - base == (256 << 20) // 6000000 * 6000000
    base = int(L.sgk_jnn_workspace_bytes(1, 2 * 10 ** 8, 2 * 10 ** 8))
    assert int(L.sgk_prefix_workspace_bytes(1, 2 * 10 ** 8, 2 * 10 ** 8)) - base == 4 * 10 ** 8


def test_float_shim(gpu, golden):
    """sgk_meanf / sgk_stdvf / sgk_medianf: the radix on float keys, +-0, NaNs, +-inf, denormals, the field seams"""
    bad = []
    for k in mc.float_cases():
        got = gpu.shim_stat_f32(k.x)
        what = [f for f, v, bts in zip(("mean", "stdv", "median"), got, golden["float"][k.name]["bits"]) if not same_bits(v, bts)]
        if what:
            bad.append("%s: %s" % (k.name, ",".join(what)))
    assert not bad, "\n".join(bad)


def test_int16_shim(gpu, cases, golden):
    names = ("edge2048_n1001_k@lo", "edge2048_n1001_k@lo+nb-1", "edge8192_n65537_k@lo-1", "mirror2048_n1000_k_in_k2_out",
             "select_med-20000_n1001", "select_distinct_20001", "all_32767_n9", "all_-32768_n1001", "len1_pos", "len2_neg",
             "len65536_pos", "clamp_low_n501", "trunc_mean_-0.5_edge2048_n1001")
    by = {c.name: c for c in cases}
    for nm in names:
        c, g = by[nm], golden["stat"][nm]
        mean, sd, med = gpu.shim_stat_i16(c.raw)
        assert med == g["raw_median"] and same_bits(mean, g["bits"][0]) and same_bits(sd, g["bits"][2]), nm


@pytest.mark.parametrize("which,want,args", [
    ("range0", "median_range0.stat.tsv", ["stat"]),
    ("prefix", "median_prefix.prefix_stat.tsv", ["prefix", "--print-stat"]),
])
def test_cli(gpu, tmp_path, which, want, args):
    """sigtk-amd on two small text SLOW5 files (six reads under `range 0`; the region reads), written here as
    tests/golden/make_golden_median_cases.py wrote them for the reference: byte for byte what the reference printed,
    plain and --host-decode"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_median_cases", os.path.join(GOLDEN, "make_golden_median_cases.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    src = str(tmp_path / "cases.slow5")
    (mk.write_range0_slow5 if which == "range0" else mk.write_prefix_slow5)(src)
    gold = open(os.path.join(GOLDEN, want), "rb").read()
    for extra in ([], ["--host-decode"]):
        p = subprocess.run([build.CLI] + args + extra + [src], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert p.stdout == gold, (extra, p.stdout.decode()[:1500])
