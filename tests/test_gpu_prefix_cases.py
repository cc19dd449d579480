"""GPU parity: every branch of the adaptor and polyA finders on every implementation of them.

The reads are the hand-made catalogue of tests/prefix_cases.py (tests/test_prefix_cases_cpu.py proves that every branch of
the reference's two loops is taken by one of them, tests/test_oracle_vs_ref.py that the oracle equals the real reference
on all of them).  Each finder exists three times on the GPU -- one read per lane (k_adaptor / k_polya), one wavefront per
read (k_adaptor_wave / k_polya_wave, which jump over tile masks and stop early) and the long-read chains (k_long_chains)
-- and every one of them is compared with the ORACLE here: positions as integers, mean / std / median as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import prefix_cases as P
from test_gpu_stat import _check_prefix

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#: stat_configure arguments: one read per lane; one wavefront per read and nothing else; one wavefront per read with
#: everything above 8192 samples on the long-read chains; what the library picks
CONFIGS = {"lane": (1, 0), "wave": (2, -1), "wave+long8192": (2, 8192), "default": (0, 0)}


class CachedOracle:
    """oracle.prefix once per (read, scaling, rna, pore): the four implementations are compared with the same record"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def prefix(self, raw, dig, off, rng, rna, pore):
        key = (raw.ctypes.data, raw.size, repr((float(dig), float(off), float(rng))), rna, pore)
        if key not in self.memo:
            with np.errstate(all="ignore"):
                self.memo[key] = self.oracle.prefix(raw, dig, off, rng, rna, pore)
        return self.memo[key]


@pytest.fixture(scope="module")
def cat():
    return P.catalogue()


@pytest.fixture(scope="module")
def ref(oracle):
    return CachedOracle(oracle)


def _scal(cases):
    return (np.array([k.dig for k in cases]), np.array([k.off for k in cases]), np.array([k.rng for k in cases]))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_whole_catalogue(gpu, ref, cat, config):
    reads = [k.raw for k in cat]
    dig, off, rng = _scal(cat)
    gpu.stat_configure(*CONFIGS[config])
    try:
        got = {(rna, pore): gpu.prefix(reads, dig, off, rng, rna, pore) for rna in (0, 1) for pore in (0, 2)}
    finally:
        gpu.stat_configure(0, 0)
    failures = []
    for (rna, pore), g in got.items():
        for r, k in enumerate(cat):   # read by read, so that a failure names the read; all of them are reported
            try:
                _check_prefix(ref, [k.raw], [k.dig], [k.off], [k.rng], rna, pore, [g[r]])
            except AssertionError as e:
                failures.append("%s rna %d pore %d %s: %s | gpu %r" % (config, rna, pore, k.name, str(e).split("\n")[0], g[r].tolist()))
        if not rna:
            assert all(int(x["polya_x"]) == -1 and int(x["polya_y"]) == -1 for x in g)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("config", ["lane", "wave", "default"])
def test_tile_geometry_at_odd_sample_offsets(gpu, ref, cat, config):
    """the reads whose run edges sit on the wave kernel's tile positions (and the tuned one-window / on-threshold ones),
    packed back to back behind fillers of odd lengths so that they start at every sample offset modulo 8; whatever lies
    between and around the reads is 12345"""
    import torch
    from sigtk_amd import device
    pick = [k for k in cat if k.name.startswith(("edges_", "one_window_", "threshold_on_slope", "gap_seg_dist", "pa_stretch_2",
                                                 "pa_merge", "pa_nomerge", "pa_tile_edge", "scale_decreasing_polya"))]
    filler = P.sig((2009, 480), noise=30, seed=77)
    reads, sc, cur = [], [], 256
    for i, k in enumerate(pick):
        flen = 2001 + ((2 * i + 1) - (cur + 2001)) % 8     # the next read starts at offset = 2 i + 1 (mod 8): always odd
        reads.append(filler[:flen]); sc.append((P.DIG, P.OFF, P.RNG))
        reads.append(k.raw); sc.append((k.dig, k.off, k.rng))
        cur += flen + k.raw.size
    dig, off, rng = (np.array([s[j] for s in sc]) for j in range(3))
    dev = torch.device("cuda", 0)
    b = device.alloc_reads(np.array([r.size for r in reads], dtype=np.int64), dev, align=1)
    assert all(int(b.offsets_host[2 * i + 1]) % 8 == (2 * i + 1) % 8 for i in range(len(pick)))
    host = np.full(b.n_samples, 12345, dtype=np.int16)
    for r, raw in enumerate(reads):
        o = int(b.offsets_host[r]); host[o:o + raw.size] = raw
    b.samples.copy_(torch.from_numpy(host).to(dev))
    b.dig.copy_(torch.from_numpy(dig).to(dev)); b.off.copy_(torch.from_numpy(off).to(dev)); b.rng.copy_(torch.from_numpy(rng).to(dev))
    gpu.stat_configure(*CONFIGS[config])
    try:
        got = {pore: np.frombuffer(device.prefix(b, 1, pore).cpu().numpy().tobytes(), dtype=gpu.PREFIX_DTYPE)[:len(reads)]
               for pore in (0, 2)}
        torch.cuda.synchronize()
    finally:
        gpu.stat_configure(0, 0)
    for pore, g in got.items():
        _check_prefix(ref, reads, dig, off, rng, 1, pore, g)


def test_job_api_longest_first(gpu, ref, cat):
    """more than 1024 reads through the job API (the catalogue's reads of up to 30 000 samples, 17 times over): the wave
    kernels take them in the order of the device-side sort by length; same records as the direct call, and the oracle's"""
    small = [k for k in cat if k.raw.size <= 30000]
    cases = small * 17
    assert len(cases) >= 1024
    reads = [k.raw for k in cases]
    dig, off, rng = _scal(cases)
    for pore in (0, 2):
        job = gpu.Job(0)
        try:
            job.stage(reads, dig, off, rng, None)
            job.launch(gpu.TOOL_PREFIX, rna=1, pore=pore)
            got = job.wait()["prefix"].copy()
        finally:
            job.close()
        direct = gpu.prefix(reads, dig, off, rng, 1, pore)
        for name in ("adapt_x", "adapt_y", "polya_x", "polya_y", "n"):
            assert np.array_equal(got[name], direct[name]), name
        for name, valid in (("adapt", direct["adapt_y"] > 0), ("polya", direct["polya_y"] > 0)):
            for f in ("_mean", "_std", "_median"):
                assert np.array_equal(got[name + f].view(np.uint32)[valid], direct[name + f].view(np.uint32)[valid]), name + f
        _check_prefix(ref, reads, dig, off, rng, 1, pore, got)


def test_shims(gpu, oracle, cat):
    """the per-read calls with the reference's signatures: jnnv2 with hi / lo / seg_dist set ON the read's own run length
    and run gap (and one off), find_adaptor on every catalogue read, find_polya on the pA arrays no raw read can form"""
    for k in P.shim_cases():
        xy, rc = gpu.shim_jnnv2(k.raw, gpu.Jnnv2Param(k.p.std_scale, k.p.seg_dist, 2000, 0.0, k.p.hi, k.p.lo))
        assert rc == 0 and xy == oracle.jnnv2(k.raw, k.p.std_scale, k.p.seg_dist, k.p.hi, k.p.lo), k.name
    for k in cat:
        for pore in (0, 2):
            assert gpu.shim_find_adaptor(k.raw, pore) == oracle.find_adaptor(k.raw, pore), (k.name, pore)
    for k in P.pa_cases():
        for pore in (0, 2):
            assert gpu.shim_find_polya(k.pa, k.top, k.bot, pore) == oracle.find_polya(k.pa, k.top, k.bot, pore), (k.name, pore)


@pytest.mark.parametrize("fname,kit", [("prefix_cases_r9.prefix_stat.tsv", "sqk-rna002"),
                                       ("prefix_cases_rna004.prefix_stat.tsv", "sqk-rna004")])
def test_cli_is_byte_identical_to_the_reference(gpu, cat, tmp_path, fname, kit):
    """`sigtk-amd prefix --print-stat` on the part of the catalogue a BLOW5 file can hold, against what the reference CLI
    printed for the same file (tests/golden/make_golden_prefix.py); batch and decode options do not change a byte"""
    from sigtk_amd import blow5, build
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    path = str(tmp_path / "cases.blow5")
    recs = [blow5.Read(k.name, 0, k.dig, k.off, k.rng, 4000.0, k.raw) for k in P.finite_cases(cat)]
    blow5.write_blow5(path, recs, {"experiment_type": "rna", "sequencing_kit": kit})
    want = open(os.path.join(GOLDEN, fname), "rb").read()
    for opts in ([], ["--batch-samples", "30000", "--threads", "3"], ["--host-decode", "-t", "1"]):
        p = subprocess.run([build.CLI, "prefix", "--print-stat", *opts, path], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert p.stdout == want, "options %s: first differing row %r" % (
            opts, next((a, b) for a, b in zip(p.stdout.split(b"\n") + [b""], want.split(b"\n")) if a != b))
