"""GPU parity: every branch of the segmenter on every implementation of it.

The reads are the hand-made catalogue of tests/jnn_cases.py (tests/test_jnn_cases_cpu.py proves that every branch of the
reference's loop and every special place of the GPU forms -- chunk ends against sync samples, candidates against lanes
and merge rounds, staging areas that run over -- is taken by one of them, tests/test_oracle_vs_ref.py that the oracle
equals the real reference on all of them, the err-- correction included).  jnn_core exists four times on the GPU: one
read per lane (k_jnn, also the redo of what the others give up on), one wavefront per read (k_jnn_wave), the long-read
chains (k_long_chains) and the float form behind jnn_pa (k_jnn_f32).  Every one of them is compared with the ORACLE
here, segment by segment as integers; there are no tolerances."""
import os
import subprocess

import numpy as np
import pytest

import jnn_cases as J

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#: stat_configure arguments: one read per lane; one wavefront per read and nothing else; one wavefront per read with
#: everything above 8192 samples on the long-read chains; what the library picks
CONFIGS = {"lane": (1, 0), "wave": (2, -1), "wave+long8192": (2, J.LONG_MIN), "default": (0, 0)}
SCALE = (8192.0, 10.0, 1402.882324)
#: the BLOW5 headers the CLI picks the preset by (as tests/golden/make_golden_jnn.py wrote them)
HEADERS = {"dna": {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"},
           "rna": {"experiment_type": "rna", "sequencing_kit": "sqk-rna002"}}


def _pairs(x, y):
    return [(int(a), int(b)) for a, b in zip(x, y)]


@pytest.fixture(scope="module")
def cat():
    return J.catalogue()


@pytest.fixture(scope="module")
def want(oracle, cat):
    """the oracle's segments, once: {run label: [(x, y)]} (jnn_cases.case_runs) and a memo for other reads"""
    memo = {}
    with np.errstate(all="ignore"):
        for k in cat:
            for label, p in J.case_runs(k):
                memo[label] = _pairs(*oracle.jnn_raw_param(k.raw, oracle.jnn_param(**p._asdict())))
    return memo


def _scal(n):
    return tuple(np.full(n, v) for v in SCALE)


def _configured(gpu, config, fn):
    gpu.stat_configure(*CONFIGS[config])
    try:
        return fn()
    finally:
        gpu.stat_configure(0, 0)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_whole_catalogue_presets(gpu, want, cat, config):
    """every preset case through the subtool with either preset; the reads whose staging areas run over (on the wave path
    and on the long path) are among them, and their answer -- k_jnn_redo's -- is the oracle's like everyone else's"""
    cases = J.preset_cases(cat)
    reads = [k.raw for k in cases]
    assert {"no_sync_16384", "no_sync_40000", "no_sync_all_5000"} <= {k.name for k in cases}
    got = _configured(gpu, config, lambda: {rna: gpu.jnn(reads, *_scal(len(reads)), rna) for rna in (0, 1)})
    failures = []
    for rna, g in got.items():
        for k, (x, y) in zip(cases, g):   # read by read, so that a failure names the read; all of them are reported
            if _pairs(x, y) != want["%s/rna%d" % (k.name, rna)]:
                failures.append("%s rna %d %s: gpu %r oracle %r" % (config, rna, k.name, _pairs(x, y)[:6], want["%s/rna%d" % (k.name, rna)][:6]))
    assert not failures, "\n".join(failures)


def test_whole_catalogue_own_parameters(gpu, want, cat):
    """every case with parameters of its own through the per-read call, which reaches the launch rule (wave or lane by
    the parameters: error 0 / 31 / 32 / -1, window 127 / 128, error against the corrector) with the library's own choice
    of kernels; the presets passed as parameters must give what the subtool gives"""
    failures = []
    for k in cat:
        if k.params is None and k.raw.size > 5000:
            continue
        for label, p in J.case_runs(k):
            got = gpu.shim_jnn_raw(k.raw, gpu.JnnParam(*p))
            if got != want[label]:
                failures.append("%s %r: gpu %r oracle %r" % (label, tuple(p), got[:6], want[label][:6]))
    assert not failures, "\n".join(failures)


def test_jnn_pa_cases(gpu, oracle):
    """jnn_pa on the float arrays no raw read can form: NaN and infinite samples, -0.0, samples ON a float threshold, NaN
    thresholds out of a NaN sample, and the err-- correction"""
    failures = []
    with np.errstate(all="ignore"):
        for k in J.pa_cases():
            e = _pairs(*oracle.jnn_pa(k.pa, oracle.jnn_param(**k.params._asdict())))
            got = gpu.shim_jnn_pa(k.pa, gpu.JnnParam(*k.params))
            if got != e:
                failures.append("%s: gpu %r oracle %r" % (k.name, got[:6], e[:6]))
    assert not failures, "\n".join(failures)


PACKED = ("sync_", "span_chunks", "weak_", "merge_across_empty", "lanes_49_50", "no_sync_16384", "no_sync_all_5000", "rich_511",
          "rich_512", "rich_513", "first_rule_", "window_1", "merge_49", "nomerge_50", "scattered_close", "open_at_0", "n1", "n2")


@pytest.mark.parametrize("config", ["lane", "wave", "default"])
def test_geometry_at_every_sample_offset(gpu, oracle, want, cat, config):
    """the tuned reads packed back to back behind fillers of odd lengths, each of them eight times so that it starts at
    every sample offset modulo 8 (the chunks are laid out from the 16-byte boundary in front of the read); whatever lies
    between and around the reads is 12345, and the last read ends on the buffer's last sample"""
    import dataclasses
    import torch
    from sigtk_amd import device
    pick = [k for k in cat if k.params is None and k.name.startswith(PACKED)]
    assert len(pick) >= 25
    filler = J.rich(331, 77)
    reads, names, cur = [], [], 256
    for j in range(8):
        for i, k in enumerate(pick):
            flen = 301 + ((i + j) - (cur + 301)) % 8      # this copy starts at offset i + j (mod 8)
            reads.append(filler[:flen]); names.append(None)
            reads.append(k.raw); names.append(k.name)
            cur += flen + k.raw.size
    tail = J.io(-20, 200, -30, 160, -(6 + (-(cur + 416)) % 8))   # ends on a multiple of 8: the end of the buffer
    reads.append(tail); names.append(None)
    cur += tail.size
    dev = torch.device("cuda", 0)
    b = device.alloc_reads(np.array([r.size for r in reads], dtype=np.int64), dev, align=1)
    assert cur % 8 == 0 and int(b.offsets_host[-1]) + tail.size == cur and cur <= b.n_samples
    starts = {}
    for r, name in enumerate(names):
        if name:
            starts.setdefault(name, set()).add(int(b.offsets_host[r]) % 8)
    assert all(v == set(range(8)) for v in starts.values())
    host = np.full(cur, 12345, dtype=np.int16)
    for r, raw in enumerate(reads):
        o = int(b.offsets_host[r]); host[o:o + raw.size] = raw
    b = dataclasses.replace(b, samples=torch.from_numpy(host).to(dev), n_samples=cur)
    for t, v in zip((b.dig, b.off, b.rng), SCALE):
        t.fill_(v)
    arena = device.SegArena(b)

    def run(rna):
        device.jnn(b, arena, rna)
        torch.cuda.synchronize()
        ns, x, y = arena.n_segs.cpu().numpy(), arena.x.cpu().numpy(), arena.y.cpu().numpy()
        assert int(arena.ws[:4].cpu().numpy().view(np.uint32)[0]) == 0
        return [_pairs(x[s:s + n], y[s:s + n]) for s, n in zip(arena.slots_host[:-1], ns)]
    got = _configured(gpu, config, lambda: {rna: run(rna) for rna in (0, 1)})
    failures = []
    for rna, g in got.items():
        for r, name in enumerate(names):
            e = want["%s/rna%d" % (name, rna)] if name else _pairs(*oracle.jnn_raw(reads[r], rna))
            if g[r] != e:
                failures.append("%s rna %d read %d (%s, offset %d mod 8): gpu %r oracle %r" % (
                    config, rna, r, name or "filler", int(b.offsets_host[r]) % 8, g[r][:6], e[:6]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("config", ["lane", "wave", "wave+long8192"])
def test_caller_sized_slots(gpu, want, cat, config):
    """the device API with slot ranges of the caller's choosing, one read per call, canaries either side of seg_x / seg_y:
    exactly as many slots as segments and nseg in (cap / 2, cap] (the wave kernel's lower half is too small: the redo must
    still be right); one slot too few, one slot, no slot: the first `cap` segments are right, the capacity error is
    counted, and nothing is written outside the slots"""
    import torch
    from sigtk_amd import device
    dev = torch.device("cuda", 0)
    CANARY, G = 0x5A5A5A5A, 64
    by_name = {k.name: k for k in cat}
    failures = []

    def run():
        for name in ("lanes_49_50", "rich_5000_seed4", "rich_16384", "no_sync_16384"):
            raw, e = by_name[name].raw, want[name + "/rna0"]
            nseg = len(e)
            assert nseg >= 2 or name == "no_sync_16384"
            b = device.upload_reads([raw], *_scal(1), dev)
            for cap in sorted({nseg, 2 * nseg - 1, nseg + 1, nseg - 1, 1, 0}):
                arena = device.SegArena(b)
                full_x = torch.full((cap + 2 * G,), CANARY, dtype=torch.int32, device=dev)
                full_y = torch.full((cap + 2 * G,), CANARY, dtype=torch.int32, device=dev)
                arena.x, arena.y = full_x[G:], full_y[G:]
                arena.slots = torch.tensor([0, cap], dtype=torch.int64, device=dev)
                device.jnn(b, arena, 0)
                torch.cuda.synchronize()
                x, y = full_x.cpu().numpy(), full_y.cpu().numpy()
                ns = int(arena.n_segs.cpu().numpy().view(np.uint32)[0])
                nerr = int(arena.ws[:4].cpu().numpy().view(np.uint32)[0])
                what = "%s %s cap %d (nseg %d)" % (config, name, cap, nseg)
                for a in (x, y):
                    if not ((a[:G] == CANARY).all() and (a[G + cap:] == CANARY).all()):
                        failures.append(what + ": written outside the slots")
                k = min(cap, nseg)
                if ns != nseg or _pairs(x[G:G + k], y[G:G + k]) != e[:k]:
                    failures.append("%s: n_segs %d, gpu %r oracle %r" % (what, ns, _pairs(x[G:G + k], y[G:G + k])[:6], e[:6]))
                if (nerr != 0) != (cap < nseg):
                    failures.append("%s: err_count %d" % (what, nerr))
    _configured(gpu, config, run)
    assert not failures, "\n".join(failures)


def test_job_api_longest_first(gpu, want, cat):
    """more than 1024 reads through the job API (the preset cases of up to 5000 samples, many times over): the wave kernel
    takes them in the order of the device-side sort by length; same segments as the direct call, and the oracle's"""
    small = [k for k in J.preset_cases(cat) if k.raw.size <= 5000]
    cases = small * (1024 // len(small) + 1)
    assert len(cases) >= 1024
    reads = [k.raw for k in cases]
    dig, off, rng = _scal(len(reads))
    for rna in (0, 1):
        job = gpu.Job(0)
        try:
            job.stage(reads, dig, off, rng, None)
            job.launch(gpu.TOOL_JNN, rna=rna)
            got = [_pairs(x, y) for x, y in job.wait()["segs"]]
        finally:
            job.close()
        direct = [_pairs(x, y) for x, y in gpu.jnn(reads, dig, off, rng, rna)]
        bad = [(r, k.name) for r, k in enumerate(cases) if got[r] != direct[r] or got[r] != want["%s/rna%d" % (k.name, rna)]]
        assert not bad, "rna %d: %r" % (rna, bad[:10])


@pytest.mark.parametrize("kind", ["dna", "rna"])
def test_cli_is_byte_identical_to_the_reference(gpu, cat, tmp_path, kind):
    """`sigtk-amd jnn` and `jnn -c` on a BLOW5 of the preset cases, against what the reference CLI printed for the same
    file (tests/golden/make_golden_jnn.py); batch and decode options do not change a byte"""
    from sigtk_amd import blow5, build
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    path = str(tmp_path / "cases.blow5")
    recs = [blow5.Read(k.name, 0, *SCALE, 4000.0, k.raw) for k in J.preset_cases(cat)]
    blow5.write_blow5(path, recs, HEADERS[kind])
    for fname, tool in (("jnn_cases_%s.jnn.tsv" % kind, ["jnn"]), ("jnn_cases_%s.jnn_c.tsv" % kind, ["jnn", "-c"])):
        want = open(os.path.join(GOLDEN, fname), "rb").read()
        for opts in ([], ["--batch-samples", "30000", "--threads", "3"], ["--host-decode", "-t", "1"]):
            p = subprocess.run([build.CLI, *tool, *opts, path], capture_output=True)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert p.stdout == want, "%s options %s: first differing row %r" % (
                fname, opts, next((a, b) for a, b in zip(p.stdout.split(b"\n") + [b""], want.split(b"\n")) if a != b))
