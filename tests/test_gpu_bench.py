"""GPU: bench.py's plain run and --dump-outputs.  The plain run prints the headline line alone (the secondary
figures are --full's), and the arrays it dumps are what the timed path computed: event counts of every read and the
events of the sampled reads, checked against the oracle on the same seeded reads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sigtk_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_what_the_path_computed(gpu, oracle, tmp_path):
    n_reads, read_len = 300, 20000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--reads", str(n_reads), "--read-len", str(read_len), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"roofline", "cpu_baseline", "parity_spot_check"} & set(d)

    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert np.array_equal(out["per_read_reads"], np.arange(n_reads))
    sample = out["sample_reads"].astype(np.int64)
    assert 0 < sample.size < n_reads and np.all(np.diff(sample) > 0)

    # bench config 2: DNA parameters, seed 1, kind 0 -- the device generator equals the host one
    reads, dig, off, rng = api.synth_reads_host(n_reads, read_len, 1, 0)
    exp = [oracle.event_raw(reads[r], dig[r], off[r], rng[r], 0) for r in range(n_reads)]
    assert np.array_equal(out["n_events"], [e.start.size for e in exp])
    cat = [np.concatenate([getattr(exp[r], f) for r in sample]) for f in ("start", "length", "mean", "stdv")]
    assert np.array_equal(out["event_start"], cat[0].astype(np.float64))
    assert np.array_equal(out["event_length"], cat[1].astype(np.float64))
    assert np.array_equal(out["event_mean"].view(np.uint32), cat[2].view(np.uint32))
    assert np.array_equal(out["event_stdv"].view(np.uint32), cat[3].view(np.uint32))
