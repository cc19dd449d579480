"""GPU: the sigtk-amd CLI on a text SLOW5 file reproduces the reference's stdout byte for byte -- the committed goldens
of sp1_dna.blow5, on the same reads written as text (the reference prints the same for both containers) -- with the
signal column parsed on the GPU (default), on the host threads (--host-decode) and with the rows formatted on the GPU
(--gpu-text); and SGK_SIGNAL_TEXT jobs against SGK_SIGNAL_INT16 jobs."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
IDS3 = ["00011a60-dd92-4aad-be1d-59a33545ab1d", "0448591b-036c-4cc7-a702-6c542ccc07de",
        "03880e3d-b79d-4bd8-aab4-15724f1331af"]


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


@pytest.fixture(scope="module")
def slow5(tmp_path_factory, sp1):
    path = str(tmp_path_factory.mktemp("slow5") / "sp1_dna.slow5")
    blow5.write_slow5(path, sp1.reads, {k: v[0] for k, v in sp1.attrs.items()})
    return path


def out(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


MODES = {"gpu-parse": [], "host-decode": ["--host-decode"], "gpu-text": ["--gpu-text"]}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("fname,args", [
    ("sp1_dna.event_c.tsv", ["event", "-c"]),
    ("sp1_dna.stat.tsv", ["stat"]),
    ("sp1_dna.jnn.tsv", ["jnn"]),
    ("sp1_dna.jnn_c.tsv", ["jnn", "-c"]),
    ("sp1_dna.prefix.tsv", ["prefix"]),
    ("sp1_dna.prefix_stat.tsv", ["prefix", "--print-stat"]),
    ("sp1_dna.ent.tsv", ["ent"]),
])
def test_sp1_goldens(cli, slow5, fname, args, mode):
    assert out(cli, *args, *MODES[mode], slow5) == gold(fname)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("tool", ["pa", "event"])
def test_sp1_large_outputs_by_hash(cli, slow5, tool, mode):
    assert hashlib.sha256(out(cli, tool, *MODES[mode], slow5)).hexdigest() == MANIFEST["sp1_dna.%s.tsv.sha256" % tool]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_options_and_read_id_mode(cli, slow5, mode):
    m = MODES[mode]
    assert out(cli, "pa", *m, slow5, *IDS3) == gold("sp1_dna.pa3.tsv")
    assert out(cli, "event", "-c", "-n", *m, slow5) == gold("sp1_dna.event_c.tsv").split(b"\n", 1)[1]
    # many small batches, several threads: rows still in file order
    assert out(cli, "stat", "--batch-samples", "5000", "-t", "3", *m, slow5) == gold("sp1_dna.stat.tsv")


def test_read_id_mode_equals_the_blow5_run(cli, slow5):
    for tool in (["event"], ["stat"], ["prefix", "--print-stat"]):
        assert out(cli, *tool, slow5, *IDS3) == out(cli, *tool, SP1, *IDS3)


@pytest.mark.parametrize("mode", ["gpu-parse", "host-decode"])
@pytest.mark.parametrize("bad", ["12,0x3,4", "1,2", "5,,6"])
def test_bad_token_ends_the_run_like_a_read_error(cli, tmp_path, sp1, mode, bad):
    path = str(tmp_path / "bad.slow5")
    blow5.write_slow5(path, sp1.reads[:3], {k: v[0] for k, v in sp1.attrs.items()})
    with open(path, "ab") as fh:
        fh.write(("poisoned\t0\t8192\t3\t1402.5\t4000\t3\t%s\n" % bad).encode())
    p = subprocess.run([cli, "stat", *MODES[mode], path], capture_output=True)
    assert p.returncode == 1
    assert b"Error in slow5_get_next. Error code -4" in p.stderr, p.stderr[-500:]


# ---------------------------------------------------------------------------------------------- job level

def test_text_jobs_equal_int16_jobs(gpu, sp1):
    reads = sp1.reads[:24]
    raws = [r.raw for r in reads] + [np.zeros(0, np.int16), np.array([-32768], np.int16)]
    dig = [8192.0] * len(raws); off = [3.0] * len(raws); rng = [1402.882324] * len(raws)
    texts = [blow5.slow5_signal_text(r) for r in raws]
    counts = [r.size for r in raws]
    job = gpu.Job(0)
    try:
        for tool, flags in ((gpu.TOOL_EVENT, 0), (gpu.TOOL_EVENT, gpu.JOB_EVENTS_LENGTHS), (gpu.TOOL_STAT, 0)):
            job.submit(tool, raws, dig, off, rng, flags=flags)
            want = job.wait()
            job.submit(tool, texts, dig, off, rng, flags=flags, counts=counts, text=True)
            got = job.wait()
            if tool == gpu.TOOL_STAT:
                assert got["stat"].tobytes() == want["stat"].tobytes()
            else:
                for a, b in zip(got["events"], want["events"]):
                    assert np.array_equal(a.start, b.start) and np.array_equal(a.length, b.length)
                    assert a.mean.tobytes() == b.mean.tobytes() and a.stdv.tobytes() == b.stdv.tobytes()
        # rows formatted on the GPU from a text batch
        ids = ["read-%d" % i for i in range(len(raws))]
        job.submit(gpu.TOOL_PA, raws, dig, off, rng, flags=gpu.JOB_TEXT, ids=ids)
        want = job.wait()["text"]
        job.submit(gpu.TOOL_PA, texts, dig, off, rng, flags=gpu.JOB_TEXT, counts=counts, ids=ids, text=True)
        assert job.wait()["text"] == want and len(want) > 0
        # a poisoned batch: refused, the status says which read and why, and the job takes the next batch
        bad = list(texts); bad_counts = list(counts)
        bad[3] = bad[3][:100] + b"x" + bad[3][101:]     # a byte that is no digit
        bad_counts[7] += 1                              # one token short of what the record announces
        job.stage(bad, dig, off, rng, counts=bad_counts, text=True)
        job.launch(gpu.TOOL_STAT)
        rc, ds = job.wait_rc()
        assert rc == gpu.SGK_ERR_FORMAT
        want_ds = np.zeros(len(raws), np.uint32); want_ds[3] = 2; want_ds[7] = 1
        assert np.array_equal(ds, want_ds)
        with pytest.raises(gpu.SigtkGpuError):        # qts does not take text input
            job.stage(texts, dig, off, rng, counts=counts, text=True)
            job.launch_qts(2, 1, False)
        job.submit(gpu.TOOL_STAT, texts, dig, off, rng, counts=counts, text=True)
        got = job.wait()
        job.submit(gpu.TOOL_STAT, raws, dig, off, rng)
        assert got["stat"].tobytes() == job.wait()["stat"].tobytes()
    finally:
        job.close()
