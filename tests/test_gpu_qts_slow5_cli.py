"""GPU: `sigtk-amd qts reads.slow5 -o q.slow5` -- text in, text out, the signal column written on the GPU -- against
what the reference wrote for the same files (tests/golden/make_golden_qts_slow5.py)."""
import hashlib
import json
import os
import subprocess

import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
AUX = os.path.join(GOLDEN, "qts_aux.slow5")
DIGESTS = json.load(open(os.path.join(GOLDEN, "qts_slow5.json")))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
METHODS = ("floor", "round", "fill-ones")


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


@pytest.fixture(scope="module")
def sp1_slow5(tmp_path_factory, sp1):
    path = str(tmp_path_factory.mktemp("qts_slow5") / "sp1_dna.slow5")
    blow5.write_slow5(path, sp1.reads, {k: v[0] for k, v in sp1.attrs.items()})
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == DIGESTS["sp1_dna.slow5.sha256"]   # what the digests are of
    return path


def run(*args, ok=True):
    p = subprocess.run([str(a) for a in args], capture_output=True, timeout=300)
    assert not ok or p.returncode == 0, p.stderr.decode()[-2000:]
    return p


def golden(method):
    return open(os.path.join(GOLDEN, "qts_aux.b3_%s.slow5" % method), "rb").read()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("extra", [(), ("--batch-samples", "100", "-t", "3"), ("--gpu-deflate",)], ids=["plain", "batches", "gpu-deflate"])
def test_hand_made_file_with_auxiliary_columns(cli, tmp_path, method, extra):
    outp = tmp_path / "q.slow5"
    run(cli, "qts", "-b", "3", "-m", method, *extra, AUX, "-o", outp)
    assert open(outp, "rb").read() == golden(method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("bits", [1, 3, 8])
def test_fixture_reads_in_several_batches(cli, tmp_path, sp1_slow5, method, bits):
    outp = tmp_path / "q.slow5"
    run(cli, "qts", "-b", bits, "-m", method, "--batch-samples", "5000", "-t", "3", sp1_slow5, "-o", outp)
    assert hashlib.sha256(open(outp, "rb").read()).hexdigest() == DIGESTS["sp1_dna.qts_b%d_%s.slow5.sha256" % (bits, method)]


def test_stat_of_the_output_is_stat_of_the_blow5_path(cli, tmp_path, sp1_slow5):
    qt, qb = tmp_path / "q.slow5", tmp_path / "q.blow5"
    run(cli, "qts", "-b", "3", sp1_slow5, "-o", qt)
    run(cli, "qts", "-b", "3", SP1, "-o", qb)
    a, b = run(cli, "stat", qt).stdout, run(cli, "stat", qb).stdout
    assert a == b and a.count(b"\n") == 101
    assert a != run(cli, "stat", SP1).stdout                      # (the quantiser did change the reads)


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="the reference binary has not been built (oracle.build(ref=True))")
def test_against_the_reference_live(cli, tmp_path, sp1_slow5):
    ours, theirs = tmp_path / "ours.slow5", tmp_path / "theirs.slow5"
    for inp in (AUX, sp1_slow5):
        run(cli, "qts", "-b", "2", "-m", "round", inp, "-o", ours)
        run(REF_BIN, "qts", "-b", "2", "-m", "round", inp, "-o", theirs)
        assert open(ours, "rb").read() == open(theirs, "rb").read()
        # the reference reads what we wrote (its statistics of a read of 0 samples are uninitialised memory: left out)
        n_recs = sum(1 for ln in open(ours, "rb") if ln[:1] not in (b"#", b"@"))
        a, b = (run(p, "stat", ours).stdout.split(b"\n") for p in (REF_BIN, cli))
        assert len(a) == len(b) == n_recs + 2
        assert [ln for ln in a if ln.split(b"\t")[1:2] != [b"0"]] == [ln for ln in b if ln.split(b"\t")[1:2] != [b"0"]]


def test_a_bad_token_ends_the_run_like_the_other_subtools(cli, tmp_path):
    src = open(AUX, "rb").read().split(b"\n")
    n_hdr = len([ln for ln in src if ln[:1] in (b"#", b"@")])
    recs = [src[n_hdr], src[n_hdr + 4], src[n_hdr + 5]]
    cols = recs[1].split(b"\t")
    cols[7] = cols[7].replace(b",", b",x", 1)
    recs[1] = b"\t".join(cols)
    inp = tmp_path / "bad.slow5"
    inp.write_bytes(b"\n".join(src[:n_hdr] + recs) + b"\n")
    p = run(cli, "qts", inp, "-o", tmp_path / "o.slow5", ok=False)
    assert p.returncode == 1 and b"Error in slow5_get_next. Error code -4" in p.stderr


def test_help_names_both_containers(cli):
    p = run(cli, "qts", "-h")
    assert b"Usage: sigtk qts a.blow5 -o out.blow5" in p.stdout and b"a.slow5 -o out.slow5" in p.stdout
