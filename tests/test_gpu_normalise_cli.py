"""GPU: `sigtk-amd pa --normalise zscore|medmad` against rows made by formatting the model's output
(tests/normalise_model.py on Oracle.pa) with "%f": the whole file in one batch and in many, read-id mode, -n, the other
record paths and a text SLOW5 file.  Degenerate reads are checked through the API (tests/test_gpu_normalise.py)."""
import os
import subprocess

import pytest

import normalise_model as nm
from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
SLOW5 = os.path.join(GOLDEN, "qts_aux.slow5")
HEADER = b"read_id\tlen_raw_signal\tnorm\n"
METHODS = {"zscore": nm.ZSCORE, "medmad": nm.MEDMAD}


@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def out(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def _rows(reads, oracle, reflib):
    """{method name: [row of every read]}, computed once per file"""
    statf = nm.statf_of(oracle, reflib)
    rows = {}
    for name, method in METHODS.items():
        rows[name] = []
        for r in reads:
            y, _ = nm.normalise(oracle.pa(r.raw, r.digitisation, r.offset, r.range), method, statf)
            rows[name].append(("%s\t%d\t%s\n" % (r.read_id, y.size, ",".join("%f" % float(v) for v in y))).encode())
    return rows


@pytest.fixture(scope="module")
def sp1_rows(sp1, oracle, reflib):
    return _rows(sp1.reads, oracle, reflib)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_whole_file_in_one_batch_and_in_many(cli, sp1_rows, method):
    want = HEADER + b"".join(sp1_rows[method])
    assert out(cli, "pa", "--normalise", method, SP1) == want
    assert out(cli, "pa", "--normalise", method, "--batch-samples", "20000", SP1) == want
    assert out(cli, "pa", "--batch-samples", "200000", "-t", "3", "--normalise", method, SP1) == want
    # the records inflated and the signal decoded on the host instead
    assert out(cli, "pa", "--normalise", method, "--host-inflate", SP1) == want
    assert out(cli, "pa", "--normalise", method, "--host-decode", SP1) == want
    assert out(cli, "pa", "--normalise", method, "--gpus", "1", SP1) == want


@pytest.mark.parametrize("method", sorted(METHODS))
def test_read_ids_no_header_and_output_option(cli, sp1, sp1_rows, method, tmp_path):
    picks = [7, 0, 99, 42]
    ids = [sp1.reads[k].read_id for k in picks]
    want = b"".join(sp1_rows[method][k] for k in picks)
    assert out(cli, "pa", "--normalise", method, SP1, *ids) == HEADER + want
    assert out(cli, "pa", "-n", "--normalise", method, SP1, *ids) == want
    assert out(cli, "pa", "--normalise", method, "-n", SP1) == b"".join(sp1_rows[method])
    # -o is accepted and ignored, as for pa
    assert out(cli, "pa", "--normalise", method, "-o", str(tmp_path / "unused"), SP1, ids[0]) == HEADER + sp1_rows[method][picks[0]]


def test_pa_itself_is_unchanged(cli):
    plain = out(cli, "pa", SP1)
    assert plain.startswith(b"read_id\tlen_raw_signal\tpa\n")
    assert plain != out(cli, "pa", "--normalise", "zscore", SP1)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_text_slow5(cli, oracle, reflib, method):
    """(the fixture has a read of no samples and one of one sample: 0 / 0.  Python prints every NaN as "nan", C's "%f" prints the sign the
    device's NaN happens to have, which IEEE leaves open: the one token is compared without it)"""
    reads = blow5.read_slow5(SLOW5).reads
    assert sorted(r.raw.size for r in reads)[:2] == [0, 1]
    want = HEADER + b"".join(_rows(reads, oracle, reflib)[method])
    assert want.count(b"nan") == 1
    assert out(cli, "pa", "--normalise", method, SLOW5).replace(b"-nan", b"nan") == want
    assert out(cli, "pa", "--normalise", method, "--host-decode", SLOW5).replace(b"-nan", b"nan") == want
