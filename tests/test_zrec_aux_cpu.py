"""CPU: the table of a BLOW5 header's auxiliary columns (b5_aux_fields, through `sigtk-amd _dump --aux FILE`), which
decides whether a file's records go to the GPU compressed and what k_zrec_tail checks them against; and the writer of
sigtk_amd/blow5.py with auxiliary columns, certified by the real reference reading its files."""
import os
import subprocess

import numpy as np
import pytest

from sigtk_amd import blow5, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def aux_line(cli, path):
    p = subprocess.run([cli, "_dump", "--aux", path], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p.stdout.decode()


def header_only(path, aux_types):
    blow5.write_blow5(path, [], {"asic_id": "1"}, aux_types=aux_types)
    return path


@pytest.mark.parametrize("name", ["sp1_dna.blow5", "sp1_dna.zstd_svb.blow5"])
def test_table_of_the_bundled_fixture(cli, name):
    """uint64_t int32_t uint8_t double enum{..} char*: five fixed columns and channel_number, a 1-byte array"""
    assert aux_line(cli, os.path.join(GOLDEN, name)) == "#aux\t6\t8\t4\t1\t8\t1\t1*\n"


def test_array_columns_of_every_kind(cli, tmp_path):
    path = header_only(str(tmp_path / "a.blow5"), [("d", "double*"), ("e", "enum{a,b}*"), ("h", "int16_t*")])
    assert aux_line(cli, path) == "#aux\t3\t8*\t1*\t2*\n"
    every = [("a", "int8_t"), ("b", "uint8_t"), ("c", "char"), ("d", "int16_t"), ("e", "uint16_t"), ("f", "int32_t"),
             ("g", "uint32_t"), ("h", "float"), ("i", "int64_t"), ("j", "uint64_t"), ("k", "double"), ("l", "enum{x}")]
    path = header_only(str(tmp_path / "b.blow5"), every + [(n + "s", t + "*") for n, t in every])
    sizes = ["1", "1", "1", "2", "2", "4", "4", "4", "8", "8", "8", "1"]
    assert aux_line(cli, path) == "#aux\t24\t" + "\t".join(sizes + [s + "*" for s in sizes]) + "\n"


def test_no_auxiliary_columns_is_an_empty_table(cli, tmp_path):
    assert aux_line(cli, header_only(str(tmp_path / "n.blow5"), None)) == "#aux\t0\n"


@pytest.mark.parametrize("bad", ["string", "uint128_t", "enum{a,b", "double**", "*"])
def test_an_unknown_type_name_gives_no_table(cli, tmp_path, bad):
    path = header_only(str(tmp_path / "u.blow5"), [("ok", "double"), ("bad", bad), ("ok2", "char*")])
    assert aux_line(cli, path) == "#aux\tnone\n"


def test_files_without_the_new_arguments_are_unchanged(tmp_path, sp1):
    a, b = str(tmp_path / "a.blow5"), str(tmp_path / "b.blow5")
    blow5.write_blow5(a, sp1.reads[:3], {"k": "v"})
    blow5.write_blow5(b, sp1.reads[:3], {"k": "v"}, aux_types=None)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    assert b"int16_t*\n#read_id" in data and data.endswith(b"5WOLB")
    assert sp1.reads[0].aux is None


def test_the_reference_reads_what_the_writer_writes(tmp_path, sp1):
    """string, empty-array and double* columns among fixed ones: `sigtk_ref stat` takes the file and prints the rows it
    prints for the same reads without auxiliary columns; read_blow5 keeps skipping the tails"""
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref has not been built")
    reads = sp1.reads[:6]
    aux_types = [("channel_number", "char*"), ("median_before", "double"), ("nothing", "int16_t*"), ("end_reason", "enum{a,b,c}"),
                 ("levels", "double*"), ("start_time", "uint64_t")]
    with_aux = [blow5.Read(r.read_id, r.read_group, r.digitisation, r.offset, r.range, r.sampling_rate, r.raw,
                           aux=("ch%d" % (100 * i), 200.5 + i, [], i % 3, [1.5, -2.25, float(i)], 12345 + i))
                for i, r in enumerate(reads)]
    attrs = {a: sp1.attr(a) for a in sp1.attrs}
    a, b = str(tmp_path / "aux.blow5"), str(tmp_path / "plain.blow5")
    blow5.write_blow5(a, with_aux, attrs, aux_types=aux_types)
    blow5.write_blow5(b, reads, attrs)
    pa = subprocess.run([REF, "stat", a], capture_output=True)
    pb = subprocess.run([REF, "stat", b], capture_output=True)
    assert pa.returncode == 0 and pb.returncode == 0, (pa.stderr[-500:], pb.stderr[-500:])
    assert pa.stdout == pb.stdout and pa.stdout.count(b"\n") == 1 + len(reads)
    back = blow5.read_blow5(a)
    assert [r.read_id for r in back.reads] == [r.read_id for r in reads]
    assert all(np.array_equal(x.raw, y.raw) for x, y in zip(back.reads, reads))
