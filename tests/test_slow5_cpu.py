"""CPU: text SLOW5 through the host reader of the sigtk-amd CLI (sigtk_amd/host/blow5.c) -- header, records, the
scalar signal parser b5_sigtext_decode, the .idx index -- and sigtk_amd.blow5.write_slow5 / read_slow5.  The text
files are generated from the committed sp1_dna.blow5."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sigtk_amd import blow5, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOW5 = os.path.join(GOLDEN, "sp1_dna.blow5")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")

HEAD = ("#slow5_version\t0.2.0\n#num_read_groups\t1\n@experiment_type\tgenomic_dna\n"
        "#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
        "#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n")


@pytest.fixture(scope="module")
def cli():
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


@pytest.fixture(scope="module")
def sp1_slow5(tmp_path_factory, sp1):
    path = str(tmp_path_factory.mktemp("slow5") / "sp1_dna.slow5")
    blow5.write_slow5(path, sp1.reads, {k: v[0] for k, v in sp1.attrs.items()})
    return path


def run(cli, *args, **kw):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120, **kw)


def fnv(raw):
    h = 1469598103934665603
    for v in np.asarray(raw, dtype=np.int16).astype(np.uint16).tolist():
        h ^= v
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def record(rid="r0", group="0", dig="8192", off="3", rng="1402.5", rate="4000", n="3", sig="1,2,3", aux=()):
    return "\t".join([rid, group, dig, off, rng, rate, n, sig, *aux]) + "\n"


def write(tmp_path, name, text):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(text.encode("latin-1"))
    return path


def records_of(stdout):
    """the record lines of a _dump (its first line names the compression of the container, which differs)"""
    lines = stdout.split("\n")
    assert lines[0].startswith("#press\t") and lines[0].endswith("\tgroups\t1")
    return lines[1:]


# ---------------------------------------------------------------------------------------------- dump equality

def test_python_writer_and_reader_round_trip(sp1, sp1_slow5):
    back = blow5.read_slow5(sp1_slow5)
    assert back.version == (0, 2, 0) and back.num_read_groups == 1 and back.attrs == sp1.attrs
    assert len(back.reads) == len(sp1.reads)
    for a, b in zip(sp1.reads, back.reads):
        assert (a.read_id, a.read_group, a.digitisation, a.offset, a.range, a.sampling_rate) == \
               (b.read_id, b.read_group, b.digitisation, b.offset, b.range, b.sampling_rate)
        assert np.array_equal(a.raw, b.raw)
    assert blow5._plain_double(1e-7) == "0.0000001" and blow5._plain_double(4000.0) == "4000"
    assert "e" not in blow5._plain_double(1.2345678901234567e-9) and float(blow5._plain_double(-0.1)) == -0.1


@pytest.mark.parametrize("extra", [[], ["--split"], ["--map"]])
def test_dump_equals_the_blow5_dump(cli, sp1_slow5, extra):
    want = run(cli, "_dump", *extra, BLOW5)
    got = run(cli, "_dump", *extra, sp1_slow5)
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    assert got.stdout.split("\n")[0] == "#press\t0\t0\tgroups\t1"
    assert records_of(got.stdout) == records_of(want.stdout) and len(records_of(got.stdout)) == 101


def test_read_id_access_and_the_index(cli, sp1, tmp_path, sp1_slow5):
    path = str(tmp_path / "a.slow5")
    shutil.copy(sp1_slow5, path)
    all_rows = records_of(run(cli, "_dump", path).stdout)
    ids = [sp1.reads[i].read_id for i in (0, 49, 99)]
    for i, rid in zip((0, 49, 99), ids):
        for extra in ([], ["--split"]):
            p = run(cli, "_dump", *extra, "--id", rid, path)
            assert p.returncode == 0 and p.stdout == all_rows[i] + "\n", (extra, p.stderr)
    assert run(cli, "_dump", "--id", "no-such-read", path).returncode == 1
    # the index: the reference's container, an entry per line (its offset, its length with the newline)
    idx = open(path + ".idx", "rb").read()
    assert len(idx) == 64 + sum(2 + len(r.read_id) + 16 for r in sp1.reads) + 8 == 5472
    assert idx[:12] == b"SLOW5IDX\x01\x00\x02\x00" and idx.endswith(b"XDI5WOLS")
    data = open(path, "rb").read()
    first = len(data) - sum(len(line) + 1 for line in data.decode().split("\n")[-101:-1])
    import struct
    idl = struct.unpack_from("<H", idx, 64)[0]
    off, size = struct.unpack_from("<QQ", idx, 66 + idl)
    assert idx[66:66 + idl].decode() == ids[0] and off == first and data[off + size - 1:off + size] == b"\n"
    assert data[off:off + idl].decode() == ids[0]
    # reused: a second run leaves it alone
    before = os.stat(path + ".idx").st_mtime_ns
    assert run(cli, "_dump", "--id", ids[1], path).stdout == all_rows[49] + "\n"
    assert os.stat(path + ".idx").st_mtime_ns == before
    # rejected when it belongs to another file: the same reads in another order under the same name
    blow5.write_slow5(path, sp1.reads[::-1], {k: v[0] for k, v in sp1.attrs.items()})
    for extra in ([], ["--split"]):
        open(path + ".idx", "wb").write(idx)
        p = run(cli, "_dump", *extra, "--id", ids[1], path)
        assert p.returncode == 0 and p.stdout == all_rows[49] + "\n", (extra, p.stderr)


def test_reference_reads_our_file_and_writes_the_same_index(cli, sp1, tmp_path, sp1_slow5):
    if not os.path.exists(REF_BIN):
        pytest.skip("the reference has not been built (oracle/_ref)")
    ours, theirs = str(tmp_path / "ours.slow5"), str(tmp_path / "ref" / "ours.slow5")
    os.mkdir(str(tmp_path / "ref"))
    shutil.copy(sp1_slow5, ours)
    shutil.copy(sp1_slow5, theirs)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(REF_BIN))
    p = subprocess.run([REF_BIN, "stat", theirs], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stdout == open(os.path.join(GOLDEN, "sp1_dna.stat.tsv")).read()
    rid = sp1.reads[49].read_id
    assert subprocess.run([REF_BIN, "stat", theirs, rid], capture_output=True, env=env).returncode == 0
    assert run(cli, "_dump", "--id", rid, ours).returncode == 0
    assert open(ours + ".idx", "rb").read() == open(theirs + ".idx", "rb").read()


# ---------------------------------------------------------------------------------------------- host parser grammar

GOOD = [("0", [0]), ("-1", [-1]), ("-32768", [-32768]), ("32767", [32767]), ("7,-32768,0,32767", [7, -32768, 0, 32767]),
        ("", [])]
BAD = [("32768", 1), ("-32769", 1), ("01", 1), ("-0", 1), ("-", 1), ("1-2", 1), (",5,6", 3), ("5,,6", 3), ("5,6,", 3),
       ("123456", 1), ("1 2", 1), (" 1", 1), ("1,2", 3), ("1,2,3", 2), ("1,-,1-2", 3), ("", 1), ("1", 0), ("1\x002", 1),
       ("+1", 1), ("1.0", 1)]


@pytest.mark.parametrize("extra", [[], ["--split"], ["--map"]])
def test_signal_grammar(cli, tmp_path, extra):
    for k, (sig, vals) in enumerate(GOOD):
        path = write(tmp_path, "good%d.slow5" % k, HEAD + record(n=str(len(vals)), sig=sig) + record("r1"))
        p = run(cli, "_dump", *extra, path)
        assert p.returncode == 0, (sig, p.stderr)
        rows = records_of(p.stdout)
        assert rows[0] == "r0\t%d\t8192\t3\t1402.5\t%016x" % (len(vals), fnv(vals)), (sig, rows)
        assert rows[1] == "r1\t3\t8192\t3\t1402.5\t%016x" % fnv([1, 2, 3])
    for k, (sig, n) in enumerate(BAD):
        path = write(tmp_path, "bad%d.slow5" % k, HEAD + record("r1") + record(n=str(n), sig=sig))
        p = run(cli, "_dump", *extra, path)
        assert p.returncode == 1, (sig, n, p.stdout)
        assert records_of(p.stdout)[0].startswith("r1\t3\t")        # the record in front of it was read
        for more in ([], ["--split"]):
            assert run(cli, "_dump", *more, "--id", "r0", path).returncode == 1, (sig, n)
            assert run(cli, "_dump", *more, "--id", "r1", path).returncode == 0


HOSTILE = {
    "seven_columns": HEAD + "r0\t0\t8192\t3\t1402.5\t4000\t3\n",
    "no_num_read_groups": HEAD.replace("#num_read_groups\t1\n", "") + record(),
    "no_version": HEAD.replace("#slow5_version\t0.2.0\n", "") + record(),
    "no_names_line": HEAD.rsplit("#read_id", 1)[0] + record(),
    "columns_out_of_order": HEAD.replace("digitisation\toffset", "offset\tdigitisation") + record(),
    "no_final_newline": HEAD + record() + record("r1")[:-1],
    "len_2_pow_32": HEAD + record(n=str(1 << 32)),
    "len_2_pow_64": HEAD + record(n=str(1 << 64)),
    "len_huge_for_its_column": HEAD + record(n="4000000000"),
    "len_leading_zero": HEAD + record(n="03"),
    "len_negative": HEAD + record(n="-3"),
    "exponent_double": HEAD + record(rng="1.4e3"),
    "nan_double": HEAD + record(off="nan"),
    "empty_double": HEAD + record(dig=""),
    "group_not_a_number": HEAD + record(group="x"),
    "empty_id": HEAD + record(rid=""),
    "empty_line": HEAD + "\n",
    "only_tabs": HEAD + "\t\t\t\t\t\t\t\n",
    "nul_in_line": HEAD + "r0\t0\t81\x0092\t3\t1402.5\t4000\t3\t1,2,3\n",
}


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_header_and_line_errors(cli, tmp_path, name):
    path = write(tmp_path, name + ".slow5", HOSTILE[name])
    for extra in ([], ["--split"], ["--map"], ["--id", "r0"], ["--split", "--id", "r0"]):
        p = run(cli, "_dump", *extra, path)
        assert p.returncode == 1, (name, extra, p.stdout, p.stderr)


def test_format_by_extension_and_by_content(cli, tmp_path, sp1_slow5):
    as_blow5, anon = str(tmp_path / "text.blow5"), str(tmp_path / "text.dat")
    shutil.copy(sp1_slow5, as_blow5)
    shutil.copy(sp1_slow5, anon)
    assert run(cli, "_dump", as_blow5).returncode == 1       # the extension decides, as in slow5_open
    assert run(cli, "_dump", anon).returncode == 0           # no known extension: the first bytes do
    as_slow5 = str(tmp_path / "binary.slow5")
    shutil.copy(BLOW5, as_slow5)
    assert run(cli, "_dump", as_slow5).returncode == 1


def test_auxiliary_columns_are_ignored(cli, tmp_path):
    head = HEAD.replace("\tint16_t*\n", "\tint16_t*\tuint64_t\tchar*\n").replace("\traw_signal\n", "\traw_signal\tstart_time\tchannel\n")
    plain = write(tmp_path, "plain.slow5", HEAD + record() + record("r1", sig="-5,6,7"))
    aux = write(tmp_path, "aux.slow5", head + record(aux=("12345", "ch-1")) + record("r1", sig="-5,6,7", aux=("9", "1,2,x")))
    for extra in ([], ["--split"], ["--map"]):
        a, b = run(cli, "_dump", *extra, plain), run(cli, "_dump", *extra, aux)
        assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout
    assert run(cli, "_dump", "--id", "r1", aux).stdout == run(cli, "_dump", "--split", "--id", "r1", plain).stdout


def test_qts_refuses_text_files(cli, tmp_path, sp1_slow5):
    for args in ((sp1_slow5, "-o", str(tmp_path / "out.blow5")), (BLOW5, "-o", str(tmp_path / "out.slow5"))):
        p = run(cli, "qts", *args)
        assert p.returncode == 1 and "qts on text SLOW5 files is not supported" in p.stderr
        assert not os.path.exists(args[2])
    anon = str(tmp_path / "text.dat")
    shutil.copy(sp1_slow5, anon)
    p = run(cli, "qts", anon, "-o", str(tmp_path / "out2.blow5"))
    assert p.returncode == 1 and "not supported" in p.stderr


# ---------------------------------------------------------------------------------------------- sanitizers

@pytest.fixture(scope="module")
def cli_asan():
    try:
        return build.build_cli_asan()
    except (subprocess.CalledProcessError, OSError) as e:  # no libasan in this toolchain
        pytest.skip("sanitizer build not available: %s" % e)


def test_hostile_text_files_under_asan_ubsan(cli_asan, tmp_path, sp1_slow5):
    """the stand-alone host build with -fsanitize=address,undefined over the same files: exit 0 or 1, no report"""
    import random
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def run_a(*args):
        p = subprocess.run([cli_asan, *args], capture_output=True, timeout=120, env=env)
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-600:])
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr[-600:]
        return p

    files = [write(tmp_path, name + ".slow5", text) for name, text in sorted(HOSTILE.items())]
    files += [write(tmp_path, "g%d.slow5" % k, HEAD + record(n=str(len(v)), sig=s)) for k, (s, v) in enumerate(GOOD)]
    files += [write(tmp_path, "b%d.slow5" % k, HEAD + record("r1") + record(n=str(n), sig=s)) for k, (s, n) in enumerate(BAD)]
    for path in files:
        for extra in ([], ["--split"], ["--map"], ["--id", "r0"], ["--split", "--id", "r0"]):
            run_a("_dump", *extra, path)
    ok = str(tmp_path / "sp1.slow5")
    shutil.copy(sp1_slow5, ok)
    for extra in ([], ["--split"], ["--map"]):
        assert run_a("_dump", *extra, ok).returncode == 0
    # truncations and byte flips of the real file
    data = open(ok, "rb").read()
    rnd = random.Random(7)
    for k in range(12):
        mut = bytearray(data)
        if k % 2:
            mut = mut[: rnd.randrange(1, len(mut))]
        else:
            for _ in range(3):
                mut[rnd.randrange(len(mut))] = rnd.choice(b"\t\n,-0 9\x00\xff")
        path = str(tmp_path / ("mut%d.slow5" % k))
        open(path, "wb").write(bytes(mut))
        for extra in ([], ["--map"], ["--split", "--id", "02ccee70-91c5-41ef-be4d-158529bef274"]):
            run_a("_dump", *extra, path)
