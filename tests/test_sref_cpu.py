"""CPU: the host side of `sigtk-amd sref` -- FASTA reader (kseq's rules), k-mer model reader, argument surface, the
no-GPU error -- and the numpy model of sref that the GPU tests use as their expectation, pinned to the goldens."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sref_model as M
from sigtk_amd import api, build


@pytest.fixture(scope="module")
def cli():
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


def run(cli, *args):
    return subprocess.run([cli, *[str(a) for a in args]], capture_output=True)


def fadump_expect(data: bytes) -> bytes:
    return b"".join(b"%s\t%d\t%016x\n" % (name, len(seq), M.fnv1a(seq)) for name, seq in M.parse_fasta(data))


def modelcheck_expect(levels: np.ndarray, k: int) -> bytes:
    return b"k\t%d\tkmers\t%d\tfnv\t%016x\n" % (k, 4 ** k, M.fnv1a(np.asarray(levels, dtype="<f4").tobytes()))


@pytest.mark.parametrize("name", M.FASTAS)
def test_fadump_follows_kseq_rules(cli, tmp_path, name):
    data = M.golden(name)
    want = fadump_expect(data)
    assert want
    p = run(cli, "_fadump", os.path.join(M.GOLDEN, name))
    assert p.returncode == 0 and p.stdout == want, p.stderr
    gz = tmp_path / (name + ".gz")
    gz.write_bytes(gzip.compress(data))
    p = run(cli, "_fadump", gz)
    assert p.returncode == 0 and p.stdout == want, p.stderr
    crlf = tmp_path / (name + ".crlf")
    crlf.write_bytes(data.replace(b"\r\n", b"\n").replace(b"\n", b"\r\n"))
    p = run(cli, "_fadump", crlf)
    assert p.returncode == 0 and p.stdout == fadump_expect(crlf.read_bytes()) == want, p.stderr


def test_fadump_line_rules_in_detail(cli, tmp_path):
    cases = [b"", b"no header at all\n", b">", b">x", b">x\n", b">x\nA", b">x\n\r", b">x\nAC\n\r", b">x\r\n\r\nACGT\r\n",
             b"junk>x y z\nAC GT\n\n\nTT\n>\nACGT\n>y\tdesc\n>z\nA\n", b">a\nACGT\n>b\nNNNN\n>c", b">t\n" + b"ACGT" * 40000 + b"\n"]
    for i, data in enumerate(cases):
        f = tmp_path / ("case%d.fa" % i)
        f.write_bytes(data)
        p = run(cli, "_fadump", f)
        assert p.returncode == 0 and p.stdout == fadump_expect(data), (data[:40], p.stdout, p.stderr)
    assert M.parse_fasta(cases[9]) == [(b"x", b"AC GTTT"), (b"", b"ACGT"), (b"y", b""), (b"z", b"A")]
    assert M.parse_fasta(b">x\r\n\r\nACGT\r\n") == [(b"x", b"\rACGT")]


def test_fadump_rejects_fastq_and_missing_files(cli, tmp_path):
    for data in (b"@r1\nACGT\n+\nIIII\n", b">r1\nACGT\n+\nIIII\n", b">ok\nACGT\n@r2\nACGT\n+\nIIII\n"):
        f = tmp_path / "reads.fq"
        f.write_bytes(data)
        p = run(cli, "_fadump", f)
        assert p.returncode == 1 and b"FASTQ" in p.stderr and p.stdout == b""
        with pytest.raises(ValueError):
            M.parse_fasta(data)
    p = run(cli, "_fadump", tmp_path / "nope.fa")
    assert p.returncode == 1 and b"cannot open" in p.stderr
    bad = tmp_path / "cut.fa.gz"
    bad.write_bytes(gzip.compress(M.golden("sref_multi.fa"))[:-200])
    p = run(cli, "_fadump", bad)
    assert p.returncode == 1 and p.stdout == b""


@pytest.mark.parametrize("k", [6, 5])
def test_modelcheck_accepts_the_golden_models(cli, tmp_path, k):
    levels = M.golden_levels(k)
    want = modelcheck_expect(levels, k)
    rna = ["--rna"] if k == 5 else []
    rs = np.random.RandomState(k)
    for i, kw in enumerate((dict(), dict(order=rs.permutation(4 ** k)), dict(k_line=False, order=rs.permutation(4 ** k)),
                            dict(extra_cols=True), dict(header=False, k_line=False), dict(extra_cols=True, header=False))):
        path = M.write_model(tmp_path / ("m%d.model" % i), levels, k, **kw)
        p = run(cli, "_modelcheck", path, *rna)
        assert p.returncode == 0 and p.stdout == want, (kw.keys(), p.stdout, p.stderr)
    # CRLF line ends and levels in other notations
    path = M.write_model(tmp_path / "sci.model", levels, k, fmt=lambda v: "%.9e" % float(v))
    text = open(path, "rb").read()
    open(path, "wb").write(text.replace(b"\n", b"\r\n"))
    p = run(cli, "_modelcheck", path, *rna)
    assert p.returncode == 0 and p.stdout == want, p.stderr


def test_modelcheck_rejects_broken_models(cli, tmp_path):
    k, levels = 6, M.golden_levels(6)
    good = open(M.write_model(tmp_path / "good.model", levels, k)).read().splitlines()
    first = next(i for i, ln in enumerate(good) if ln.startswith("AAAAAA"))

    def check(lines, word, *opts):
        f = tmp_path / "bad.model"
        f.write_text("\n".join(lines) + "\n")
        p = run(cli, "_modelcheck", f, *opts)
        assert p.returncode == 1 and p.stdout == b"" and word in p.stderr, (word, p.stderr)

    check(good[:first + 7] + good[first + 8:], b"4095 of the 4096")                       # a missing k-mer
    check(good + [good[first + 3]], b"occurs twice")                                      # a duplicate
    check(good[:first + 9] + [good[first + 9].replace("AAAAGC", "AAAANC")] + good[first + 10:], b"not A, C, G or T")
    check(good[:first + 9] + [good[first + 9].replace("AAAAGC", "aaaagc")] + good[first + 10:], b"not A, C, G or T")
    check(good[:first + 5] + ["AAACCC\tabc"] + good[first + 6:], b"not a number")         # an unparsable level
    check(good[:first + 5] + ["AAACCC"] + good[first + 6:], b"not a number")              # no level at all
    check(good[:first + 5] + ["AAACCC\t1.5x\t2"] + good[first + 6:], b"not a number")
    check(good[:first + 5] + ["AAACC\t1.5"] + good[first + 6:], b"5 letters where k is 6")
    check(good, b"6-mer model", "--rna")                                                  # a wrong k for the mode
    check(open(M.write_model(tmp_path / "m5.model", M.golden_levels(5), 5)).read().splitlines(), b"5-mer model")
    check([ln.replace("#k\t6", "#k\t7") for ln in good], b"1..6")
    check([ln.replace("#k\t6", "#k\t5") for ln in good], b"letters where k is 5")
    check(["#k\t6"], b"no k-mer lines")
    p = run(cli, "_modelcheck", tmp_path / "nope.model")
    assert p.returncode == 1 and b"cannot open" in p.stderr


def test_usage_and_the_kmer_model_requirement(cli, tmp_path):
    p = run(cli, "sref")
    assert p.returncode == 1 and p.stderr.startswith(b"Usage: sigtk sref") and b"--kmer-model FILE" in p.stderr
    for line in (b"   -h ", b"   -n ", b"   --version ", b"   --rna "):      # the reference's options (src/sref.c:240-245)
        assert line in p.stderr
    p = run(cli, "sref", "-h")
    assert p.returncode == 0 and p.stdout.startswith(b"Usage: sigtk sref") and b"--kmer-model FILE" in p.stdout
    for v in ("--version", "-V"):
        p = run(cli, "sref", v)
        assert p.returncode == 0 and p.stdout == b"sigtk 0.2.0\n"
    fa = os.path.join(M.GOLDEN, "sref_edge.fa")
    p = run(cli, "sref", fa)
    assert p.returncode == 1 and p.stdout == b"" and b"no built-in pore model" in p.stderr and b"--kmer-model" in p.stderr
    p = run(cli, "--help")
    assert p.returncode == 0 and b"sref/ss are not part of it" not in p.stdout and b"ss is not part of it" in p.stdout
    assert b"         sref " in p.stdout
    # a model of the wrong k for the mode, a FASTQ file: errors before any GPU work
    m5 = M.write_model(tmp_path / "m5.model", M.golden_levels(5), 5)
    p = run(cli, "sref", "--kmer-model", m5, fa)
    assert p.returncode == 1 and p.stdout == b"" and b"5-mer model" in p.stderr
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nIIII\n")
    p = run(cli, "sref", "--rna", "--kmer-model", m5, fq)
    assert p.returncode == 1 and p.stdout == b"" and b"FASTQ" in p.stderr


def test_sref_without_a_gpu_is_a_loud_error(cli, tmp_path):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    m6 = M.write_model(tmp_path / "m6.model", M.golden_levels(6), 6)
    p = run(cli, "sref", "--kmer-model", m6, os.path.join(M.GOLDEN, "sref_edge.fa"))
    assert p.returncode == 1 and b"no usable GPU" in p.stderr and p.stdout == b""
    # the library: every entry point says so, none computes on the host
    lib = api.load_library()
    b = api.SrefBatch(None, 0, None, 0, 6, 1, 0, 0)
    import ctypes as C
    assert lib.sgk_sref_levels(C.byref(b), None, None, None) == api.SGK_ERR_NODEVICE
    ws = (C.c_uint8 * 128)()
    assert lib.sgk_sref_text_measure(C.byref(b), None, None, C.addressof(ws) // 16 * 16 + 16, 64, None) == api.SGK_ERR_NODEVICE
    assert lib.sgk_sref_text_write(C.byref(b), None, None, 0, C.addressof(ws) // 16 * 16 + 16, 64, None) == api.SGK_ERR_NODEVICE
    pipe = C.c_void_p()
    levels = (C.c_float * 4096)()
    assert lib.sgk_sref_pipe_create(0, levels, 6, C.byref(pipe)) == api.SGK_ERR_NODEVICE and not pipe.value


@pytest.mark.parametrize("out", sorted(M.FIXTURES))
def test_numpy_model_reproduces_the_goldens(cli, tmp_path, out):
    """rank, the reverse-strand rule, the head-only rows and %f through Python's '%f' % float32, with the model the CLI
    reads from the file the helper writes (its table hash through `_modelcheck`): this is the expectation of the large
    GPU cases"""
    src, opts = M.FIXTURES[out]
    rna = "--rna" in opts
    k = 5 if rna else 6
    levels = M.golden_levels(k)
    path = M.write_model(tmp_path / "m.model", levels, k, order=np.random.RandomState(1).permutation(4 ** k))
    p = run(cli, "_modelcheck", path, *(["--rna"] if rna else []))
    assert p.returncode == 0 and p.stdout == modelcheck_expect(levels, k), p.stderr
    got = M.sref_text(M.parse_fasta(M.golden(src)), levels, k, rna, header="-n" not in opts)
    assert got == M.golden(out)
    # the spans the wrapper cuts (api.sref_spans) cover every row exactly once, in order
    recs = M.parse_fasta(M.golden(src))
    spans, row_of = api.sref_spans([len(s) for _, s in recs], k, rna, max_span=100, cuts=[1, 255, 256, 257])
    rows = M.rows_of(M.golden(out), header="-n" not in opts)
    assert int(row_of[-1]) + 1 == len(rows)
    for r, row in enumerate(rows):
        sp = spans[row_of == r]
        assert int(sp["count"].sum()) == max(row[3], 0) and int(sp["first"][0]) == 0
        assert np.array_equal(sp["first"][1:], np.cumsum(sp["count"])[:-1])
        assert set(sp["seq_len"]) == {row[1]} and set(sp["strand"]) == {int(row[2] == b"-")}


def test_host_parsers_under_asan_ubsan(tmp_path):
    """the FASTA and model readers in the sanitizer build of the host sources (build.build_cli_asan): fixtures, hostile
    line structures, truncated gzip -- exit code 0 or 1 and no sanitizer report"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    try:   # skip only where the toolchain has no sanitizer runtime; a compile error in the host sources is a failure
        subprocess.run(["gcc", "-fsanitize=address,undefined", "-o", str(tmp_path / "probe"), str(probe)], check=True,
                       capture_output=True)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build not available: %s" % e)
    cli_asan = build.build_cli_asan()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def run_a(*args):
        p = subprocess.run([cli_asan, *[str(a) for a in args]], capture_output=True, timeout=120, env=env)
        assert p.returncode in (0, 1), (args, p.returncode, p.stderr[-600:])
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr[-600:]
        return p

    for name in M.FASTAS:
        assert run_a("_fadump", os.path.join(M.GOLDEN, name)).stdout == fadump_expect(M.golden(name))
    rs = np.random.RandomState(3)
    alphabet = np.frombuffer(b">>@+\n\n\r \tACGTNacgt", dtype=np.uint8)
    for i in range(60):
        data = alphabet[rs.randint(0, alphabet.size, size=rs.randint(0, 200))].tobytes()
        f = tmp_path / "h.fa"
        f.write_bytes(data)
        p = run_a("_fadump", f)
        try:
            want = fadump_expect(data)
        except ValueError:
            assert p.returncode == 1
        else:
            assert p.returncode == 0 and p.stdout == want, data
    z = gzip.compress(M.golden("sref_multi.fa"))
    for cut in (1, 10, len(z) // 2, len(z) - 1):
        f = tmp_path / "cut.gz"
        f.write_bytes(z[:cut])
        run_a("_fadump", f)
    levels = M.golden_levels(6)
    good = M.write_model(tmp_path / "good.model", levels, 6)
    assert run_a("_modelcheck", good).returncode == 0
    text = open(good, "rb").read()
    for i in range(40):
        b = bytearray(text[:rs.randint(1, len(text))] if i % 2 else text)
        for _ in range(rs.randint(1, 5)):
            b[rs.randint(0, len(b))] = rs.randint(0, 256)
        f = tmp_path / "fuzz.model"
        f.write_bytes(bytes(b))
        run_a("_modelcheck", f)
