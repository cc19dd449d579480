"""CPU: `sigtk-amd ss paf2tsv` -- the host path (--host-decode) against the reference's recorded output for every fixture,
the argument surface, the no-GPU error, the divergences from the reference against the Python model of
tests/ss_model.py, the live reference when it has been built, and the reader under the sanitizer build."""
import os
import subprocess

import numpy as np
import pytest

import ss_model as M
from sigtk_amd import api, build

REF = os.path.join(M.ROOT, "oracle", "_ref", "sigtk_ref")
USAGE = b"Usage: sigtk ss paf2tsv in.paf\n"


@pytest.fixture(scope="module")
def cli():
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


def run(cli, *args):
    return subprocess.run([cli, *[str(a) for a in args]], capture_output=True, timeout=120)


def host(cli, path, *opts):
    return run(cli, "ss", "paf2tsv", "--host-decode", *opts, path)


def check_against_model(cli, tmp_path, data: bytes, *opts, word=None):
    """the CLI's stdout, exit status and (for the Bad ss lines) stderr equal the model's"""
    f = tmp_path / "case.paf"
    f.write_bytes(data)
    out, rc, err = M.paf2tsv(data)
    p = host(cli, f, *opts)
    assert p.returncode == rc, (p.returncode, rc, p.stderr[-300:])
    assert p.stdout == out
    if rc and err.startswith(b"Bad ss"):
        assert p.stderr == err + b"\n"
    elif rc:
        assert (word or err) in p.stderr, p.stderr
    return p


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_model_equals_the_recorded_reference(name):
    want_rc, want_err = M.FIXTURES[name]
    out, rc, err = M.paf2tsv(M.golden(name))
    assert out == M.expected(name) and rc == want_rc and err == want_err


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_host_decode_equals_the_recorded_reference(cli, name):
    want_rc, want_err = M.FIXTURES[name]
    for opts in ((), ("--batch", 1), ("--batch", 256), ("--batch", 257)):
        p = host(cli, os.path.join(M.GOLDEN, name), *opts)
        assert p.returncode == want_rc, p.stderr[-300:]
        assert p.stdout == M.expected(name)
        if want_err is not None:
            assert p.stderr == want_err + b"\n"


def test_usage_and_arguments(cli, tmp_path):
    p = run(cli, "ss")
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(USAGE)
    assert b"--host-decode" in p.stderr and b"--batch INT" in p.stderr
    p = run(cli, "ss", "paf2tsv")
    assert p.returncode == 1 and p.stderr.startswith(USAGE)
    p = run(cli, "ss", "paf2tsv", "a.paf", "b.paf")
    assert p.returncode == 1 and p.stderr.startswith(USAGE)
    p = run(cli, "ss", "-h")
    assert p.returncode == 0 and p.stdout.startswith(USAGE) and b"--host-decode" in p.stdout and b"--batch INT" in p.stdout
    for v in ("--version", "-V"):
        p = run(cli, "ss", v)
        assert p.returncode == 0 and p.stdout == b"sigtk 0.2.0\n"
    p = run(cli, "ss", "tsv2paf", os.path.join(M.GOLDEN, "ss_dna.paf"))      # the reference: nothing, exit 0
    assert p.returncode == 0 and p.stdout == b""
    p = run(cli, "--help")
    assert p.returncode == 0 and b"         ss        ss string conversion\n" in p.stdout
    p = host(cli, tmp_path / "nope.paf")
    assert p.returncode == 1 and p.stdout == b"" and b"cannot open" in p.stderr


def test_ss_without_a_gpu_is_a_loud_error(cli):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    p = run(cli, "ss", "paf2tsv", os.path.join(M.GOLDEN, "ss_dna.paf"))
    assert p.returncode == 1 and b"no usable GPU" in p.stderr and p.stdout == b""
    import ctypes as C
    lib = api.load_library()
    b = api.SsBatch(None, 0, None, None, 0, 0)
    ws = (C.c_uint8 * 256)()
    w = C.addressof(ws) // 16 * 16 + 16
    assert lib.sgk_ss_decode(C.byref(b), None, None, None, None, None) == api.SGK_ERR_NODEVICE
    assert lib.sgk_ss_text_measure(C.byref(b), None, None, None, None, w, 128, None) == api.SGK_ERR_NODEVICE
    assert lib.sgk_ss_text_write(C.byref(b), None, None, None, None, 0, w, 128, None) == api.SGK_ERR_NODEVICE
    pipe = C.c_void_p()
    assert lib.sgk_ss_pipe_create(0, C.byref(pipe)) == api.SGK_ERR_NODEVICE and not pipe.value


def good_lines(seed=5, n=2):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ss, raw = M.random_ss(rs, 30 + i)
        out.append(M.paf_line(b"good%d" % i, ss, 100, 100 + raw, 7, 37 + i, 50))
    return out


@pytest.mark.parametrize("st_k", [2000, 2500, 10 ** 6])
def test_large_start_kmer_follows_the_algorithm(cli, tmp_path, st_k):
    """the reference's tables hold 2000 entries and grow late: it loses the first mapping or corrupts its heap here"""
    rs = np.random.RandomState(st_k)
    ss, raw = M.random_ss(rs, 600)
    dna = M.paf_line(b"r-dna", ss, 3, 3 + raw, st_k, st_k + 600, st_k + 700)
    rna = M.paf_line(b"r-rna", ss, 3, 3 + raw, st_k + 600, st_k, st_k + 700)
    p = check_against_model(cli, tmp_path, dna + rna)
    assert p.returncode == 0 and p.stdout.count(b"\n") == 1201 and b"\t.\t." in p.stdout


def test_long_deletion_run(cli, tmp_path):
    data = good_lines()[0] + M.paf_line(b"del", b"5,100000D5,", 0, 10, 0, 100002, 100002)
    p = check_against_model(cli, tmp_path, data, "--batch", 4096)
    assert p.returncode == 0 and p.stdout.endswith(b"del\t100000\t.\t.\ndel\t100001\t5\t10\n")


@pytest.mark.parametrize("ss, cols", [
    (b"12345678901,", (0, 0, 0, 1)),                      # a run of 11 digits
    (b"00000000001,", (0, 1, 0, 1)),                      # ... also when its value is small
    (b"2147483648,", (0, 0, 0, 1)),                       # INT32_MAX + 1
    (b"2147483647,1,", (0, 0, 0, 2)),                     # two tokens whose sum passes INT32_MAX
    (b"2147483647D1,", (0, 1, 0, 2)),                     # ... in the k-mer index
])
def test_numbers_out_of_range_are_an_error_of_their_own(cli, tmp_path, ss, cols):
    g = good_lines()
    data = g[0] + M.paf_line(b"big", ss, cols[0], cols[1], cols[2], cols[3], 10) + g[1]
    assert M.paf2tsv(data)[2] == M.MESSAGES[5]
    p = check_against_model(cli, tmp_path, data)
    assert p.returncode == 1 and p.stderr == b"Bad ss: Number out of range\n"


def test_ten_digits_up_to_int32_max_are_fine(cli, tmp_path):
    data = M.paf_line(b"max", b"2147483647I0000000000,", 0, 2147483647, 0, 1, 10)
    p = check_against_model(cli, tmp_path, data)
    assert p.returncode == 0 and p.stdout == M.HEADER + b"max\t0\t2147483647\t2147483647\n"


def test_the_lower_byte_error_wins_and_byte_errors_come_first(cli, tmp_path):
    for ss, st in ((b"5,,x", 1), (b"5x,,", 2), (b",", 1), (b"x", 2), (b"12345678901,,", 1), (b"99999999999,x", 2),
                   (b"5 ,", 2), (b"-5,", 2), (b"5,\x00", 2)):
        rec = M.Record(b"r", ss, 0, 0, 0, 0, 0)
        assert M.decode(rec)[0] == st, ss
        if b"\x00" in ss:
            continue     # (a NUL ends a PAF line: it cannot reach the decoder through a file)
        data = good_lines()[0] + M.paf_line(b"bad", ss, 0, 5, 0, 1, 10)
        p = check_against_model(cli, tmp_path, data)
        assert p.stderr == M.MESSAGES[st] + b"\n"
    # the signal check comes before the k-mer check
    p = check_against_model(cli, tmp_path, M.paf_line(b"both", b"5,", 0, 6, 0, 2, 10))
    assert p.stderr == M.MESSAGES[3] + b"\n"


def test_lines_the_reference_aborts_on_are_errors_with_a_line_number(cli, tmp_path):
    g = good_lines()
    ok = M.paf_line(b"r", b"5,", 0, 5, 0, 1, 10)
    cases = [
        (b"\t".join(ok.split(b"\t")[:11]) + b"\n", b"line 2: fewer than 12 fields"),          # 11 fields
        (b"\n", b"line 2: fewer than 12 fields"),                                             # an empty line
        (ok.replace(b"\t+\t", b"\t*\t"), b"line 2: the strand column"),
        (ok.replace(b"\t+\t", b"\t+-\t"), b"line 2: the strand column"),
        (M.paf_line(b"r", b"5,", -1, 4, 0, 1, 10), b"line 2: column 3 is negative"),
        (M.paf_line(b"r", b"5,", 0, 5, -2, 1, 10), b"line 2: column 8 is negative"),
        (M.paf_line(b"r", b"5,", 0, 5, 1, -1, 10), b"line 2: column 9 is negative"),
        (ok.replace(b"\t10\t0\t1\t", b"\t99999999999\t0\t1\t"), b"line 2: column 7 does not fit an int"),
        (b"\t".join(ok.split(b"\t")[:12]) + b"\ttp:A:P\n", b"ss:Z: tag not found in paf record for r"),
        (b"\t".join(ok.split(b"\t")[:12]) + b"\tSS:Z:5,\n", b"ss:Z: tag not found in paf record for r"),
    ]
    for line, word in cases:
        p = check_against_model(cli, tmp_path, g[0] + line + g[1], word=word)
        assert p.returncode == 1 and word in p.stderr and p.stdout == M.paf2tsv(g[0])[0], (line, p.stderr)
    # a bad string in front of a bad line: the string's message is the one printed
    p = check_against_model(cli, tmp_path, M.paf_line(b"r", b"5,,", 0, 5, 0, 1, 10) + b"\n")
    assert p.stderr == M.MESSAGES[1] + b"\n"


def test_field_rules(cli, tmp_path):
    """empty fields vanish, CR is a separator, atoi's reading of a column, the last ss:Z: field wins, a final line
    without a line end, a line of 300 000 bytes"""
    rs = np.random.RandomState(8)
    ss, raw = M.random_ss(rs, 60000)
    long_line = M.paf_line(b"long", ss, 0, raw, 0, 60000, 60000, tags_before=[b"xx:Z:" + b"A" * 100000])
    lines = [
        M.paf_line(b"a", b"5,", 0, 5, 0, 1, 10).replace(b"\t", b"\t\t\r\t"),
        M.paf_line(b"b", b"5,", 0, 5, 0, 1, 10).replace(b"\t0\t5\t", b"\t+0x\t 5.9\t"),
        M.paf_line(b"c", b"4,1,", 0, 5, 0, 2, 10, tags_before=[b"ss:Z:5,"], tags_after=[b"ss:Z", b"xss:Z:9,"]),
        long_line,
        M.paf_line(b"d", b"3I2,", 0, 5, 9, 8, 4, eol=b""),
    ]
    p = check_against_model(cli, tmp_path, b"".join(lines))
    assert p.returncode == 0 and p.stdout.endswith(b"d\t-5\t3\t5\n")
    check_against_model(cli, tmp_path, b"".join(lines), "--batch", 1000)


def test_live_reference_on_a_fresh_in_domain_paf(cli, tmp_path):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/sigtk_ref has not been built")
    rs = np.random.RandomState(int.from_bytes(os.urandom(4), "little"))
    lines = []
    for i in range(200):
        rows = int(rs.choice([0, 1, 2, 30, 255, 256, 257, 600, 1500]))
        ss, raw = M.random_ss(rs, rows)
        st_k, start_raw = int(rs.randint(0, 1999)), int(rs.randint(0, 10 ** 6))
        rna = bool(rs.randint(0, 2))
        a, b = (st_k + rows, st_k) if rna else (st_k, st_k + rows)
        lines.append(M.paf_line(b"read-%d" % i, ss, start_raw, start_raw + raw, a, b, st_k + rows + int(rs.randint(0, 50)),
                                eol=b"\r\n" if i % 17 == 0 else b"\n"))
    f = tmp_path / "fresh.paf"
    f.write_bytes(b"".join(lines))
    r = subprocess.run([REF, "ss", "paf2tsv", str(f)], capture_output=True, timeout=120)
    p = host(cli, f)
    assert r.returncode == 0 and p.returncode == 0 and p.stdout == r.stdout
    assert M.paf2tsv(f.read_bytes())[0] == r.stdout


def test_reader_and_decoder_under_asan_ubsan(tmp_path):
    """the PAF reader and ss_decode_host in the sanitizer build of the host sources (build.build_cli_asan): the fixtures
    and hostile files -- exit status 0 or 1 and no sanitizer report"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    try:   # skip only where the toolchain has no sanitizer runtime; a compile error in the host sources is a failure
        subprocess.run(["gcc", "-fsanitize=address,undefined", "-o", str(tmp_path / "probe"), str(probe)], check=True,
                       capture_output=True)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build not available: %s" % e)
    cli_asan = build.build_cli_asan()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def run_a(path, *opts):
        p = subprocess.run([cli_asan, "ss", "paf2tsv", "--host-decode", *[str(o) for o in opts], str(path)], capture_output=True,
                           timeout=120, env=env)
        assert p.returncode in (0, 1), (p.returncode, p.stderr[-600:])
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr[-600:]
        return p

    for name, (rc, _) in M.FIXTURES.items():
        for opts in ((), ("--batch", 7)):
            p = run_a(os.path.join(M.GOLDEN, name), *opts)
            assert p.returncode == rc and p.stdout == M.expected(name)
    ok = M.paf_line(b"r", b"5,", 0, 5, 0, 1, 10)
    hostile = {
        "megabyte": ok[:-1] + b"\tzz:Z:" + b"7" * (1 << 20) + b"\n",
        "tabs": b"\t" * 5000 + b"\n",
        "nul": ok[:20] + b"\0\0" + ok[20:] + b"\0" + ok,
        "nul_in_ss": M.paf_line(b"r", b"5,\x003,", 0, 5, 0, 1, 10),
        "digits": b"9" * 300000,
        "digits_in_ss": M.paf_line(b"r", b"9" * 300000, 0, 5, 0, 1, 10, eol=b""),
        "huge_claim": M.paf_line(b"r", b"5,", 0, 5, 0, 2147483647, 10),
        "empty": b"",
        "only_newlines": b"\n\n\n",
    }
    for name, data in hostile.items():
        f = tmp_path / (name + ".paf")
        f.write_bytes(data)
        p = run_a(f)
        out, rc, err = M.paf2tsv(data)
        assert p.returncode == rc and p.stdout == out, name
    rs = np.random.RandomState(4)
    alphabet = np.frombuffer(b"0123456789,,,IDD\t\t\t\n\r+-x:sZ\0", dtype=np.uint8)
    for i in range(40):
        data = ok + alphabet[rs.randint(0, alphabet.size, size=rs.randint(0, 300))].tobytes()
        f = tmp_path / "fuzz.paf"
        f.write_bytes(data)
        p = run_a(f)
        out, rc, err = M.paf2tsv(data)
        assert p.returncode == rc and p.stdout == out, data
