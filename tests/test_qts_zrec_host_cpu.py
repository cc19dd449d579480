"""CPU: the host side of the record path `qts --gpu-inflate` shares with the other subtools -- heads parsed, rooms computed
(b5_zrec_room), a head-parsed view never used as a record -- in a stand-alone C program (tests/host/zrec_room_check.c)
built with -fsanitize=address,undefined where the toolchain has the sanitizers (else plainly) and run on the fixtures."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "sigtk_amd", "host")
SRC = os.path.join(ROOT, "tests", "host", "zrec_room_check.c")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("zrec_room") / "zrec_room_check")
    base = ["gcc", "-O1", "-g", "-std=c99", "-D_GNU_SOURCE", "-Wall", "-Werror", "-I", HOST]
    srcs = [SRC, os.path.join(HOST, "blow5.c"), os.path.join(HOST, "zstd_dec.c")]
    libs = ["-lz", "-lm"]
    san = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(base + san + ["-o", out] + srcs + libs, capture_output=True)
    if p.returncode != 0:   # (a toolchain without the sanitizer runtimes: the checks themselves still run)
        subprocess.run(base + ["-o", out] + srcs + libs, check=True)
    return out


def run(prog, path, slack):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    p = subprocess.run([prog, path, str(slack)], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-1500:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    m = re.match(rb"(\d+) records, (\d+) fit their room, (\d+) head bytes, (\d+) tail bytes\n", p.stdout)
    assert m, p.stdout
    return tuple(int(x) for x in m.groups())


def test_rooms_of_the_zlib_fixture(prog):
    n, fit, head, tail = run(prog, os.path.join(GOLDEN, "sp1_dna.blow5"), 256)
    assert (n, fit) == (100, 100)
    assert head == 100 * (2 + 36 + 36) and tail > 100 * 22      # uuid ids; five fixed columns (22 bytes) and a string
    # without slack the string column has no room: the records that carry a non-empty one do not fit
    n0, fit0, head0, tail0 = run(prog, os.path.join(GOLDEN, "sp1_dna.blow5"), 0)
    assert (n0, head0, tail0) == (n, head, tail) and fit0 < 100


def test_rooms_of_the_zstd_fixture_are_exact(prog):
    a = run(prog, os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5"), 256)
    b = run(prog, os.path.join(GOLDEN, "sp1_dna.blow5"), 256)
    assert a == b
