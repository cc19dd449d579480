"""CPU: the staging layout of the host text pipes (StageCursor of sigtk_amd/csrc/text_pipe.h) in a stand-alone program
(tests/host/stage_check.cpp) built with -fsanitize=address,undefined where the toolchain has the sanitizers (else
plainly).  The header is host code on the HIP runtime's declarations; the program calls none of them."""
import os
import subprocess

import pytest

from sigtk_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stage_check.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stage") / "stage_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include, "-I", build.CSRC]
    p = subprocess.run(base + ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", out, SRC], capture_output=True)
    if p.returncode != 0:   # (a toolchain without the sanitizer runtimes: the checks themselves still run)
        subprocess.run(base + ["-o", out, SRC], check=True)
    return out


def test_staging_offsets_equal_the_spelled_out_formulas(prog):
    p = subprocess.run([prog], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr.decode(errors="replace")[-2000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout == b"169000 layouts: 0 wrong\n"
