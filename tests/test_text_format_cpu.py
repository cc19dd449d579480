"""CPU: csrc/text_format.h -- the number formatting of the device-side TSV writer (csrc/text_kernels.hip) -- compiled
by the host compiler into `sigtk-amd _textcheck` and compared with glibc's snprintf, bytes and length-only form; the
CLI's usage names --gpu-text.  (The same header on the device: tests/test_gpu_text.py.)"""
import os
import subprocess

import pytest

from sigtk_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True)


@pytest.mark.parametrize("args", [("9973",), ("7919",), ("1", "0x58635f00", "0x58636100"), ("3", "0", "0x00ffffff"),
                                  ("1013", "0x58635faa", "0x7f800010"), ("1013", "0xd8635faa", "0xff800010")])
def test_text_format_matches_snprintf(cli, args):
    """"%f" on a strided sweep of all float bit patterns (two co-prime strides), densely around 1e15 where the multi-limb
    path takes over, over the denormals and the smallest normals, over the huge range up to FLT_MAX and past the
    infinities into the NaNs, both signs -- plus, in every run, the fixed cases: powers of two and their neighbours,
    ties (0x3c000000 -> 0.007812) and carries, 0x58635fa8 / a9 / aa, FLT_MAX (46 bytes), +-0, +-inf, +-nan, and "%ld" on
    0, +-1, powers of ten +- 1, INT64_MIN / MAX."""
    p = run(cli, "_textcheck", *args)
    assert p.returncode == 0 and p.stdout.strip().endswith(" 0 mismatches"), p.stdout
    n = int(p.stdout.split()[1])
    assert n > 100000          # the sweep ran: the fixed cases alone are ~250 000 values


def test_textcheck_counts_the_fixed_cases(cli):
    """an empty sweep still checks the fixed list (so a broken list cannot hide behind a passing sweep)"""
    p = run(cli, "_textcheck", "1", "5", "4")
    assert p.returncode == 0 and p.stdout.strip().endswith(" 0 mismatches"), p.stdout
    assert int(p.stdout.split()[1]) > 240000


@pytest.mark.parametrize("tool", ["pa", "event"])
def test_usage_names_gpu_text(cli, tool):
    p = run(cli, tool, "-h")
    assert p.returncode == 0 and "--gpu-text" in p.stdout
    p = run(cli, tool)
    assert p.returncode == 1 and "--gpu-text" in p.stderr


def test_header_is_plain_c_and_shared_with_the_kernels():
    """the kernels and the CLI compile the same file"""
    assert '#include "text_format.h"' in open(os.path.join(ROOT, "sigtk_amd", "csrc", "text_kernels.hip")).read()
    assert "text_format.h" in open(os.path.join(ROOT, "sigtk_amd", "host", "selftest.c")).read()
    assert "text_kernels.hip" in build.HIP_SOURCES
