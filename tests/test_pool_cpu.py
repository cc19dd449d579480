"""CPU: the host program's thread pool and blocking queue (sigtk_amd/host/pool.c) in a stand-alone C program
(tests/host/pool_check.c) built with -fsanitize=thread where the toolchain has the sanitizer (else plainly)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sigtk_amd", "host")
SRC = os.path.join(ROOT, "tests", "host", "pool_check.c")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """pool.c and its header cli.h alone: no GPU library, no BLOW5 reader"""
    out = str(tmp_path_factory.mktemp("pool") / "pool_check")
    base = ["gcc", "-O1", "-g", "-std=c99", "-D_GNU_SOURCE", "-Wall", "-Werror", "-I", HOST]
    srcs = [SRC, os.path.join(HOST, "pool.c")]
    p = subprocess.run(base + ["-fno-omit-frame-pointer", "-fsanitize=thread", "-o", out] + srcs + ["-lpthread"], capture_output=True)
    if p.returncode != 0:   # (a toolchain without the sanitizer runtime: the checks themselves still run)
        subprocess.run(base + ["-o", out] + srcs + ["-lpthread"], check=True)
    return out


def test_pool_and_queue_run_clean(prog):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=97")
    p = subprocess.run([prog], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr.decode(errors="replace")[-2000:])
    assert b"Sanitizer" not in p.stderr and b"WARNING" not in p.stderr, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout == b"pools of 1, 2 and 8 threads and the queue: 0 wrong\n"
