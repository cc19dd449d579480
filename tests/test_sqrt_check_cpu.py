"""CPU: tools/sqrt_check (built by __graft_entry__.build()) on every 251st float bit pattern: no result that
sgk_sqrt_cert (sigtk_amd/csrc/tstat_math.h) certifies differs from sqrtf, with the hardware's reciprocal square root
modelled at its measured error and at twice that.  (All 2^32 patterns: `tools/sqrt_check`, about a minute.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sqrt_check_strided():
    exe = os.path.join(ROOT, "tools", "sqrt_check")
    assert os.path.exists(exe), "tools/sqrt_check not built (run __graft_entry__.build())"
    p = subprocess.run([exe, "251"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = re.findall(r"(\d+) certified \(([0-9.]+) %\), (\d+) certified outside the domain, (\d+) mismatches", p.stdout)
    assert len(rows) == 5
    for certified, share, outside, bad in rows:
        assert int(bad) == 0 and int(outside) == 0 and int(certified) > 0 and float(share) > 99.99
