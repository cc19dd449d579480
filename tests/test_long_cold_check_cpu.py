"""CPU: tools/long_cold_check (built by __graft_entry__.build()) on 4 * 10^6 window pairs per long window: the lazy long
detector's bound, formed from the f32 sums of the window's two halves (sigtk_amd/csrc/tstat_math.h: sgk_lside_halves +
sgk_long_cold), never calls a pair cold whose reference statistic exceeds 9 -- same-sign, mixed-sign, constant and
stepped windows, and windows steered to a statistic of about 9.  (10^9 pairs per window: `tools/long_cold_check`, a few
minutes; profiles/event_leading_window.md has that run.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_cold_check_reduced():
    exe = os.path.join(ROOT, "tools", "long_cold_check")
    assert os.path.exists(exe), "tools/long_cold_check not built (run __graft_entry__.build())"
    p = subprocess.run([exe, "4000000"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = re.findall(r"^W2 = (\d+): (\d+) cases, (\d+) violations", p.stdout, flags=re.M)
    assert [int(w) for w, _, _ in rows] == [6, 14]
    for _, cases, bad in rows:
        assert int(cases) == 4000000 and int(bad) == 0
    # every kind of window was generated, and the steered kinds do land next to the threshold
    kinds = re.findall(r"kind (\d): +(\d+) cases, +(\d+) with the reference in \(8\.5, 9\.5\), (\d+) violations", p.stdout)
    assert len(kinds) == 16 and all(int(c) > 400000 and int(b) == 0 for _, c, _, b in kinds)
    assert all(int(near) > int(c) // 3 for k, c, near, _ in kinds if k in "1346")
