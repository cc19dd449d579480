"""GPU: the certified square root of create_event (sgk_sqrt_cert, sigtk_amd/csrc/tstat_math.h) with the hardware's
v_rsq_f32, against numpy.sqrt on float32 (correctly rounded), bit for bit.  tools/sqrt_cert_gpu (built by
__graft_entry__.build()) runs the same two steps as the event builder: the certified form, and sqrtf where the
certificate or the domain test fails."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
LO, HI = np.float32(2.0 ** -64), np.float32(2.0 ** 41)     # the stated domain: [2^-64, 2^41)


def _ulp_neighbours(x):
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))])


def inputs():
    rs = np.random.RandomState(17)
    parts = [
        # the edges of the domain and what lies just outside; zero, negative zero, a negative, the specials
        _ulp_neighbours([LO, HI]), np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1.1754944e-38, 3.4028235e38], dtype=np.float32),
        # powers of two +- 1 ulp over the whole exponent range
        _ulp_neighbours(np.float32(2.0) ** np.arange(-126, 128, dtype=np.float32)),
        # perfect squares +- 1 ulp: k^2 for every k below 4096 (exact in float), and squares of random 12-bit mantissas scaled
        _ulp_neighbours((np.arange(1, 4096, dtype=np.float64) ** 2).astype(np.float32)),
        _ulp_neighbours(((rs.randint(2048, 4096, size=50000).astype(np.float64) * 2.0 ** rs.randint(-40, 10, size=50000)) ** 2).astype(np.float32)),
    ]
    fixed = np.concatenate(parts)
    n_rand = N - fixed.size
    # seeded fill: half of it random bit patterns inside the domain, half variances as events have them (0.5 .. 400 pA^2)
    bits = rs.randint(int(LO.view(np.uint32)), int(HI.view(np.uint32)), size=n_rand // 2).astype(np.uint32)
    typical = rs.uniform(0.5, 400.0, size=n_rand - n_rand // 2).astype(np.float32)
    x = np.concatenate([fixed, bits.view(np.float32), typical]).astype(np.float32)
    assert x.size == N
    return x


def test_sqrt_cert_matches_numpy(gpu, tmp_path):
    exe = os.path.join(ROOT, "tools", "sqrt_cert_gpu")
    assert os.path.exists(exe), "tools/sqrt_cert_gpu not built (run __graft_entry__.build())"
    x = inputs()
    fin, fout = str(tmp_path / "in.f32"), str(tmp_path / "out.u32")
    x.tofile(fin)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = np.fromfile(fout, dtype=np.uint32).reshape(N, 3)
    cert, final, ok = out[:, 0], out[:, 1], out[:, 2] != 0
    with np.errstate(all="ignore"):
        want = np.sqrt(x).view(np.uint32)
    xb = x.view(np.uint32)
    in_dom = (xb >= LO.view(np.uint32)) & (xb < HI.view(np.uint32))
    nan = np.isnan(x)
    print("sqrt_cert: %d values, %d in the domain, %d certified (%.5f %% of the domain), %d take sqrtf" % (
        N, in_dom.sum(), ok.sum(), 100.0 * ok.sum() / in_dom.sum(), (~ok).sum()))
    # nothing outside the domain is certified.  Inside it the certificate fails when a rounding boundary lies within
    # 2^-40 (relative) of the root: 2 * 2^-40 of a spacing of at least 2^-24, i.e. at most 2^-15 of random inputs (four
    # times that is allowed here), and by construction at the two neighbours of every even power of two, whose roots are
    # 2^k (1 -+ 2^-25 - ...): half-way between two floats (2 * 53 such inputs lie in the domain)
    assert not (ok & ~in_dom).any()
    assert (in_dom & ~ok).sum() <= 2 * 53 + in_dom.sum() * 2.0 ** -13
    # certified results equal numpy's sqrt; uncertified ones took the fallback and equal it too (NaN: any NaN)
    bad = np.flatnonzero(ok & (cert != want))
    assert bad.size == 0, "certified but wrong: %r" % [(hex(int(xb[i])), hex(int(cert[i])), hex(int(want[i]))) for i in bad[:8]]
    same = (final == want) | (nan & np.isnan(final.view(np.float32))) | ((x < 0) & np.isnan(final.view(np.float32)))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, "final value wrong: %r" % [(hex(int(xb[i])), hex(int(final[i])), hex(int(want[i]))) for i in bad[:8]]
    assert (final[ok] == cert[ok]).all()
