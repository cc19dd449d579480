"""The definition of sgk_normalise_f32 / sgk_normalise (include/sigtk_gpu.h) in numpy float32.

meanf / stdvf / medianf come from Oracle.statf (oracle/sigtk_oracle.c), or from RefLib.statf -- the reference's own
functions -- where oracle/_ref has been built.  np.float32 subtraction, np.abs, multiplication and division are the
per-operation IEEE results: one rounding each, subnormals kept.

Comparisons are by bit pattern.  Where both sides hold a NaN they count as equal whatever its sign and payload (the rule
of tests/test_gpu_shims.py and tests/test_gpu_stat_f32.py): IEEE 754 leaves both open for 0 / 0 and inf - inf, and x86
gives the negative default NaN where the GPU gives the positive one."""
import numpy as np

F = np.float32
ZSCORE, MEDMAD = 1, 2
ZERO_SCALE, NONFINITE = 1, 2
MAD_TO_SIGMA = F(1.4826)
NAN = F("nan")


def statf_of(oracle, reflib=None):
    """the statistics' source: the reference where it is built, else the oracle"""
    return (reflib if reflib is not None else oracle).statf


def normalise(x, method, statf):
    """-> (y float32[n], (shift, scale, n, flags)) of one read"""
    assert method in (ZSCORE, MEDMAD)
    x = np.ascontiguousarray(x, dtype=F)
    n = x.size
    if n == 0:
        return np.zeros(0, F), (NAN, NAN, 0, 0)
    if not np.isfinite(x).all():
        return np.full(n, NAN, F), (NAN, NAN, n, NONFINITE)
    with np.errstate(all="ignore"):
        mean, std, med = (F(v) for v in statf(x))
        if method == ZSCORE:
            shift, scale = mean, std
        else:
            shift = med
            d = np.abs(x - shift)
            assert d.dtype == F
            scale = F(F(statf(d)[2]) * MAD_TO_SIGMA)
        y = (x - shift) / scale
    assert y.dtype == F
    return y, (shift, scale, n, ZERO_SCALE if scale == 0 else 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(got, want):
    """element-wise: the same bit pattern, or a NaN on both sides"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def is_subnormal(a):
    a = np.ascontiguousarray(a, dtype=F)
    return (a != 0) & (np.abs(a) < np.finfo(F).tiny)
