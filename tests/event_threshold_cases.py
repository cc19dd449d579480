"""Parameter sets and reads for the presets' kernels with run-time thresholds (SGK_EVENT_PARAMS_PRESET_KERNELS): windows
3/6 and 7/14 with the caller's threshold1, threshold2 >= 9 and peak_height.  The yardstick is tests/event_params_model.py.

What the reads are for: a kernel that ignored one of its three run-time numbers and used the preset's must fail somewhere.
tests/test_event_thresholds_cpu.py checks, with the model alone, that the reads can tell: every set changes the events of
at least three reads against its preset, and threshold2 decides on reads made for it."""
from typing import NamedTuple

import numpy as np

import event_cases as E
import event_params_model as M

F = np.float32
P = M.P
FLT_MAX = M.FLT_MAX
T14 = float(F(1.4))
T14_UP = float(np.nextafter(F(1.4), F(2.0)))       # one ulp above the DNA preset's threshold1
T9_DOWN = float(np.nextafter(F(9.0), F(0.0)))      # one ulp below 9: outside the fast domain

#: sets the flag sends to the presets' kernels, DNA windows
FAST_DNA = [
    P(3, 6, 1.0, 9.0, float(F(0.1))),
    P(3, 6, T14_UP, 9.0, float(F(0.2))),
    P(3, 6, 0.0, 9.0, 0.0),                 # an event every few samples: the builder's 512-per-2 048 fallback
    P(3, 6, T14, 9.0, 0.0),
    P(3, 6, FLT_MAX, 9.0, float(F(0.2))),   # the short detector never valid, the long one never reset
    P(3, 6, FLT_MAX, 12.0, float(F(0.2))),
    P(3, 6, T14, FLT_MAX, float(F(0.2))),
    P(3, 6, 2.0, 20.0, 0.5),
    P(3, 6, FLT_MAX, 20.0, float(F(0.2))),  # (beyond the issue's list: threshold2 = 20 inside a replay of the whole read)
]
#: ... RNA windows
FAST_RNA = [
    P(7, 14, 1.5, 12.0, 0.5),
    P(7, 14, float(F(2.5)), 9.0, 0.0),
    P(7, 14, FLT_MAX, 9.0, 1.0),
    P(7, 14, float(F(2.5)), FLT_MAX, 1.0),
    P(7, 14, FLT_MAX, 12.0, 1.0),           # (beyond the issue's list, as above)
    P(7, 14, FLT_MAX, 20.0, 1.0),
]
FAST = FAST_DNA + FAST_RNA
#: sets that take the generic kernel even with the flag
GENERIC_WITH_FLAG = [
    P(3, 6, T14, T9_DOWN, float(F(0.2))),
    P(3, 6, T14, 3.0, float(F(0.2))),
    P(3, 7, T14, 9.0, float(F(0.2))),
    P(6, 12, T14, 9.0, float(F(0.2))),
    P(7, 14, float(F(2.5)), 1.0, 1.0),
]
#: two tuned sets per window pair for the launch forms
FORM_SETS = {0: [FAST_DNA[0], FAST_DNA[5]], 1: [FAST_RNA[0], FAST_RNA[4]]}


def ident(p):
    return "%d-%d-%s-%s-%s" % (p.w1, p.w2, *("max" if v == FLT_MAX else "%.9g" % v for v in p[2:]))


def rna_of(p):
    return 1 if p.w1 == 7 else 0


def preset_of(p):
    return M.PRESETS[rna_of(p)]


class Read(NamedTuple):
    name: str
    raw: np.ndarray      # int16
    scale: tuple         # (digitisation, offset, range)


def _r(name, raw, scale=E.SCALE):
    return Read(name, np.ascontiguousarray(raw, dtype=np.int16), tuple(float(v) for v in scale))


# ---------------------------------------------------------------- reads on which threshold2 decides
# Noisy steps with step / noise ratios spread so that the long window's statistic peaks anywhere between about 5 and 40:
# with threshold1 = FLT_MAX the short detector never resets the long one, and which of its peaks become boundaries is
# threshold2's decision alone.  (On the catalogue every long-detector peak is far above 2 000: any threshold2 below
# FLT_MAX gives the events of 9.)

def thr2_read(seed, n=700):
    rng = np.random.default_rng(seed)
    x = np.empty(n)
    lvl, i = 500.0, 0
    while i < n:
        k = int(rng.integers(25, 60))
        x[i:i + k] = lvl
        i += k
        lvl += float(rng.choice([-1.0, 1.0])) * float(rng.uniform(16.0, 130.0))
        lvl = min(max(lvl, 100.0), 1500.0)
    x += rng.normal(0.0, 8.0, n)
    return np.rint(x).astype(np.int16)


def thr2_reads():
    return [_r("thr2_steps_seed%d" % s, thr2_read(s)) for s in range(9100, 9106)]


# ---------------------------------------------------------------- reads on which one ulp of threshold1 decides
# A short-window statistic of exactly nextafter(1.4f) at a peak: the preset's `peak_value > 1.4f` holds, the tuned set's
# `peak_value > nextafter(1.4f)` does not, and the boundary is the preset's alone.  Windows {0, 15, 30} and {14, 29, 44}
# (times a factor) have the statistic 1.4 in real arithmetic; which float the reference's expression rounds to depends on
# the read's scale, and the scales below are the ones at which it is the float above 1.4f (found by search with the model,
# pinned by tests/test_event_thresholds_cpu.py).

ULP_READS = [   # (name, samples, (digitisation, offset, range))
    ("ulp_a", [266, 298, 316, 282, 328, 274, 297, 334, 330, 304, 337, 265, 346, 301, 256, 388, 343, 298, 332, 352, 334, 362,
               371, 329, 335, 378, 320, 311, 341, 315, 346, 351, 315, 340, 326, 333], (8192.0, 12.0, 1485.7822298710807)),
    ("ulp_b", [649, 677, 671, 664, 686, 638, 631, 634, 648, 644, 632, 697, 652, 607, 739, 649, 694, 702, 717, 707, 669, 671,
               663, 686, 672, 695, 665, 698, 694, 715], (8192.0, 34.0, 1308.0970801335238)),
    ("ulp_c", [580, 575, 579, 560, 578, 578, 561, 564, 586, 585, 544, 584, 573, 569, 575, 560, 564, 594, 534, 622, 562, 592,
               581, 609, 595, 609, 574, 585, 613, 579, 587, 575, 577, 586, 583], (8192.0, -3.0, 1495.384524058745)),
    ("ulp_d", [251, 265, 266, 243, 285, 223, 260, 237, 269, 260, 276, 281, 257, 245, 273, 227, 239, 256, 301, 211, 343, 253,
               298, 298, 264, 267, 277, 290, 317, 290, 270, 287, 311, 314, 283, 317, 321, 322, 275],
     (8192.0, -13.0, 1434.1758223139154)),
    ("ulp_e", [423, 408, 423, 443, 404, 419, 425, 387, 415, 439, 420, 460, 415, 370, 502, 457, 412, 484, 443, 426, 427, 475,
               441, 486, 422, 466, 460, 440, 427], (8192.0, 34.0, 1410.9844439794517)),
]


def ulp_reads():
    return [_r(name, np.array(raw), scale) for name, raw, scale in ULP_READS]


# ---------------------------------------------------------------- everything

def edge_lengths():
    out = [0, 1]
    for w in (3, 6, 7, 14):
        out += [2 * w - 1, 2 * w, 2 * w + 1]
    return out + [63, 64, 65, 4095, 4096, 4097]


def edge_reads():
    rng = np.random.default_rng(515)
    return [_r("edge_n%d" % n, M.random_read(rng, n)) for n in edge_lengths()]


def guard_read():
    """np.full(300, 1 - offset), as tests/test_gpu_event_params.py::test_presets_without_the_flag_take_sgk_event_opt builds
    it.  (Every pA value is range / digitisation = 0.17: the read is flat, but it PASSES the exactness guard -- the
    fallback reads that test counts are other catalogue reads.  guard_fail_read is the one that fails it.)"""
    return _r("flat_at_1-offset", np.full(300, 1 - int(E.SCALE[1]), dtype=np.int16))


def guard_fail_read():
    """noisy steps around 85 pA with ten samples of 0.00017 pA (raw = -10 under an offset of 10.001): magnitudes 2^19
    apart, where the exactness guard tolerates 2^16 -- on raw input and, with the same values, on pA input.  The read
    goes to k_event_fallback."""
    x = thr2_read(9150, 400)
    x[50:60] = -10
    return _r("fails_the_exactness_guard", x, (E.SCALE[0], 10.001, E.SCALE[2]))


def catalogue_reads(max_len=None):
    return [_r("cat_" + k.name, k.raw) for k in E.catalogue() if max_len is None or k.raw.size <= max_len]


def random_reads():
    return [_r("random_%d" % k, x) for k, x in enumerate(M.random_reads(2025, 24, 3000))]


_ALL = None


def reads():
    """the inputs of every fast-domain set: catalogue, random reads, edge lengths, the flat read and the guard-failing read, the reads made
    for threshold2 and for one ulp of threshold1 (built once)"""
    global _ALL
    if _ALL is None:
        _ALL = catalogue_reads() + random_reads() + edge_reads() + [guard_read(), guard_fail_read()] + thr2_reads() + ulp_reads()
    return _ALL


def differ(a, b):
    return a.start.size != b.start.size or not np.array_equal(a.start, b.start)
