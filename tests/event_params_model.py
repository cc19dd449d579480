"""The yardstick of the event path with caller-supplied detector parameters: the reference's own steps, composed from the
oracle's generic pieces with free parameters -- oracle.pa -> oracle.prefix_sums -> oracle.tstat(w1), oracle.tstat(w2) ->
orc_peaks(t1, t2, n, w1, w2, thr1, thr2, peak_height) -> create_event (src/events.c:457-473) between consecutive peaks in
numpy float32, one rounding per operator.  For the two presets this composition is oracle.getevents
(test_event_params_cpu.py pins that before anything is compared with it).

The library's definitions where the reference is undefined: no peak gives one event [0, n), an empty read none, a window
with n < 2w an all-zero statistic (orc_tstat's)."""
import ctypes as C
from typing import NamedTuple

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(F).max)


class P(NamedTuple):
    w1: int
    w2: int
    thr1: float
    thr2: float
    ph: float


PRESETS = {0: P(3, 6, float(F(1.4)), 9.0, float(F(0.2))), 1: P(7, 14, float(F(2.5)), 9.0, float(F(1.0)))}

#: the parameter grid of the feature's tests: the presets first, then the off-preset sets
GRID_OFF = [
    P(2, 2, 0.5, 0.5, 0.0),                     # the smallest windows, everything emits
    P(5, 9, float(F(1.4)), 3.0, float(F(0.2))),  # odd windows, w2 != 2 w1
    P(8, 4, 2.0, 1.0, float(F(0.1))),           # w2 < w1
    P(3, 20, float(F(1.4)), 2.0, float(F(0.2))),  # a wide gap, long detector busy
    P(64, 64, 1.0, 1.0, 0.5),                   # the cap
    P(3, 6, FLT_MAX, 1.0, float(F(0.2))),       # the short detector never valid: the long one is unmasked throughout
    P(3, 6, 0.0, 9.0, float(F(0.2))),           # the short detector dominates from its first peak
]
GRID = [PRESETS[0], PRESETS[1]] + GRID_OFF


class Events(NamedTuple):
    start: np.ndarray   # uint32
    length: np.ndarray  # uint32
    mean: np.ndarray    # float32
    stdv: np.ndarray    # float32


def peaks(oracle, t1, t2, p: P) -> np.ndarray:
    """orc_peaks called directly with free parameters"""
    t1 = np.ascontiguousarray(t1, dtype=F)
    t2 = np.ascontiguousarray(t2, dtype=F)
    n = t1.size
    pk = np.empty(max(n, 1), dtype=np.int64)
    fp = C.POINTER(C.c_float)
    k = oracle.lib.orc_peaks(t1.ctypes.data_as(fp), t2.ctypes.data_as(fp), C.c_int64(n), C.c_int(p.w1), C.c_int(p.w2),
                             C.c_float(p.thr1), C.c_float(p.thr2), C.c_float(p.ph),
                             pk.ctypes.data_as(C.POINTER(C.c_int64)))
    return pk[:k].copy()


def peaks_of_pa(oracle, pa, p: P) -> np.ndarray:
    pa = np.ascontiguousarray(pa, dtype=F)
    s, q = oracle.prefix_sums(pa)
    return peaks(oracle, oracle.tstat(s, q, p.w1), oracle.tstat(s, q, p.w2), p)


def create_events(s, q, bounds) -> Events:
    """create_event for the events [bounds[k], bounds[k+1]): every operator rounds once, to float32"""
    b = np.asarray(bounds, dtype=np.int64)
    st, en = b[:-1], b[1:]
    length = (en - st).astype(F)
    with np.errstate(all="ignore"):
        mean = (s[en] - s[st]).astype(F) / length
        dsq = (q[en] - q[st]).astype(F)
        var = dsq / length - mean * mean
        stdv = np.sqrt(np.maximum(var, F(0.0)))
    return Events(st.astype(np.uint32), (en - st).astype(np.uint32), mean.astype(F), stdv.astype(F))


def events_pa(oracle, pa, p: P) -> Events:
    pa = np.ascontiguousarray(pa, dtype=F)
    n = pa.size
    if n == 0:
        z = np.zeros(0, dtype=np.uint32)
        return Events(z, z.copy(), np.zeros(0, dtype=F), np.zeros(0, dtype=F))
    s, q = oracle.prefix_sums(pa)
    pk = peaks(oracle, oracle.tstat(s, q, p.w1), oracle.tstat(s, q, p.w2), p)
    return create_events(s, q, [0] + pk.tolist() + [n])


def events_raw(oracle, raw, dig, off, rng, p: P) -> Events:
    return events_pa(oracle, oracle.pa(np.ascontiguousarray(raw, dtype=np.int16), dig, off, rng), p)


# ---------------------------------------------------------------- seeded reads

def random_read(rng: np.random.Generator, n: int) -> np.ndarray:
    """int16 read of n samples: steps, ramps, noise or a flat line (or a mix), in the range of a real signal"""
    if n == 0:
        return np.zeros(0, dtype=np.int16)
    kind = int(rng.integers(0, 5))
    x = np.full(n, float(rng.integers(300, 900)))
    if kind in (0, 4):      # steps: plateaus of random length and level
        i = 0
        while i < n:
            k = int(rng.integers(2, 40))
            x[i:i + k] = float(rng.integers(300, 900))
            i += k
    if kind == 1:           # ramps
        i = 0
        lvl = x[0]
        while i < n:
            k = int(rng.integers(3, 60))
            nxt = float(rng.integers(300, 900))
            m = min(k, n - i)
            x[i:i + m] = np.linspace(lvl, nxt, k)[:m]
            lvl = nxt
            i += k
    if kind in (2, 4):      # noise
        x = x + rng.normal(0.0, float(rng.choice([1.0, 5.0, 30.0])), n)
    # kind 3: the flat line
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def random_reads(seed: int, count: int, max_len: int):
    rng = np.random.default_rng(seed)
    return [random_read(rng, int(rng.integers(0, max_len + 1))) for _ in range(count)]
