"""GPU parity of the detector's certificate masks and of the builder's tile walk, on the three paths that share
csrc/event_detect.h: one wavefront per read, segments of 1 024 samples, 8 lanes per read.

The detector decides per index whether its fast t-statistic is certified (variance above its floor AND the tail's
rounding certificate) and whether the long window is provably cold; both decisions are lane masks combined on the scalar
unit.  The reads here are chosen for those masks: lengths at the window and tile edges, a constant stretch (variance at
its floor: never certified), periodic stretches (delta == 0 at every index), and one 100 000-sample read per preset that
meets uncertified tails at their natural rate.  Both input types (int16 through device.event, float pA through
sgk_event_pa_opt) are compared with the oracle field by field, bit for bit; there are no tolerances."""
import numpy as np
import pytest

import event_cases as E
from test_gpu_event_cases import _event_pa, options  # noqa: F401  (options: a fixture)

pytestmark = pytest.mark.gpu

#: 2 * W1, 2 * W2 of both presets, one builder tile (lane: 32 samples, wave: 2 048), a segment, +- 1
LENGTHS = [0, 1, 5, 6, 11, 12, 13, 27, 28, 29, 199, 200, 1023, 1024, 1025, 2047, 2049, 4097]
PATHS = {"whole": dict(lanes_per_short_read=-1, tail_split=-1),
         "segments1024": dict(segment_len=1024, long_min=1025),
         "packed8": dict(lanes_per_short_read=8, tail_split=-1, short_max=131072)}
TILE = 2048
TILE_POSITIONS = (0, 1, 31, 32, 33, 2047)


def noisy(rs, n, level, amp=8):
    return level + rs.randint(-amp, amp + 1, size=n)


def const_stretch_read():
    """noise, 64 equal samples (every window inside has variance 0: cv at its floor), noise"""
    rs = np.random.RandomState(5)
    return np.concatenate([noisy(rs, 1000, 600), np.full(64, 640), noisy(rs, 1000, 700)]).astype(np.int16)


def periodic_read(period):
    """noise around stretches of a pattern of the given period: windows of W1 = period (and W2 = 2 * period) samples have
    equal sums at every index inside, so delta == 0 with a variance far above the floor"""
    rs = np.random.RandomState(period)
    pat = np.array([500, 520, 545, 510, 560, 530, 575][:period])
    parts = []
    for k in range(4):
        parts += [noisy(rs, 150 + 37 * k, 600 + 40 * k), np.tile(pat + 10 * k, 40 + k)]
    return np.concatenate(parts + [noisy(rs, 200, 650)]).astype(np.int16)


def step_read(n, p):
    """n samples of noise of +-8 around a level that steps up by 200 raw units at sample p"""
    rs = np.random.RandomState(n + p)
    x = noisy(rs, n, 500)
    x[p:] += 200
    return x.astype(np.int16)


def tile_reads():
    """-> [(n, p, read)]: a step at position 0, 1, 31, 32, 33, 2047 of every builder tile of reads of 2 048 and 4 096 samples"""
    out = []
    for n in (2048, 4096):
        for tb in range(0, n, TILE):
            for q in TILE_POSITIONS:
                p = tb + q
                if 16 <= p <= n - 16:     # a step needs both windows of either preset inside the read
                    out.append((n, p, step_read(n, p)))
    return out


def dense_read(n=2048):
    """a level change every 3 samples (with noise of +-2): more boundary records than a builder tile holds"""
    rs = np.random.RandomState(3)
    return (np.repeat(np.tile([420, 610], n // 6 + 1), 3)[:n] + rs.randint(-2, 3, size=n)).astype(np.int16)


def _scal(n):
    return tuple(np.full(n, v) for v in E.SCALE)


@pytest.fixture(scope="module")
def edge_reads(gpu):
    reads, _, _, _ = gpu.synth_reads_host(len(LENGTHS), LENGTHS, seed=23, kind=0)
    reads = [r.astype(np.int16) for r in reads] + [const_stretch_read(), periodic_read(3), periodic_read(7)]
    names = ["len_%d" % n for n in LENGTHS] + ["const_64", "period_3", "period_7"]
    return names, reads


@pytest.fixture(scope="module")
def long_reads(gpu):
    """one 100 000-sample synthetic read per preset (the generator's DNA-like and RNA-like kinds)"""
    return {rna: gpu.synth_reads_host(1, 100000, seed=31 + rna, kind=rna)[0][0] for rna in (0, 1)}


@pytest.fixture(scope="module")
def expected(oracle):
    """the oracle's events, once per (read, preset, input type) for the whole module"""
    memo = {}

    def f(raw, rna, as_pa):
        key = (raw.tobytes(), rna, as_pa)
        if key not in memo:
            memo[key] = oracle.getevents(oracle.pa(raw, *E.SCALE), rna) if as_pa else oracle.event_raw(raw, *E.SCALE, rna)
        return memo[key]
    return f


def _run(gpu, oracle, reads, rna, as_pa):
    """-> (list of Events, status) of the batch through device.event (int16) or sgk_event_pa_opt (float pA), under the options
    that are set"""
    if as_pa:
        return _event_pa(gpu, [oracle.pa(r, *E.SCALE) for r in reads], rna)
    import torch
    from sigtk_amd import device
    b = device.upload_reads(reads, *_scal(len(reads)), torch.device("cuda", 0))
    arena = device.EventArena(b)
    device.event(b, arena, rna)
    torch.cuda.synchronize()
    return [arena.read_events(r) for r in range(len(reads))], arena.status()


def _compare(expected, names, reads, rna, as_pa, got, what):
    failures = []
    for name, raw, g in zip(names, reads, got):
        exp = expected(raw, rna, as_pa)
        for field, a, b in (("count", np.array([g.start.size]), np.array([exp.start.size])),
                            ("start", g.start.astype(np.uint64), exp.start), ("length", g.length.astype(np.float32), exp.length),
                            ("mean", g.mean.view(np.uint32), exp.mean.view(np.uint32)),
                            ("stdv", g.stdv.view(np.uint32), exp.stdv.view(np.uint32))):
            if a.shape != b.shape or not np.array_equal(a, b):
                failures.append("%s rna %d %s %s (n=%d): %s differs" % (what, rna, "pA" if as_pa else "int16", name, raw.size, field))
                break
    assert not failures, "\n".join(failures)


def _path_taken(gpu, path, reads, rna, st):
    """the status counters / the plan say that the batch ran on the path under test"""
    lens = [r.size for r in reads]
    if path == "segments1024":
        assert st.n_split_reads == sum(1 for n in lens if n >= 1025)
    else:
        assert st.n_split_reads == 0
        plan = gpu.event_plan(len(reads), sum(lens), max(lens), rna)
        assert plan.lanes_per_short_read == (8 if path == "packed8" else 0)


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("path", list(PATHS))
def test_edge_reads(gpu, oracle, options, expected, edge_reads, path, rna, as_pa):
    names, reads = edge_reads
    options(**PATHS[path])
    got, st = _run(gpu, oracle, reads, rna, as_pa)
    print("masks edge reads %-12s rna %d %s: n_fallback_reads %d n_split_reads %d n_rerun_passes %d" % (
        path, rna, "pA" if as_pa else "int16", st.n_fallback_reads, st.n_split_reads, st.n_rerun_passes))
    _compare(expected, names, reads, rna, as_pa, got, path)
    _path_taken(gpu, path, reads, rna, st)
    assert st.n_capacity_overflow == 0 and got[0].start.size == 0


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("path", list(PATHS))
def test_long_read_uncertified_tails(gpu, oracle, options, expected, long_reads, path, rna, as_pa):
    """100 000 indices: at 2^-14 a handful of tails miss their certificate and are redone with the reference expression;
    the read stays on the fast path"""
    reads = [long_reads[rna]]
    options(**PATHS[path])
    got, st = _run(gpu, oracle, reads, rna, as_pa)
    print("masks long read %-12s rna %d %s: n_fallback_reads %d n_split_reads %d n_segments %d n_rerun_passes %d" % (
        path, rna, "pA" if as_pa else "int16", st.n_fallback_reads, st.n_split_reads, st.n_segments, st.n_rerun_passes))
    _compare(expected, ["synth_100000"], reads, rna, as_pa, got, path)
    _path_taken(gpu, path, reads, rna, st)
    assert st.n_fallback_reads == 0 and st.n_capacity_overflow == 0


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
def test_tile_boundaries(gpu, oracle, options, expected, rna, as_pa):
    """whole reads: a boundary on the first, second, 32nd .. 34th and last sample of a builder tile (the lane's first and
    last bit, the neighbour lane's first), and a tile with more boundaries than it has records"""
    tiles = tile_reads()
    reads = [x for _, _, x in tiles] + [dense_read()]
    names = ["step_%d_at_%d" % (n, p) for n, p, _ in tiles] + ["dense_2048"]
    options(**PATHS["whole"])
    got, st = _run(gpu, oracle, reads, rna, as_pa)
    print("masks tile boundaries rna %d %s: n_fallback_reads %d" % (rna, "pA" if as_pa else "int16", st.n_fallback_reads))
    _compare(expected, names, reads, rna, as_pa, got, "whole")
    for (n, p, x), g in zip(tiles, got):
        assert p in set(g.start.tolist()), "no boundary at the step of step_%d_at_%d" % (n, p)
    assert st.n_split_reads == 0 and st.n_capacity_overflow == 0
    if rna == 0:
        # 683 boundaries in 2 048 samples: more than BREC = 576 records, the read is redone by the fallback kernel
        assert got[-1].start.size > 576 and st.n_fallback_reads >= 1
