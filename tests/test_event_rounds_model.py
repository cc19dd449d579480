"""The builder's round schedule (csrc/event_build.h: build_read), parent form against the carrying form (SGK_BUILD_CARRY),
on the model of tests/event_rounds_cases.py: both forms emit the same (rank, previous boundary, boundary) triples in the
same order, every rank once; the carrying form keeps a leftover for one tile at the most (the model asserts what its
16-bit position can express) and never runs more rounds than the parent form.  No GPU."""
import itertools

import numpy as np

import event_rounds_cases as R

COUNTS = (0, 1, 63, 64, 65, 127, 128, 511, 512)


def _same(bounds, hi, **kw):
    a, b = R.schedule_parent(bounds, hi, **kw), R.schedule_carry(bounds, hi, **kw)
    if a["dense"] or b["dense"]:
        # the leftovers count: a read the parent form builds may be too dense for the carrying form, never the reverse
        assert b["dense"] and (a["dense"] or b["dense_by_leftovers"])
        return a, b
    assert a["events"] == b["events"]
    rank0, skip = kw.get("rank0", 0), kw.get("skip_first", False)
    ranks = [e[0] for e in a["events"]]
    first = rank0 + (1 if skip and len(bounds) else 0)
    assert ranks == list(range(first, rank0 + len(bounds)))
    assert (a["rank"], a["prev"]) == (b["rank"], b["prev"])          # what the read's closing event takes
    assert a["lanes"] == b["lanes"] == len(bounds) and b["rounds"] <= a["rounds"]
    # previous boundary of every event: the boundary in front of it in the read
    if not skip:
        assert b["events"] == list(zip(range(rank0, rank0 + len(bounds)), [0] + list(bounds[:-1]), bounds))
    return a, b


def test_every_sequence_of_edge_counts():
    saved = 0
    for ntiles in (1, 2, 3, 4):
        for counts in itertools.product(COUNTS, repeat=ntiles):
            a, b = _same(R.spread(counts), ntiles * R.TILE)
            assert not b["dense"]
            # a partial round only at the end, or where fewer than 64 records hold leftovers already
            for t in b["partial"]:
                assert t == ntiles - 1 or (b["m_in"][t] > 0 and b["m_in"][t] + counts[t] < R.LANES)
            assert b["rounds"] == sum((b["m_in"][t] + counts[t]) // R.LANES for t in range(ntiles)) + len(b["partial"])
            saved += a["rounds"] - b["rounds"]
    assert saved > 0


def test_random_sequences():
    rs = np.random.RandomState(2024)
    dense = 0
    for _ in range(2000):
        ntiles = int(rs.randint(1, 7))
        bounds = []
        for t in range(ntiles):
            kind = rs.randint(4)
            c = int(rs.randint(0, 3)) if kind == 0 else int(rs.randint(0, 130)) if kind == 1 else int(rs.randint(300, 600))
            bounds += sorted(t * R.TILE + rs.choice(R.TILE, size=c, replace=False))
        cut = int(rs.randint(1, R.TILE + 1))                     # the last tile is cut short
        hi = (ntiles - 1) * R.TILE + cut
        bounds = [int(b) for b in bounds if b < hi]
        a, b = _same(bounds, hi)
        dense += b["dense"]
    assert 0 < dense < 1000


def test_segment_starts():
    """a segment's walk: it starts at the 32-sample word of the last boundary in front of the segment, whose record ends no
    event of this segment (skip_rank) and lends the first one its start"""
    rs = np.random.RandomState(7)
    for k in range(600):
        seg_a = int(rs.randint(1, 40)) * 1024
        seg_len = int(rs.choice([1024, 2048, 3072, 4096, 8192]))
        front = seg_a - int(rs.randint(1, (3000, 40, 5)[k % 3]))
        if front < 0:
            continue
        walk0 = front & ~31
        c = int(rs.randint(0, (seg_len // 4, 70, 3)[k % 3] + 1))
        own = sorted(int(x) for x in seg_a + rs.choice(seg_len, size=c, replace=False))
        bounds = [front] + own
        rank0 = int(rs.randint(0, 100000))
        a, b = _same(bounds, seg_a + seg_len, walk0=walk0, rank0=rank0, skip_first=True)
        if not b["dense"]:
            assert [e[2] for e in b["events"]] == own and (not own or b["events"][0][1] == front)


def test_average_rounds_of_a_dna_read():
    """396.5 boundaries per tile (config 2 of bench.py: 1.936e8 events in 1e9 samples), here spread at random: the parent
    form rounds every tile's count up, the carrying form the read's"""
    rs = np.random.RandomState(1)
    n = 100000
    bounds = sorted(int(x) for x in rs.choice(n, size=19358, replace=False))
    a, b = _same(bounds, n)
    per_tile = R.per_tile(np.array(bounds), n)
    assert a["rounds"] == sum(-(-c // R.LANES) for c in per_tile) and b["rounds"] == len(bounds) // R.LANES + 1
    assert a["rounds"] - b["rounds"] > 0.4 * len(per_tile)
