"""GPU parity of the builder's rounds (csrc/event_build.h: build_read; SGK_BUILD_CARRY: the records that do not fill a
round wait in LDS for the next tile's) on the hand-made reads of tests/event_rounds_cases.py, which put the carrying form
in each of its places: 0, 1 and 63 leftovers going into a tile, tiles of a multiple of 64 records, a tile without a
boundary while leftovers wait, reads that end without leftovers, of fewer than 64 events, of one tile, and tiles that are
too dense by themselves or only with the leftovers in front of them (these reads take the fallback).

Every batch runs whole (one wavefront per read), in segments of 1 024 and of 4 096 samples (two builder tiles: the first
segment walks the whole read's first two tiles), with 8 lanes per read, and through the fallback kernel (the same reads
with a sample that fails the exactness guard), with both presets and both input types, and is compared with the oracle bit
for bit: number of events, start, length, mean and stdv as bit patterns; the status counters say which reads were
flagged.  Per path the test requires, by the oracle's boundaries and the model, the places that path can reach.  No test
here times anything; the reads have 7 044 samples at the most."""
import pytest

import event_rounds_cases as R
from test_gpu_event_cases import options  # noqa: F401  (a fixture)
from test_gpu_event_masks import PATHS, _compare, _run
from test_gpu_event_masks import expected  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

PATHS_HERE = dict(PATHS, segments4096=dict(segment_len=R.SEGMENT, long_min=R.SEGMENT + 1))
SEGMENT_OF = {"segments1024": 1024, "segments4096": R.SEGMENT}


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("path", list(PATHS_HERE) + ["fallback"])
def test_rounds_reads(gpu, oracle, options, expected, path, rna, as_pa):  # noqa: F811
    names, reads = R.reads_of(rna)
    if path == "fallback":
        reads = R.flagged(reads)
        options(**PATHS["whole"])
    else:
        options(**PATHS_HERE[path])
    # the places this path can reach are reached, by the oracle's boundaries (a condition on the reads, not on the GPU)
    got_places = set()
    for x in reads:
        b = R.boundaries(oracle, x, rna)
        got_places |= R.places_first_segment(b, x.size) if path == "segments4096" else R.places(b, x.size)
    want = R.PLACES_OF_SEGMENTS[rna] if path == "segments4096" else R.PLACES_OF_PRESET[rna]
    assert not set(want) - got_places, sorted(set(want) - got_places)

    got, st = _run(gpu, oracle, reads, rna, as_pa)
    print("rounds %-12s rna %d %s: n_fallback_reads %d n_split_reads %d n_segments %d" % (
        path, rna, "pA" if as_pa else "int16", st.n_fallback_reads, st.n_split_reads, st.n_segments))
    _compare(expected, names, reads, rna, as_pa, got, path)
    assert st.n_capacity_overflow == 0
    lens = [x.size for x in reads]
    if path in SEGMENT_OF:
        assert st.n_split_reads == sum(1 for n in lens if n > SEGMENT_OF[path])
    else:
        assert st.n_split_reads == 0
        plan = gpu.event_plan(len(reads), sum(lens), max(lens), rna)
        assert plan.lanes_per_short_read == (8 if path == "packed8" else 0)
    if path == "fallback":
        assert st.n_fallback_reads == len(reads)
    elif path != "segments1024":
        # the flags: exactly the reads with a tile that is too dense.  k_event<3, *> ships the carrying form, where the
        # leftovers count; the other kernels ship whichever form measured better on their bench line (event_build.h) and
        # may build the read that is too dense only with its leftovers
        by_carry = sum(bool(R.schedule_carry(R.boundaries(oracle, x, rna), x.size)["dense"]) for x in reads)
        by_parent = sum(bool(R.schedule_parent(R.boundaries(oracle, x, rna), x.size)["dense"]) for x in reads)
        assert (by_carry, by_parent) == ((2, 1) if rna == 0 else (0, 0))
        assert st.n_fallback_reads in ((by_carry,) if path == "whole" else (by_carry, by_parent))
