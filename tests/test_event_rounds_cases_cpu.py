"""The hand-made reads of tests/event_rounds_cases.py reach every place of the carrying builder (csrc/event_build.h,
SGK_BUILD_CARRY), by the oracle's boundaries and the model of the round schedule.  No GPU; tests/test_gpu_event_rounds.py
runs the same reads on every path."""
import numpy as np

import event_rounds_cases as R


def _reached(oracle, rna, reads, first_segment=False):
    got = set()
    for x in reads:
        b = R.boundaries(oracle, x, rna)
        got |= R.places_first_segment(b, x.size) if first_segment else R.places(b, x.size)
    return got


def test_every_place_is_reached(oracle):
    for rna in (0, 1):
        names, reads = R.reads_of(rna)
        assert max(x.size for x in reads) <= 7100 and all(x.dtype == np.int16 for x in reads)
        for batch in (reads, R.flagged(reads)):
            missing = set(R.PLACES_OF_PRESET[rna]) - _reached(oracle, rna, batch)
            assert not missing, (rna, sorted(missing))
            missing = set(R.PLACES_OF_SEGMENTS[rna]) - _reached(oracle, rna, batch, first_segment=True)
            assert not missing, (rna, "first segments", sorted(missing))


def test_the_starting_point(oracle):
    """plateaus of 4 samples, 3 x 2 048 + 500 samples, DNA preset: 511, 512, 512 and 125 boundaries in the four tiles --
    63 leftovers go into the second tile, 575 records are in LDS there, one under BREC"""
    x = R.build(R.SPECS[0]["plateaus_of_4"], 0)
    b = R.boundaries(oracle, x, 0)
    assert x.size == 3 * R.TILE + 500 and R.per_tile(b, x.size) == [511, 512, 512, 125]
    s = R.schedule_carry(b, x.size)
    assert s["m_in"] == [0, 63, 63, 63] and not s["dense"] and s["partial"] == [3]
    assert s["rounds"] == 7 + 8 + 8 + 3 and R.schedule_parent(b, x.size)["rounds"] == 8 + 8 + 8 + 2


def test_the_dense_reads(oracle):
    """mixed 3- and 4-sample plateaus: a tile the parent form builds, too dense with the 63 leftovers in front of it"""
    x = R.build(R.SPECS[0]["dense_with_leftovers"], 0)
    b = R.boundaries(oracle, x, 0)
    assert max(R.per_tile(b, x.size)) <= R.BREC
    assert not R.schedule_parent(b, x.size)["dense"] and R.schedule_carry(b, x.size)["dense_by_leftovers"]
    x = R.build(R.SPECS[0]["dense"], 0)
    assert max(R.per_tile(R.boundaries(oracle, x, 0), x.size)) > R.BREC
