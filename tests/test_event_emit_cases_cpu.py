"""The hand-made reads of tests/event_emit_cases.py reach every place of the emission bookkeeping of k_event<3, *>'s fast pass
(csrc/event_detect.h, SGK_EVENT_EMIT), by the oracle's boundaries: the branch model that places them gives the oracle's
peaks on every read, and the committed search constants are what the searches find.  No GPU; tests/test_gpu_event_emit.py
runs the same reads."""
import numpy as np
import pytest

import event_cases as E
import event_emit_cases as M


@pytest.fixture(scope="module")
def catalogue():
    return M.reads()


def test_the_model_places_the_boundaries_of_the_oracle(oracle, catalogue):
    """the emissions the places are worked out from are the oracle's boundaries, read by read"""
    for name, x in zip(*catalogue):
        assert x.dtype == np.int16 and 600 <= x.size <= 5000, name
        peaks = E.analyse(x, 0)[0]
        want = oracle.event_raw(x, *E.SCALE, 0).start.tolist()
        assert want == [0] + [p for p, _ in peaks], name
        se, _ = M.analyse(x)
        assert sorted(p for p, _ in se) == sorted(p for p, k in peaks if k == 0), name


def test_every_place_is_reached(catalogue):
    names, reads = catalogue
    got = {}
    for name, x in zip(names, reads):
        for p in M.places_of(x):
            got.setdefault(p, []).append(name)
    missing = [p for p in M.PLACES if p not in got]
    assert not missing, missing
    # every residue of a span, in the first span a chunk touches and in a later one; the half-span and the span's ends
    for r in (15, 16, 31, 0):
        assert got[M.RESIDUE_FIRST[r]] and got[M.RESIDUE_LATER[r]]
    # the reads that were made for a place take it
    for m in M.END_M:
        assert "end_m%d" % m in got[M.END_M[m]]
    assert "rare_last_bit" in got[M.RARE_LAST_BIT] and "rare_first_bit" in got[M.RARE_FIRST_BIT]
    assert "run_same_word" in got[M.RUN_SAME_WORD] and "run_previous_word" in got[M.RUN_PREVIOUS_WORD]
    assert "run_older" in got[M.RUN_OLDER]
    assert "stairs_7_5000" in got[M.K_ODD] and "stairs_7_1500" in got[M.K_EVEN]


def test_the_geometry_restated():
    """chunks of 80 on 63 lanes at 5 000 samples, of 32 at 1 500 (event_cases.lanes_whole); a pass starts `lead` in front"""
    for n in (700, 1500, 2100, 5000):
        K, own = M.lanes(n)
        lead, want = E.lanes_whole(n, 0)
        assert lead == M.LEAD and [(s, e) for _, s, e in own] == want
        assert all(ib % 16 == 0 and ib == (s - lead if c else 0) for c, (ib, s, e) in enumerate(own))
    assert M.lanes(5000)[0] == 80 and M.lanes(1500)[0] == 32 and M.lanes(2100)[0] == 48 and M.lanes(700)[0] == 16


def test_no_lane_meets_more_hot_runs_than_it_records(catalogue):
    """the reads stay on the fast path: at most LZ_NREC certainly hot runs end in a lane's chunk"""
    for name, x in zip(*catalogue):
        _, own = M.lanes(x.size)
        ends = [M._lane(own, min(r.b, x.size - 1)) for r in M.analyse(x)[1] if r.sure_hot]
        assert max([ends.count(c) for c in set(ends)], default=0) <= E.LZ_NREC, name


def test_no_tile_is_too_dense_for_the_builder(oracle, catalogue):
    """... nor does the builder send one to the fallback: no tile of 2 048 samples holds more boundary records than fit"""
    import event_rounds_cases as R
    for name, x in zip(*catalogue):
        assert not R.schedule_carry(R.boundaries(oracle, x, 0), x.size)["dense"], name


def test_search_constants_are_what_the_searches_find():
    assert {m: M.search_end(m) for m in M.END_M} == M.END_FOUND
    assert {t: M.search_rare(t) for t in M.RARE_FOUND} == M.RARE_FOUND
    assert {t: M.search_run(t) for t in M.RUN_FOUND} == M.RUN_FOUND
