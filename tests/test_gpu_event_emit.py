"""GPU parity of the emission bookkeeping of k_event<3, *>'s fast pass (csrc/event_detect.h, SGK_EVENT_EMIT: the bitmap word
built by shifting the emission mask in as a carry, one rare test per index) on the hand-made reads of
tests/event_emit_cases.py, which tests/test_event_emit_cases_cpu.py shows to reach every place of it: every residue of an
emitted peak in its 32-position span, in a chunk's first span and in later ones, chunks of odd and even multiples of 16,
reads that end 1, 15, 16, 17 and 31 positions into a span, emissions in the predicated steps and in a chunk's last block,
rare emissions either side of a flush, recorded hot runs that start in the current word, the previous one and further back.

Every batch runs whole (one wavefront per read: k_event<3, short> and k_event<3, float>), whole with a warm-up of 16
samples (speculation fails, chunks are run again from the true state and their words produced twice), and in segments
of 1 024 samples (k_event_seg, which keeps the form with a bit per index: it bounds a regression in the shared headers).
Events are compared with the oracle bit for bit; the counters of the status word must agree with the events, with the
model's hot runs and between the two input types.  DNA preset only: the RNA kernels keep the earlier form.  No timing;
the batch has 14 reads of 5 000 samples at the most."""
import pytest

import event_emit_cases as M
from test_gpu_event_cases import options  # noqa: F401  (a fixture)
from test_gpu_event_masks import _compare, _run
from test_gpu_event_masks import expected  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

PATHS = {"whole": dict(lanes_per_short_read=-1, tail_split=-1),
         "whole_warmup16": dict(lanes_per_short_read=-1, tail_split=-1, warmup=16),
         "segments1024": dict(segment_len=1024, long_min=1025)}


@pytest.fixture(scope="module")
def hot_runs():
    """per read of the catalogue: the model's certainly hot runs that a reset ends (a lane records and replays each)"""
    names, reads = M.reads()
    return [[r for r in M.analyse(x)[1] if r.sure_hot] for x in reads]


@pytest.mark.parametrize("path", list(PATHS))
def test_emit_reads(gpu, oracle, options, expected, hot_runs, path):  # noqa: F811
    names, reads = M.reads()
    options(**PATHS[path])
    counters = {}
    for as_pa in (False, True):
        got, st = _run(gpu, oracle, reads, 0, as_pa)
        print("emit %-14s %s: n_events_total %d n_long_replays %d n_replay_indices %d n_rerun_passes %d n_fallback_reads %d "
              "n_split_reads %d" % (path, "pA" if as_pa else "int16", st.n_events_total, st.n_long_replays, st.n_replay_indices,
                                    st.n_rerun_passes, st.n_fallback_reads, st.n_split_reads))
        _compare(expected, names, reads, 0, as_pa, got, path)
        assert st.n_events_total == sum(g.start.size for g in got) and st.n_capacity_overflow == 0
        # every read stays on the fast path (tests/test_event_emit_cases_cpu.py: no lane meets more than 8 hot runs)
        assert st.n_fallback_reads == 0
        assert st.n_split_reads == (sum(1 for x in reads if x.size >= 1025) if path == "segments1024" else 0)
        if path == "whole_warmup16":
            assert st.n_rerun_passes > 0
        if path != "segments1024":
            # a certainly hot run is recorded by the lane that holds its end and replayed over all of its indices
            lanes_with_a_run = 0
            for x, runs in zip(reads, hot_runs):
                _, own = M.lanes(x.size, 16 if path == "whole_warmup16" else M.LEAD)
                lanes_with_a_run += len({M._lane(own, min(r.b, x.size - 1)) for r in runs})
            assert st.n_long_replays >= lanes_with_a_run > 0
            assert st.n_replay_indices >= sum(r.b - r.a for runs in hot_runs for r in runs)
        assert st.n_long_replays > 0 and st.n_replay_indices > 0
        counters[as_pa] = (st.n_events_total, st.n_long_replays, st.n_replay_indices, st.n_rerun_passes)
    # the float kernel sees the pA values the int16 kernel forms: the same proofs fail, the same chunks are run again
    assert counters[False] == counters[True]
