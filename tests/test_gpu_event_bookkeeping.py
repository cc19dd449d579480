"""GPU parity of the detector's per-index bookkeeping (csrc/event_detect.h: LazyPass::dstep_core): the emitted peak's bit in
the lane's bitmap word, and the lazy long detector's mask and run start, which the kernels that take the mask-history
form (LazyPass::BOOK) keep as scalar lane masks and one register.

Hand-made reads of at most a few thousand samples, placed by the branch model of tests/event_cases.py (`places` below
says which place a read reaches, and test_the_reads_reach_their_places requires every one with either preset):

  * a usual emission (the peak lies w1/2 + 1 indices back) on every block-relative index 0 .. 15, with its bit on bit 31
    of the bitmap word and on bit 0 of the next, on a lane's chunk start and on its last index;
  * a rare emission (the peak is older: a rise that rolls off slowly keeps the statistic below the peak's by less than
    peak_height) alone in its 16-index block, directly behind a usual one in the same block, directly in front of one;
  * a hot run of the long detector that starts behind the mask of a usual emission (peak_pos + w1 + 1) and one that
    starts at the index of a rare emission (whose mask has run out), each recorded at the next reset;
  * reads that end 1, w1/2 + 1 and 15 indices into a block;
  * reads of different lengths in one packed wave: lanes that are done while their neighbours still step.

Every batch runs on the three paths that share event_detect.h and on the fallback kernel (each read with a tiny-|pA|
sample and a large one: it fails the exactness guard), with both presets and both input types, and is compared with the oracle bit for
bit (start, length, mean and stdv as bit patterns).  No test here times anything."""
import numpy as np
import pytest

import event_cases as E
from test_gpu_event import _check_events
from test_gpu_event_cases import options  # noqa: F401  (a fixture)
from test_gpu_event_masks import PATHS, _path_taken, _run

pytestmark = pytest.mark.gpu

R = 16
TINY = int(1 - E.SCALE[1])         # raw + offset == 1: |pA| = 0.17, the read fails the exactness guard


# ---------------------------------------------------------------- the reads
def stairs(rna, units=72):
    """noisy plateaus of 17 (DNA) / 33 (RNA) samples, 200 raw units apart: a usual emission per step, one block-relative
    index further each time; the noise keeps the long detector cold"""
    rs = np.random.RandomState(11 + rna)
    L = 33 if rna else 17
    level = np.repeat(np.tile([500, 700], units // 2 + 1)[:units], L)
    return level + rs.randint(-6, 7, size=level.size)


def roll_off(length, rna, base, front, back, onset=None):
    """E.decline with plateaus of `front` and `back` samples: the peak that opens at the onset is emitted about `length`
    indices behind its position"""
    x = E.decline(length, rna, onset or E.DECLINE_ONSET[rna], base)
    return x[60 - front:x.size - 60 + back]


#: seeds of roll_offs() that the search below kept: [rna]
ROLL_OFF_SEED = {0: 0, 1: 8}
#: [rna] -> (pieces, longest plateau + 1, longest roll-off + 1): a plateau is a certainly hot run when both long windows fit
ROLL_OFF_SHAPE = {0: (60, 25, 17), 1: (40, 45, 20)}
#: E.decline(4, 0, onset): a usual emission, then a peak that is emitted 3 = w1 indices behind its position (rare, and its
#: mask still reaches one index behind the emission)
ONSET_DNA_3_BEHIND = (0, 0, 12)


def roll_offs(rna, seed):
    """noise-free roll-offs of 4 and more samples between plateaus of 5 and more: rare emissions a few indices behind
    their peaks, next to the usual ones of the steps back down; the longer plateaus are hot runs of the long detector"""
    rs = np.random.RandomState(1000 * rna + seed)
    pieces, p_hi, l_hi = ROLL_OFF_SHAPE[rna]
    out = []
    for k in range(pieces):
        length, base, front, back = int(rs.randint(4, l_hi)), int(rs.randint(280, 420)), int(rs.randint(5, p_hi)), int(rs.randint(5, p_hi))
        if rna == 0 and k % 6 == 5:
            out.append(roll_off(4, 0, base, front, 12 + back, ONSET_DNA_3_BEHIND))
        else:
            out.append(roll_off(length, rna, base, front, back))
    return E.cat_(*out)


def seeds(rna):
    """the catalogue's seeds (a long-detector boundary each) behind plateaus of different lengths, in noise"""
    rs = np.random.RandomState(21 + rna)
    out = []
    for k in range(6):
        lo, hi = (1143, 1226) if rna else (876, 931)
        out += [lo + rs.randint(-8, 9, size=150 + 7 * k), E.rna_seed(60 + k, 80) if rna else E.dna_seed(42 + k, 75), hi + rs.randint(-8, 9, size=120)]
    return E.cat_(*out)


PART = 320    # samples of a part of the roll-offs: 8 lanes share it in chunks of 48, a hot run or two each


def reads_of(rna, packed=False):
    """-> (names, reads): the three kinds, and cuts of them that end 1, w1/2 + 1 and 15 indices into a block.  packed: for
    8 lanes per read, whose chunks would hold more hot runs of the roll-offs than a lane records (the read would take the
    fallback): the roll-offs in parts of 320 samples, cut at multiples of 16 so that every place keeps its block index"""
    h1 = E.PRESET[rna].w1 // 2
    full = {"stairs": stairs(rna), "roll_offs": roll_offs(rna, ROLL_OFF_SEED[rna]), "seeds": seeds(rna)}
    names, reads = [], []
    for name, x in full.items():
        names.append(name)
        reads.append(x)
    for name, cut in (("roll_offs", 1), ("seeds", h1 + 1), ("roll_offs", 15), ("stairs", 1), ("seeds", 15), ("stairs", h1 + 1)):
        x = full[name]
        n = (x.size * (2 + len(names) % 3) // 5) // R * R + cut      # different lengths: lanes of a packed wave finish apart
        names.append("%s_cut_%d" % (name, cut))
        reads.append(x[:n])
    if packed:
        keep = [k for k, name in enumerate(names) if not name.startswith("roll_offs")]
        names, reads = [names[k] for k in keep], [reads[k] for k in keep]
        x = full["roll_offs"]
        for k, a in enumerate(range(0, x.size - PART // 2, PART)):
            names.append("roll_offs_part_%d" % k)
            reads.append(x[a:a + PART + (1, h1 + 1, 15, 0)[k % 4]])
    return names, [np.ascontiguousarray(x, dtype=np.int16) for x in reads]


def flagged(reads):
    """the same reads with a tiny-|pA| sample and a large one (2^15 times as large: beyond what the guard lets a read of
    any length have) in the first plateau"""
    out = []
    for x in reads:
        y = x.copy()
        y[2], y[3] = TINY, 32000
        out.append(y)
    return out


# ---------------------------------------------------------------- which places a read reaches, by the branch model
USUAL_AT = ["usual_emission_at_block_index_%d" % u for u in range(R)]
PLACES = USUAL_AT + ["usual_peak_on_bit_31", "usual_peak_on_bit_0", "usual_emission_at_a_chunk_start", "usual_emission_at_a_chunk's_last_index",
                     "rare_emission_alone_in_its_block", "rare_emission_behind_a_usual_one_in_the_block",
                     "rare_emission_in_front_of_a_usual_one_in_the_block", "hot_run_starts_behind_the_mask_of_a_usual_emission",
                     "hot_run_starts_at_the_index_of_a_rare_emission", "hot_run_starts_behind_the_mask_of_a_rare_emission"]


def places(raw, rna, lanes=64):
    """lanes: how many lanes share the read (the chunks whose edges count)"""
    p = E.PRESET[rna]
    h1 = p.w1 // 2
    _, _, info = E.analyse(raw, rna)
    n = info["n"]
    em = info["short_emits"]                      # (position, index of the emission), in order
    _, own = E.lanes_whole(n, rna, lanes)
    starts, lasts = {s for s, _ in own[1:]}, {e - 1 for _, e in own[:-1]}
    out = set()
    usual = [i - x == h1 + 1 for x, i in em]
    for k, (x, i) in enumerate(em):
        if usual[k]:
            out.add(USUAL_AT[i % R])
            out |= {"usual_peak_on_bit_31"} if x % 32 == 31 else {"usual_peak_on_bit_0"} if x % 32 == 0 else set()
            out |= {"usual_emission_at_a_chunk_start"} if i in starts else set()
            out |= {"usual_emission_at_a_chunk's_last_index"} if i in lasts else set()
        else:
            before = k > 0 and em[k - 1][1] // R == i // R
            after = k + 1 < len(em) and em[k + 1][1] // R == i // R
            if not before and not after:
                out.add("rare_emission_alone_in_its_block")
            if before and usual[k - 1]:
                out.add("rare_emission_behind_a_usual_one_in_the_block")
            if after and usual[k + 1]:
                out.add("rare_emission_in_front_of_a_usual_one_in_the_block")
    by_index = {i: (x, u) for (x, i), u in zip(em, usual)}
    for r in info["runs"]:
        if not r.sure_hot or r.b >= n:            # recorded at the next reset, not at the read's end
            continue
        for i in range(r.a - p.w1, r.a + 1):      # the emission that was the last reset in front of the run
            if i in by_index:
                x, u = by_index[i]
                if r.a == x + p.w1 + 1 and r.a > i:
                    out.add("hot_run_starts_behind_the_mask_of_a_usual_emission" if u else "hot_run_starts_behind_the_mask_of_a_rare_emission")
                elif r.a == i and not u:
                    out.add("hot_run_starts_at_the_index_of_a_rare_emission")
    return out


def search_roll_off_seed(rna):
    want = set(PLACES) - set(USUAL_AT) - {"usual_emission_at_a_chunk_start", "usual_emission_at_a_chunk's_last_index",
                                          "usual_peak_on_bit_31", "usual_peak_on_bit_0"}
    for seed in range(400):
        if want <= places(roll_offs(rna, seed), rna):
            return seed
    return None


def test_the_reads_reach_their_places():
    """(needs no GPU work, but belongs to the reads: without it the parity below could pass on reads that miss a place)"""
    for rna in (0, 1):
        for packed in (False, True):
            names, reads = reads_of(rna, packed)
            got = set()
            for x in reads:
                got |= places(x, rna, 8 if packed else 64)
            assert not set(PLACES) - got, (rna, packed, sorted(set(PLACES) - got))
            h1 = E.PRESET[rna].w1 // 2
            assert {x.size % R for x in reads} >= {1, h1 + 1, 15}
            assert max(x.size for x in reads) <= 6000 and len({x.size for x in reads}) >= 9


# ---------------------------------------------------------------- parity
class _Expected:
    """the oracle's events, once per (read, preset, input type) for the module; shaped for _check_events"""

    def __init__(self, oracle):
        self.oracle, self.memo, self.as_pa = oracle, {}, False

    def event_raw(self, raw, dig, off, rng, rna):
        key = (raw.tobytes(), rna, self.as_pa)
        if key not in self.memo:
            o = self.oracle
            self.memo[key] = o.getevents(o.pa(raw, dig, off, rng), rna) if self.as_pa else o.event_raw(raw, dig, off, rng, rna)
        return self.memo[key]


@pytest.fixture(scope="module")
def expected(oracle):
    return _Expected(oracle)


def _compare(expected, names, reads, rna, as_pa, got, what):
    expected.as_pa = as_pa
    failures = []
    for r, (name, raw) in enumerate(zip(names, reads)):
        try:
            _check_events(expected, [raw], [E.SCALE[0]], [E.SCALE[1]], [E.SCALE[2]], rna, [got[r]])
        except AssertionError as e:
            failures.append("%s rna %d %s %s (n=%d): %s" % (what, rna, "pA" if as_pa else "int16", name, raw.size,
                                                           str(e).strip().split("\n")[0][:200]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("as_pa", [False, True], ids=["int16", "pa"])
@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("path", list(PATHS) + ["fallback"])
def test_bookkeeping_reads(gpu, oracle, options, expected, path, rna, as_pa):
    names, reads = reads_of(rna, packed=path == "packed8")
    if path == "fallback":
        reads = flagged(reads)
        options(**PATHS["whole"])
    else:
        options(**PATHS[path])
    got, st = _run(gpu, oracle, reads, rna, as_pa)
    print("bookkeeping %-12s rna %d %s: n_long_replays %d n_replay_indices %d n_fallback_reads %d n_split_reads %d n_rerun_passes %d" % (
        path, rna, "pA" if as_pa else "int16", st.n_long_replays, st.n_replay_indices, st.n_fallback_reads, st.n_split_reads,
        st.n_rerun_passes))
    _compare(expected, names, reads, rna, as_pa, got, path)
    assert st.n_capacity_overflow == 0
    if path == "fallback":
        assert st.n_fallback_reads == len(reads) and st.n_split_reads == 0
    else:
        _path_taken(gpu, path, reads, rna, st)
        assert st.n_fallback_reads == 0
    assert st.n_long_replays > 0 and st.n_replay_indices > 0


if __name__ == "__main__":
    for rna_ in (0, 1):
        print("ROLL_OFF_SEED[%d] = %r" % (rna_, search_roll_off_seed(rna_)))
        for name_, x_ in zip(*reads_of(rna_)):
            print(rna_, name_, x_.size, x_.size % R, len(places(x_, rna_)))
