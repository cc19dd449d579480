"""Hand-made reads for the emission bookkeeping of k_event<3, *>'s fast pass (csrc/event_detect.h: SGK_EVENT_EMIT), and the
model that says which of its places a read reaches.

A lane of the fast pass walks its chunk in blocks of 16 indices and keeps the peaks it emits in a bitmap word of 32
pass-relative positions.  A usual emission (the peak lies 2 indices back) is shifted into that word as the carry of one
add, so the word is built in reversed order; it is bit-reversed where it leaves for the lane's ring in LDS (once per 32
positions, decided at a position with residue 0 of a span), and right-aligned first where the pass ends with a partly
filled word.  A rare emission (an older peak) takes its bit back and sets the right one in the ring.  The rare emission and
the recorded hot run of the long detector sit behind one test per index.

The geometry is restated from tests/event_cases.py (lanes_whole): a read of n samples is cut into chunks of K samples, K a
multiple of 16; lane c > 0 starts its pass at c * K, warms up over `lead` samples and owns [c * K + lead, (c + 1) * K + lead).
Positions in a pass are relative to its first index, so the span of a peak at x is (x - c * K) >> 5 and its residue
(x - c * K) & 31.  `places` works all of that out from the branch model's emissions (event_cases.peaks_model, which
tests/test_event_emit_cases_cpu.py holds against the oracle's boundaries on every read here).

The reads are staircases (plateaus of 4 to 9 samples, 40 raw units apart, noise of +-2: a boundary on every step with the
DNA preset), stretches of noise, and noise-free pieces of tests/event_cases.py: its DNA seed (a hot run of the long
detector behind an emission) and the onset of a smooth transition whose short peak is emitted 4 indices behind its
position.  Where a place needs a position, a search finds the length of the stretch in front (`python
tests/event_emit_cases.py`), and what it found is committed in END_FOUND, RARE_FOUND and RUN_FOUND."""
import numpy as np

import event_cases as E

LEAD = 32                      # LEAD_DNA_SHORT: every read here is shorter than 32 768 samples
H1 = 1                         # w1 / 2 of the DNA preset: the usual emission lies H1 + 1 indices behind its peak
NM = 2                         # the long detector's run starts NM indices behind a usual emission
W2 = 6


def lanes(n, lead=LEAD):
    """-> (K, [(first index of the pass, s, e)]): the pass and the range [s, e) of every lane of a whole read's wavefront"""
    K = E.chunk_len_fast(n, lead)
    out = []
    for c in range(64):
        s = 0 if c == 0 else c * K + lead
        e = min(lead + K if c == 0 else s + K, n)
        if s < n:
            out.append((c * K, s, e))
    return K, out


def _lane(own, x):
    for c, (_, s, e) in enumerate(own):
        if s <= x < e:
            return c
    raise AssertionError(x)


RESIDUE_FIRST = {r: "residue_%d_in_the_first_span_of_a_chunk" % r for r in range(32)}
RESIDUE_LATER = {r: "residue_%d_in_a_later_span" % r for r in range(32)}
K_ODD = "chunks_of_an_odd_multiple_of_16:the_pass_ends_14_shifts_into_a_word"
K_EVEN = "chunks_of_a_multiple_of_32:the_pass_ends_30_shifts_into_a_word"
END_M = {m: "the_read_ends_%d_positions_into_a_span_behind_an_emission" % m for m in (1, 15, 16, 17, 31)}
EMIT_PREDICATED = "emission_in_the_predicated_steps_at_the_read's_end"
EMIT_LAST_BLOCK = "emission_in_the_last_block_of_a_chunk:the_lane_is_frozen_right_after"
RARE_LAST_BIT = "rare_emission_whose_usual_bit_is_the_last_before_a_flush"
RARE_FIRST_BIT = "rare_emission_whose_usual_bit_is_the_first_after_a_flush"
RUN_SAME_WORD = "recorded_hot_run_starts_behind_an_emission_in_the_current_word"
RUN_PREVIOUS_WORD = "recorded_hot_run_starts_behind_an_emission_in_the_previous_word"
RUN_OLDER = "recorded_hot_run_starts_behind_an_emission_more_than_32_indices_back"
PLACES = tuple(RESIDUE_FIRST.values()) + tuple(RESIDUE_LATER.values()) + (K_ODD, K_EVEN) + tuple(END_M.values()) + (
    EMIT_PREDICATED, EMIT_LAST_BLOCK, RARE_LAST_BIT, RARE_FIRST_BIT, RUN_SAME_WORD, RUN_PREVIOUS_WORD, RUN_OLDER)


def places(n, short_emits, runs, lead=LEAD):
    """the places a whole read of n samples reaches: short_emits [(peak position, index of its emission)] and runs (Run) as
    event_cases.peaks_model gives them for the DNA preset"""
    out = set()
    if n < 64:
        return out
    K, own = lanes(n, lead)
    out.add(K_ODD if (K // 16) % 2 else K_EVEN)
    emitted_at = {i: x for x, i in short_emits}
    last = len(own) - 1
    for x, i in short_emits:
        c = _lane(own, x)
        ib, s, e = own[c]
        if i >= e:
            continue                   # pending at the chunk's end: the lane behind emits it (lz_emit_slow)
        blk = ib + (i - ib) // 16 * 16
        predicated = blk + 15 > n - W2
        if i - x == H1 + 1:
            p = x - ib
            out.add((RESIDUE_FIRST if p >> 5 == (s - ib) >> 5 else RESIDUE_LATER)[p & 31])
            if predicated:
                out.add(EMIT_PREDICATED)
            if c < last and i >= e - 16:
                out.add(EMIT_LAST_BLOCK)
            if x >= n - 8 and (n - ib) & 31 in END_M:     # (the lane that holds the read's last indices, or the one in front)
                out.add(END_M[(n - ib) & 31])
        elif i - x <= 200 and not predicated and x >= blk - 200:
            # an older peak met in a fast step: the bit the step shifted in stands for position i - H1 - 1
            u = (i - H1 - 1 - ib) & 31
            if u == 31:
                out.add(RARE_LAST_BIT)
            if u == 0:
                out.add(RARE_FIRST_BIT)
    for r in runs:
        if not r.sure_hot or r.b >= n:
            continue
        c = _lane(own, r.b)
        ib, s, e = own[c]
        ie = r.a - NM                  # the index of the emission the run starts behind
        if emitted_at.get(ie) != ie - H1 - 1 or ie - H1 - 1 < ib:
            continue                   # (not a usual emission of this pass)
        wa, wb = (ie - H1 - 1 - ib) >> 5, (r.b - H1 - 1 - ib) >> 5
        if wb == wa:
            out.add(RUN_SAME_WORD)
        elif wb == wa + 1 and r.b - r.a <= 32:
            out.add(RUN_PREVIOUS_WORD)
        elif r.b - r.a > 32:
            out.add(RUN_OLDER)
    return out


def analyse(raw):
    """-> (short_emits, runs) of the branch model with the DNA preset"""
    info = E.analyse(raw, 0)[2]
    return info["short_emits"], info["runs"]


def places_of(raw, lead=LEAD):
    se, runs = analyse(raw)
    return places(len(raw), se, runs, lead)


# ---------------------------------------------------------------- the reads
NOISE_SEED = 11


def stairs(rs, n, plateau, level=500):
    """n samples of plateaus of `plateau` samples, 40 raw units apart, noise of +-2"""
    reps = n // plateau + 1
    lv = level + 40 * (np.arange(reps) & 1)
    return (np.repeat(lv, plateau)[:n] + rs.randint(-2, 3, size=n)).astype(np.int64)


def noisy(rs, n, level, amp=8):
    return level + rs.randint(-amp, amp + 1, size=n)


#: the onset of event_cases.train(3, 1500, ("smooth",)): its short peak at 70 is emitted at 74
RARE_PIECE = (40, 110)


def rare_piece():
    a, b = RARE_PIECE
    return E.train(3, 1500, ("smooth",))[a:b]


def build(spec):
    """-> int16 read of a spec: a list of parts ("stairs", samples, plateau) | ("noise", samples, level) | ("rare",) |
    ("seed", front plateau, back plateau) | ("step", samples): a plateau 200 above the last level"""
    rs = np.random.RandomState(NOISE_SEED)
    parts = []
    for part in spec:
        kind = part[0]
        if kind == "stairs":
            parts.append(stairs(rs, part[1], part[2]))
        elif kind == "noise":
            parts.append(noisy(rs, part[1], part[2]))
        elif kind == "rare":
            parts.append(rare_piece())
        elif kind == "seed":
            parts.append(E.dna_seed(part[1], part[2]))
        elif kind == "step":
            parts.append(noisy(rs, part[1], 740, 2))
        else:
            raise ValueError(kind)
    return E.cat_(*parts).astype(np.int16)


def _end_spec(n, tail):
    """a staircase of 5-sample plateaus that ends, n samples long, `tail` samples behind a step"""
    return [("stairs", n - tail, 5), ("step", tail)]


def search_end(m):
    """(n, tail) of _end_spec: the read ends m positions into a span of its last lane, behind an emission"""
    for n in range(1400, 1600):
        for tail in range(3, 9):
            if END_M[m] in places_of(build(_end_spec(n, tail))):
                return n, tail
    return None


def _rare_spec(front):
    return [("noise", front, 600), ("rare",), ("noise", 2000, 900)]


def search_rare(tag):
    for front in range(1000, 1100):
        if tag in places_of(build(_rare_spec(front))):
            return front
    return None


def _run_spec(front, back):
    return [("noise", front, 876), ("seed", 42, back), ("noise", 2500, 931)]


def search_run(tag):
    for back in ((75, 44) if tag == RUN_OLDER else (6, 10, 14, 20, 30)):
        for front in range(1000, 1096):
            if tag in places_of(build(_run_spec(front, back))):
                return front, back
    return None


#: what the searches found: m -> (n, tail); tag -> front; tag -> (front, back)
END_FOUND = {1: (1409, 4), 15: (1423, 3), 16: (1424, 3), 17: (1425, 3), 31: (1407, 3)}
RARE_FOUND = {RARE_LAST_BIT: 1055, RARE_FIRST_BIT: 1056}
RUN_FOUND = {RUN_SAME_WORD: (1000, 6), RUN_PREVIOUS_WORD: (1024, 6), RUN_OLDER: (1000, 75)}


def specs():
    """name -> spec"""
    out = {"stairs_7_5000": [("stairs", 5000, 7)],        # K = 80: 63 lanes, every residue in first and later spans
           "stairs_7_1500": [("stairs", 1500, 7)],        # K = 32
           "stairs_4_2100": [("stairs", 2100, 4)],        # K = 48, the densest staircase a builder tile takes (512 records)
           "stairs_9_700": [("stairs", 700, 9)]}          # K = 16: every block is a chunk's last
    for m, (n, tail) in sorted(END_FOUND.items()):
        out["end_m%d" % m] = _end_spec(n, tail)
    for tag, front in sorted(RARE_FOUND.items()):
        out["rare_%s" % ("last_bit" if tag == RARE_LAST_BIT else "first_bit")] = _rare_spec(front)
    for tag, (front, back) in sorted(RUN_FOUND.items()):
        out["run_%s" % {RUN_SAME_WORD: "same_word", RUN_PREVIOUS_WORD: "previous_word", RUN_OLDER: "older"}[tag]] = _run_spec(front, back)
    return out


def reads():
    """-> (names, int16 reads)"""
    sp = specs()
    names = sorted(sp)
    return names, [build(sp[k]) for k in names]


if __name__ == "__main__":
    print("END_FOUND = %r" % {m: search_end(m) for m in END_M})
    print("RARE_FOUND = %r" % {t: search_rare(t) for t in (RARE_LAST_BIT, RARE_FIRST_BIT)})
    print("RUN_FOUND = %r" % {t: search_run(t) for t in (RUN_SAME_WORD, RUN_PREVIOUS_WORD, RUN_OLDER)})
    got = set()
    for name, x in zip(*reads()):
        p = places_of(x)
        got |= p
        print("%-24s n %5d  %d places" % (name, x.size, len(p)))
    print("missing:", sorted(set(PLACES) - got))
