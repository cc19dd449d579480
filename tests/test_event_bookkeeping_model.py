"""CPU: the lazy long detector's bookkeeping in csrc/event_detect.h (LazyPass::dstep_core), one lane of it as plain Python,
in its two forms side by side:

  * "vector": lm (the short peak's position at the last emission) and r0 (the emission's index) per lane, the mask
    decided by the compare lm < u - W1 at every index, a run's start formed as max(r0, lm + W1 + 1) where it is recorded;
  * "history" (LazyPass::BOOK): the mask as NM - 1 = W1 - H1 - 1 carried lane masks (moff), the run's start as one value
    (rs).  The usual emission (its peak lies H1 + 1 indices back: em & hist[H1]) sets both from constants; the rare one
    (an older peak) and every emission of a block on the `oldpeak` path form them from sp.

Nothing else of the detector is modelled: a step takes what the short detector decided at the index -- pos (peak_pos =
i), em (the peak is emitted), dom (in a strong peak: the long detector is reset), hck (the long window may be hot), live
(the lane takes the step) -- and "usual" follows from the history of pos as in the kernel.  Positions are block-relative
and rebased every 16 indices as in pass_lazy; at every block boundary the state a chunk would hand over (LzSnapState's
lm and r0) is formed from either form.  Required equal at every index: on, hot, the recorded runs (start, end), and the
hand-over state at the boundaries.

Sequences are the valid ones: an emission needs a peak whose position was not set during the last H1 indices nor at
this one, dom needs a peak, and a lane that stops being live stays frozen (in the kernel a lane that steps on after a
frozen block is one that is `done`: nothing it decides lands anywhere).  "Exhaustive" walks every valid sequence of up
to 10 steps as a graph over the pairs of states: sequences that led both forms to the same pair of states have the same
continuations."""
import random

import pytest

R = 16
LZ_NONE = -(1 << 29)


class Cfg:
    def __init__(self, w1):
        self.W1, self.H1 = w1, w1 // 2
        self.NM = self.W1 - self.H1


# ---- what both forms share: the short detector's side (in a peak, peak position, history of pos)
def short_init():
    return (False, 0, ())          # inpk, sp, hist (filled to H1 + 1 by short_step)


def short_step(c, st, u, pos, em, live):
    inpk, sp, hist = st
    hist = hist or (False,) * (c.H1 + 1)
    if pos:
        sp = u
    inpk = (inpk and not em) or pos
    if live:
        hist = (pos,) + hist[:-1]   # a frozen lane's history does not age
    return (inpk, sp, hist)


# ---- form "vector"
def vec_init():
    return (LZ_NONE, 0, False)     # lm, r0, hot


def vec_step(c, st, short, u, ib, em, dom, hck, live):
    lm, r0, hot = st
    sp = short[1]
    rec = None
    if em:
        lm, r0 = sp, u
    if dom and hot:
        rec = (ib + max(r0, lm + c.W1 + 1), ib + u)
    on = (lm < u - c.W1) and live
    hot = (hot and not dom) or (on and hck and (not dom or em))
    return (lm, r0, hot), on, rec


def vec_rebase(st):
    lm, r0, hot = st
    return (LZ_NONE if lm < LZ_NONE else lm - R, r0 - R, hot)


def vec_snapshot(c, st, ib):
    lm, r0, _ = st
    return (LZ_NONE if lm + c.W1 < 0 else ib + lm + c.W1, ib + max(r0, lm + c.W1 + 1))


# ---- form "history"
def hist_init(c):
    return ((False,) * (c.NM - 1), 0, False)   # moff, rs, hot


def hist_step(c, st, short, u, ib, em, dom, hck, live, oldpeak):
    moff, rs, hot = st
    sp, hist = short[1], short[2] or (False,) * (c.H1 + 1)
    nm1 = c.NM - 1

    def from_sp(off, nx, kn):
        off = off or sp + c.W1 >= u
        nx = tuple(nx[k] or (k < kn and sp + c.W1 >= u + k + 1) for k in range(nm1))
        return off, nx
    if oldpeak:
        off, nx = moff[0] if nm1 else False, tuple(moff[k + 1] if k + 1 < nm1 else False for k in range(nm1))
        if em:
            rs = max(u, sp + c.W1 + 1)
            off, nx = from_sp(off, nx, nm1)
    else:
        usual = em and hist[c.H1]
        rare = em and not hist[c.H1]
        if em:
            rs = u + c.NM
        off = (moff[0] if nm1 else False) or usual
        nx = tuple((moff[k + 1] if k + 1 < nm1 else False) or usual for k in range(nm1))
        if rare:
            rs = max(u, sp + c.W1 + 1)
            off, nx = from_sp(off, nx, nm1 - 1)
    rec = (ib + rs, ib + u) if dom and hot else None
    on = (not off) and live
    if live:
        moff = nx                  # a frozen lane's mask does not age
    hot = (hot and not dom) or (on and hck and (not dom or em))
    return (moff, rs, hot), on, rec


def hist_rebase(st):
    moff, rs, hot = st
    return (moff, rs - R, hot)


def hist_snapshot(c, st, ib):
    _, rs, _ = st
    return (LZ_NONE if rs - 1 < 0 else ib + rs - 1, ib + rs)


def hist_from_snapshot(c, snap, i_begin, hot):
    """pass_lazy's start from a state that was handed over"""
    lm, r0 = snap
    mt = LZ_NONE if lm == LZ_NONE else lm - i_begin
    return (tuple(mt >= k for k in range(c.NM - 1)), max(r0 - i_begin, mt + 1), hot)


def vec_from_snapshot(c, snap, i_begin, hot):
    lm, r0 = snap
    return (LZ_NONE if lm == LZ_NONE else lm - c.W1 - i_begin, r0 - i_begin, hot)


# ---- the inputs a step may take in a state
def choices(c, short, live_before):
    """-> [(pos, em, dom, hck, live)] valid at this index"""
    inpk, _, hist = short
    hist = hist or (False,) * (c.H1 + 1)
    out = []
    for live in ((True, False) if live_before else (False,)):
        if not live:
            out.append((False, False, False, True, False))   # the kernel masks pos, em and dom of a frozen lane
            continue
        kinds = [(False, False), (True, False)]
        if inpk and not any(hist[:c.H1]):
            kinds.append((False, True))
        for pos, em in kinds:
            for dom in ((False, True) if inpk else (False,)):
                for hck in (False, True):
                    out.append((pos, em, dom, hck, True))
    return out


class Pair:
    """both forms (and the history form on the oldpeak path) in step"""

    def __init__(self, c, i0, state=None):
        self.c, self.i = c, i0
        self.short, self.vec, self.his, self.old, self.live = state or (short_init(), vec_init(), hist_init(c), hist_init(c), True)

    def key(self):
        return (self.i, self.short, self.vec, self.his, self.old, self.live)

    def step(self, inp):
        c = self.c
        pos, em, dom, hck, live = inp
        u, ib = self.i % R, self.i - self.i % R
        pos, em, dom = pos and live, em and live, dom and live
        v, on_v, rec_v = vec_step(c, self.vec, self.short, u, ib, em, dom, hck, live)
        h, on_h, rec_h = hist_step(c, self.his, self.short, u, ib, em, dom, hck, live, False)
        o, on_o, rec_o = hist_step(c, self.old, self.short, u, ib, em, dom, hck, live, True)
        assert on_v == on_h == on_o, ("on", self.i, inp, self.key())
        assert v[2] == h[2] == o[2], ("hot", self.i, inp, self.key())
        assert rec_v == rec_h == rec_o, ("recorded run", self.i, inp, self.key(), rec_v, rec_h, rec_o)
        self.short = short_step(c, self.short, u, pos, em, live)
        self.vec, self.his, self.old, self.live = v, h, o, live
        self.i += 1
        if self.i % R == 0:
            inpk, sp, hist = self.short
            self.short = (inpk, sp - R, hist)
            self.vec, self.his, self.old = vec_rebase(self.vec), hist_rebase(self.his), hist_rebase(self.old)
            sv, sh, so = vec_snapshot(c, self.vec, self.i), hist_snapshot(c, self.his, self.i), hist_snapshot(c, self.old, self.i)
            assert sv == sh == so, ("hand-over state", self.i, sv, sh, so)
            # ... and a pass that starts from the state handed over is where this one is (a frozen lane's mask has not
            # aged: it hands nothing over)
            if live:
                assert hist_from_snapshot(c, sv, self.i, h[2]) == self.his == self.old, (self.i, sv, self.his)
            if self.vec[0] + c.W1 >= 0:   # (the vector form normalises a mask that no longer masks away)
                assert vec_from_snapshot(c, sv, self.i, v[2])[0] == self.vec[0]
        return rec_v, on_v


@pytest.mark.parametrize("i0", [0, 9, 13])
def test_every_sequence_of_up_to_10_steps_w1_3(i0):
    """W1 = 3, from the start of a block and from two places that put a block boundary (the rebase, the hand-over state)
    inside the sequence"""
    c = Cfg(3)
    frontier = {Pair(c, i0).key()}
    n_steps = n_rec = n_rare = 0
    for _ in range(10):
        nxt = set()
        for key in frontier:
            i, short, vec, his, old, live = key
            for inp in choices(c, short, live):
                p = Pair(c, i, (short, vec, his, old, live))
                hist = short[2] or (False,) * (c.H1 + 1)
                n_rare += bool(inp[1] and not hist[c.H1])
                rec, _ = p.step(inp)
                n_rec += rec is not None
                n_steps += 1
                nxt.add(p.key())
        frontier = nxt
    print("bookkeeping model: i0 %d, %d transitions, %d state pairs at depth 10, %d recorded runs, %d rare emissions" % (
        i0, n_steps, len(frontier), n_rec, n_rare))
    assert n_rec > 0 and n_rare > 0


@pytest.mark.parametrize("w1", [3, 7])
def test_random_sequences_of_64_steps(w1):
    c = Cfg(w1)
    rs = random.Random(100 + w1)
    n_rec = n_rare = n_usual = n_masked = 0
    starts = set()
    for trial in range(4000):
        p = Pair(c, rs.choice((0, 3, 11)))
        freeze = rs.choice((None, None, rs.randrange(1, 64)))
        for k in range(64):
            ch = choices(c, p.short, p.live)
            ch = [x for x in ch if x[4] == (p.live and (freeze is None or k < freeze))] or ch
            # emissions and resets often enough for hot runs to be recorded
            w = [4 if x[1] else 2 if x[2] else 1 for x in ch]
            inp = rs.choices(ch, w)[0]
            hist = p.short[2] or (False,) * (c.H1 + 1)
            n_rare += bool(inp[1] and not hist[c.H1])
            n_usual += bool(inp[1] and hist[c.H1])
            rec, on = p.step(inp)
            n_masked += not on
            if rec is not None:
                n_rec += 1
                starts.add(rec[0] - (rec[1] - rec[1] % R))
    print("bookkeeping model: W1 %d: %d recorded runs (%d different block-relative starts), %d usual and %d rare emissions, "
          "%d masked steps" % (w1, n_rec, len(starts), n_usual, n_rare, n_masked))
    assert n_rec > 100 and n_rare > 100 and n_usual > 100 and n_masked > 100


def test_the_model_can_fail():
    """a history one index short (NM - 1 instead of NM indices masked) is caught"""
    c = Cfg(3)
    c.NM = 1
    with pytest.raises(AssertionError):
        frontier = {Pair(c, 0).key()}
        for _ in range(8):
            nxt = set()
            for key in frontier:
                for inp in choices(c, key[1], key[5]):
                    p = Pair(c, key[0], key[1:])
                    p.step(inp)
                    nxt.add(p.key())
            frontier = nxt
