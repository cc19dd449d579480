"""CPU: the bitmap word of k_event<3, *>'s fast pass (csrc/event_detect.h: LazyPass::bw, bw_advance, the flush at the end of
pass_lazy), one lane of it as plain Python, in its two forms side by side:

  * "bit" (SGK_EVENT_EMIT without bit 1): a usual emission at block-relative index u of the block at jb sets bit
    (jb + u - H1 - 1) & 31 of the word; the word goes to the ring and is zeroed when that position enters the next span
    (step H1 + 1 of a block with jb a multiple of 32); a rare emission clears the bit again;
  * "carry" (bit 1): every step shifts the word left by one and the emission in as bit 0 (bw + bw + carry), the steps of a
    block on the `oldpeak` path shift a zero in; the word is bit-reversed where it goes to the ring; the word that is left
    when the pass ends has seen m = (jb - H1 - 1) & 31 shifts and is reversed and moved down by 32 - m; a rare emission
    clears bit 0.  With and without zeroing the word where it goes to the ring: old bits leave at the top.

Both write the ring with OR, rare emissions and the emissions of oldpeak steps set their position's bit in the ring
directly, and the ring leaves for the read's bitmap in 16-bit units (lz_flush): pass-relative position p is bit
(i_begin + p) of the bitmap, i_begin a multiple of 16.  Required: the same ring words, and the bitmap that holds exactly
the emitted positions, for passes of every length up to 96 indices (in whole blocks), starting on either half of a
32-position span of the read, with emissions at every single index, at all of them, and at random ones.

Part 3 of the change this file was written for (the run start read off the emission history) is not built, so it has no
model here; tests/test_event_bookkeeping_model.py holds the run start of the shipped form."""
import random

import pytest

R, H1, RING_WORDS = 16, 1, 16
M32 = 0xffffffff


def bitrev32(w):
    return int("{:032b}".format(w)[::-1], 2)


def run_pass(form, steps, em, rare, oldpeak_blocks, zero=True):
    """one lane's pass of `steps` indices (a multiple of 16) -> ring words.  em[i]: an emission at pass-relative index i;
    rare[i]: position of the older peak it emits (None: the usual one, at i - H1 - 1); oldpeak_blocks: blocks (by jb)
    whose steps take the oldpeak path, where every emission goes to the ring directly"""
    ring = [0] * RING_WORDS
    bw = 0
    jb = 0
    while jb < steps:
        for u in range(R):
            i = jb + u
            if u == H1 + 1 and jb % 32 == 0:
                p = jb - 1
                ring[(p >> 5) & (RING_WORDS - 1)] |= bitrev32(bw) if form == "carry" else bw
                if zero or form == "bit":
                    bw = 0
            e = em[i]
            pos = i - H1 - 1 if rare[i] is None else rare[i]
            bit = 1 << ((jb + u - H1 - 1) & 31)
            if jb in oldpeak_blocks:
                if form == "carry":
                    bw = (bw + bw) & M32
                if e and pos >= 0:
                    ring[(pos >> 5) & (RING_WORDS - 1)] |= 1 << (pos & 31)
                continue
            if form == "carry":
                bw = (bw + bw + (1 if e else 0)) & M32
            elif e:
                bw |= bit
            if e and rare[i] is not None:
                bw &= ~1 & M32 if form == "carry" else ~bit & M32
                ring[(pos >> 5) & (RING_WORDS - 1)] |= 1 << (pos & 31)
        jb += R
    p = max(jb - H1 - 2, 0)
    w = bw
    if form == "carry":
        m = (jb - H1 - 1) & 31
        assert 0 < m < 32
        w = bitrev32(bw) >> (32 - m)
    ring[(p >> 5) & (RING_WORDS - 1)] |= w
    return ring


def bitmap(ring, i_begin, steps):
    """lz_flush: 16-bit units of the ring words -> {read positions set}"""
    out = set()
    for k in range(RING_WORDS):
        for half in (0, 1):
            unit = (ring[k] >> (16 * half)) & 0xffff
            p0 = 32 * k + 16 * half
            if p0 < steps:
                out |= {i_begin + p0 + b for b in range(16) if unit >> b & 1}
            else:
                assert unit == 0 or p0 >= 32 * (RING_WORDS - 1), (k, half, unit)   # (position -1, -2: the ring's last word)
    return out


def check(steps, em, rare=None, oldpeak_blocks=()):
    rare = rare or [None] * steps
    want = {(i - H1 - 1 if rare[i] is None else rare[i]) for i in range(steps) if em[i]}
    want = {p for p in want if p >= 0}
    rings = [run_pass("bit", steps, em, rare, oldpeak_blocks), run_pass("carry", steps, em, rare, oldpeak_blocks),
             run_pass("carry", steps, em, rare, oldpeak_blocks, zero=False)]
    for ring in rings:
        # (an emission at index 0 or 1 of a pass stands for a position in front of it: the ring's last word, never flushed)
        ring[RING_WORDS - 1] &= ~(3 << 30) if steps <= 32 * (RING_WORDS - 1) else M32
    assert rings[0] == rings[1] == rings[2], (steps, em, rare, oldpeak_blocks)
    for i_begin in (0, 16):
        assert bitmap(rings[1], i_begin, steps) == {i_begin + p for p in want}, (steps, i_begin, em)


def test_bitrev32():
    assert bitrev32(1) == 1 << 31 and bitrev32(0x80000001) == 0x80000001 and bitrev32(0x0000ffff) == 0xffff0000
    assert all(bitrev32(bitrev32(w)) == w for w in (0, 1, 0x12345678, M32))


@pytest.mark.parametrize("steps", [16, 32, 48, 64, 80, 96])
def test_every_length_single_all_and_random_emissions(steps):
    """lengths 1 .. 96: a pass of `steps` indices whose last emissions lie at every index up to its end"""
    for length in range(max(steps - 15, 1), steps + 1):
        for i in range(length):
            check(steps, [j == i for j in range(steps)])
        check(steps, [j < length for j in range(steps)])
        check(steps, [j < length and j % 2 == 0 for j in range(steps)])
    rs = random.Random(steps)
    for _ in range(300):
        dens = rs.choice((0.1, 0.5, 0.9))
        check(steps, [rs.random() < dens for _ in range(steps)])


@pytest.mark.parametrize("steps", [32, 48, 64, 96])
def test_rare_emissions_and_oldpeak_blocks(steps):
    """a rare emission at every index (its usual bit is the last before a flush at index 33, the first after one at 34),
    with usual emissions around it; blocks on the oldpeak path between fast ones"""
    rs = random.Random(1000 + steps)
    for i in range(4, steps):
        for back in (H1 + 2, 5, min(i, 20)):
            if i - back < 0 or back <= H1 + 1:
                continue
            em = [rs.random() < 0.3 for _ in range(steps)]
            rare = [None] * steps
            em[i] = True
            rare[i] = i - back
            # the older peak's position holds no usual emission's bit (an emission ends its peak)
            if i - back + H1 + 1 < steps:
                em[i - back + H1 + 1] = False
            check(steps, em, rare)
    for _ in range(300):
        em = [rs.random() < 0.4 for _ in range(steps)]
        blocks = {jb for jb in range(0, steps, R) if rs.random() < 0.4}
        check(steps, em, None, blocks)


def test_the_model_can_fail():
    """a final word that is reversed but not moved down is caught"""
    steps = 48
    em = [j == 40 for j in range(steps)]
    ring = run_pass("bit", steps, em, [None] * steps, ())
    bw = 0
    for i in range(34, steps):
        bw = (bw + bw + (1 if em[i] else 0)) & M32
    assert ring[1] == 1 << (38 & 31) == bitrev32(bw) >> (32 - ((steps - H1 - 1) & 31)) != bitrev32(bw)
