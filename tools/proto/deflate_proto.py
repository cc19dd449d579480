"""CPU model of k_deflate (sigtk_amd/csrc/deflate_kernels.hip): the zlib stream the kernel writes, byte for byte.

The stream: header 78 9C; DEFLATE blocks over DEF_BLOCK input bytes each; big-endian Adler-32.

Tokens of a block: literals and matches of distance 1.  A maximal run of L equal bytes inside the block is one literal
and then matches over its other L - 1 bytes, greedily 258 at a time; a rest of 1 or 2 bytes is written as literals.
Runs end at the block's end.

A block is a dynamic-Huffman block when that takes fewer bits than a stored block from the same bit position (the
stored block's padding to the byte boundary counted), else a stored block.

Huffman code lengths (build_lengths): the used symbols sorted by (count, symbol); a Huffman tree by the two-queue
method (of a leaf and an internal node of equal weight the internal node is taken first); the number of leaves per depth,
depths beyond the limit counted at the limit; while the code is over-subscribed, zlib's repair step (a leaf of the
deepest level above the limit moves one level down and takes one leaf from the limit as its sibling: 2^-limit less);
then the lengths are handed out over the sorted order, longest to the rarest.  Codes are canonical.

Code lengths in the block header: the literal/length lengths (HLIT trimmed to the last used symbol) followed by the one
distance length (1 with a match in the block, else 0), run-length coded as one sequence:
  zeros:   18 for 11 .. 138 at a time while at least 11 are left, then 17 for 3 .. 10, else the zeros themselves
  others:  the length once, then 16 for 3 .. 6 at a time while at least 3 are left, then the length itself
The code length code is limited to 7 bits with the same builder.
"""
from __future__ import annotations

import numpy as np

DEF_BLOCK = 16384
CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def deflate_bound(n: int, block: int = DEF_BLOCK) -> int:
    per = min(block, 65535)
    return n + 5 * max(1, -(-n // per)) + 6


def adler32(x: np.ndarray) -> int:
    a, b = 1, 0
    for i in range(0, x.size, 1024):
        t = x[i:i + 1024].astype(np.int64)
        m = t.size
        b = (b + m * a + int((t * (m - np.arange(m))).sum())) % 65521
        a = (a + int(t.sum())) % 65521
    return (b << 16) | a


def build_lengths(freq, maxbits: int):
    """freq: counts per symbol -> code length per symbol (0: unused).  A single used symbol gets a partner (symbol 0,
    or 1 when 0 is the used one) with count 1, as zlib forces two codes."""
    freq = [int(f) for f in freq]
    used = [s for s, f in enumerate(freq) if f]
    if len(used) < 2:
        extra = 0 if 0 not in used else 1
        freq[extra] = 1
        if not used:
            freq[1 if extra == 0 else 0] = 1
        used = [s for s, f in enumerate(freq) if f]
    order = sorted(used, key=lambda s: (freq[s], s))
    n = len(order)
    w = [freq[s] for s in order] + [0] * (n - 1)
    par = [0] * (2 * n - 1)
    li, ii = 0, n
    for node in range(n, 2 * n - 1):
        for _ in range(2):
            if li < n and (ii >= node or w[li] < w[ii]):
                pick = li
                li += 1
            else:
                pick = ii
                ii += 1
            w[node] += w[pick]
            par[pick] = node
    root = 2 * n - 2
    count = [0] * (maxbits + 1)
    for leaf in range(n):
        d, x = 0, leaf
        while x != root:
            x = par[x]
            d += 1
        count[min(d, maxbits)] += 1
    excess = sum(count[b] << (maxbits - b) for b in range(1, maxbits + 1)) - (1 << maxbits)
    while excess > 0:
        bits = maxbits - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[maxbits] -= 1
        excess -= 1
    lens = [0] * len(freq)
    q = 0
    for bits in range(maxbits, 0, -1):
        for _ in range(count[bits]):
            lens[order[q]] = bits
            q += 1
    return lens


def canonical_codes(lens):
    """bit-reversed canonical codes (as they enter an LSB-first bit stream)"""
    maxb = max(lens) if lens else 0
    count = [0] * (maxb + 2)
    for v in lens:
        if v:
            count[v] += 1
    nxt = [0] * (maxb + 2)
    code = 0
    for b in range(1, maxb + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            c = nxt[v]
            nxt[v] += 1
            out[s] = int(format(c, "0%db" % v)[::-1], 2)
    return out


def length_symbol(ln: np.ndarray):
    """match length 3 .. 258 -> (symbol, extra bits, extra value)"""
    ln = np.asarray(ln, dtype=np.int64)
    l3 = ln - 3
    e = np.where(l3 >= 8, np.floor(np.log2(np.maximum(l3, 1))).astype(np.int64) - 2, 0)
    sym = np.where(l3 < 8, 257 + l3, 261 + 4 * e + ((l3 >> e) & 3))
    xv = np.where(l3 < 8, 0, l3 & ((1 << e) - 1))
    sym = np.where(ln == 258, 285, sym)
    e = np.where(ln == 258, 0, e)
    xv = np.where(ln == 258, 0, xv)
    return sym, e, xv


def tokens(b: np.ndarray):
    """the block's tokens in stream order: (symbol, extra bits, extra value, is_match) arrays"""
    m = b.size
    idx = np.arange(m)
    start = np.ones(m, dtype=bool)
    start[1:] = b[1:] != b[:-1]
    k = idx - np.maximum.accumulate(np.where(start, idx, 0))
    end = np.ones(m, dtype=bool)
    end[:-1] = b[1:] != b[:-1]
    o = (k - 1) % 258
    full = (k >= 1) & (o == 257)
    rest = (k >= 1) & end & ~full
    rlen = o + 1
    mt = full | (rest & (rlen >= 3))
    lit1 = (k == 0) | (rest & (rlen < 3))
    lit2 = rest & (rlen == 2)
    mlen = np.where(full, 258, rlen)
    msym, mext, mval = length_symbol(np.where(mt, mlen, 3))
    # at most two tokens per position: (match) or (literal [, literal])
    sym = np.stack([np.where(mt, msym, b.astype(np.int64)), b.astype(np.int64)], axis=1)
    ext = np.stack([np.where(mt, mext, 0), np.zeros(m, dtype=np.int64)], axis=1)
    val = np.stack([np.where(mt, mval, 0), np.zeros(m, dtype=np.int64)], axis=1)
    ism = np.stack([mt, np.zeros(m, dtype=bool)], axis=1)
    keep = np.stack([mt | lit1, lit2], axis=1)
    return sym[keep], ext[keep], val[keep], ism[keep]


def rle_lengths(seq):
    """the code length sequence -> [(code length symbol, extra bits, extra value)]"""
    out = []
    i, n = 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                out.append((18, 7, t - 11))
                r -= t
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out.extend([(0, 0, 0)] * r)
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                out.append((16, 2, t - 3))
                r -= t
            out.extend([(v, 0, 0)] * r)
    return out


class BitWriter:
    def __init__(self):
        self.vals = []
        self.nbs = []
        self.nbits = 0

    def put(self, val, nb):
        val = np.atleast_1d(np.asarray(val, dtype=np.uint64))
        nb = np.atleast_1d(np.asarray(nb, dtype=np.int64))
        self.vals.append(val)
        self.nbs.append(nb)
        self.nbits += int(nb.sum())

    def align(self):
        self.put(0, (-self.nbits) % 8)

    def bytes(self) -> bytes:
        vals = np.concatenate(self.vals)
        nbs = np.concatenate(self.nbs)
        offs = np.cumsum(nbs) - nbs
        total = int(nbs.sum())
        rep = np.repeat(np.arange(vals.size), nbs)
        bit = np.arange(total) - np.repeat(offs, nbs)
        bits = ((vals[rep] >> bit.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits, bitorder="little").tobytes()


def plan_block(b: np.ndarray):
    """everything about the block's dynamic form: dict with the lengths, the header items and the size in bits"""
    sym, ext, val, ism = tokens(b)
    freq = np.bincount(sym, minlength=286).astype(np.int64)
    freq[256] = 1
    lens = build_lengths(freq, 15)
    has_match = bool(ism.any())
    nlit = max(257, max(s for s in range(286) if lens[s]) + 1)
    seq = lens[:nlit] + [1 if has_match else 0]
    items = rle_lengths(seq)
    clfreq = [0] * 19
    for s, _, _ in items:
        clfreq[s] += 1
    cllens = build_lengths(clfreq, 7)
    ncl = 19
    while ncl > 4 and cllens[CLORDER[ncl - 1]] == 0:
        ncl -= 1
    bits = 3 + 14 + 3 * ncl + sum(cllens[s] + e for s, e, _ in items)
    bits += int(sum(int(freq[s]) * lens[s] for s in range(286))) + int(ext.sum()) + int(ism.sum())
    return dict(sym=sym, ext=ext, val=val, ism=ism, lens=lens, nlit=nlit, items=items, cllens=cllens, ncl=ncl, bits=bits,
                has_match=has_match)


def deflate(data, block: int = DEF_BLOCK, info=None, choose=None) -> bytes:
    """info (a list) receives one dict per block: type ('dynamic' / 'stored'), pos (the bit position in its byte at which
    the block starts), the plan of its dynamic form.  choose(dynamic bits, pos, block bytes) -> bool replaces the rule
    that picks the form (tests: a block forced dynamic, wrong rules that the checks must catch)"""
    x = np.frombuffer(bytes(data), dtype=np.uint8)
    w = BitWriter()
    w.put(0x78 | (0x9C << 8), 16)
    nblocks = max(1, -(-x.size // block))
    for bi in range(nblocks):
        b = x[bi * block:(bi + 1) * block]
        final = 1 if bi == nblocks - 1 else 0
        p = plan_block(b)
        pos = w.nbits & 7
        stored_bits = 3 + ((-(pos + 3)) % 8) + 32 + 8 * b.size
        dynamic = p["bits"] < stored_bits if choose is None else bool(choose(p["bits"], pos, b.size))
        if info is not None:
            info.append(dict(type="dynamic" if dynamic else "stored", pos=pos, **p))
        if not dynamic:
            w.put(final, 3)
            w.align()
            w.put(b.size | ((b.size ^ 0xFFFF) << 16), 32)
            if b.size:
                w.put(b.astype(np.uint64), np.full(b.size, 8))
            continue
        lens, cllens = p["lens"], p["cllens"]
        codes, clcodes = canonical_codes(lens), canonical_codes(cllens)
        w.put(final | (2 << 1) | ((p["nlit"] - 257) << 3) | (0 << 8) | ((p["ncl"] - 4) << 13), 17)
        w.put([cllens[CLORDER[k]] for k in range(p["ncl"])], [3] * p["ncl"])
        w.put([clcodes[s] | (v << cllens[s]) for s, e, v in p["items"]], [cllens[s] + e for s, e, v in p["items"]])
        la = np.asarray(lens, dtype=np.int64)
        ca = np.asarray(codes, dtype=np.int64)
        sym, ext, val, ism = p["sym"], p["ext"], p["val"], p["ism"]
        # a match: length code, extra bits, then the one-bit distance code 0
        w.put((ca[sym] | (val << la[sym])).astype(np.uint64), la[sym] + ext + ism.astype(np.int64))
        w.put(codes[256], lens[256])
    w.align()
    ad = adler32(x)
    w.put([(ad >> 24) & 255, (ad >> 16) & 255, (ad >> 8) & 255, ad & 255], [8] * 4)
    return w.bytes()


if __name__ == "__main__":
    import sys
    import zlib
    raw = open(sys.argv[1], "rb").read() if len(sys.argv) > 1 else bytes(100000)
    blocks = []
    z = deflate(raw, info=blocks)
    assert zlib.decompress(z) == raw
    print("%d -> %d bytes (bound %d), blocks: %s" % (len(raw), len(z), deflate_bound(len(raw)),
                                                    " ".join(b["type"][0] for b in blocks)))
