"""A DEFLATE / zlib stream WRITER for tests (RFC 1950, RFC 1951), written from the RFCs: bit writer, canonical codes, stored /
fixed / dynamic block emitters that also write what no compressor writes (and what no inflate may accept), a token model
with a plain expander, and two catalogues built from fixed seeds:

    valid_streams()    -> [(name, stream, expected bytes)]
    invalid_streams()  -> [(name, stream, sgk_inflate status, fragment of zlib's error text)]
    coverage()         -> what the valid catalogue's writer wrote (symbols, code lengths, seams, stored-header bit offsets)

tests/test_deflate_craft_cpu.py has zlib judge every entry; tests/test_gpu_inflate.py gives them to sgk_inflate.  The cases
sit on the constants of sigtk_amd/csrc/inflate_kernels.hip (NEAR = 3838: the furthest match served from the LDS ring, LB = 10
/ DB = 8: look-up table bits, RUN = 16: literals per parallel run, FLUSH = 1024: bytes per flush), named here only as numbers
the cases are built around -- no kernel code is used."""
import bisect
import zlib

import numpy as np

NEAR, LB, DB, RUN, FLUSH, CHUNK_BYTES = 3838, 10, 8, 16, 1024, 256

CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0) + tuple(e for e in range(1, 14) for _ in (0, 1))
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8       # 288 symbols: 286 and 287 have codes and no meaning
FIXED_DIST = [5] * 32                                         # 30 and 31 likewise


def length_symbol(length, alt=False):
    """-> (symbol, extra bits, extra value); alt: 258 as symbol 284 with all five extra bits set (legal, never emitted)"""
    assert 3 <= length <= 258
    if length == 258 and not alt:
        return 285, 0, 0
    k = bisect.bisect_right(LBASE, length) - 1
    if length == 258:
        k = 27
    return 257 + k, LEXT[k], length - LBASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = bisect.bisect_right(DBASE, dist) - 1
    return k, DEXT[k], dist - DBASE[k]


def canonical(lengths):
    """RFC 1951 3.2.2: code of every symbol (most significant bit first), 0 where the length is 0.  Over-subscribed and
    incomplete sets get the codes the same rule gives them."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        nxt[n] += 1 if n else 0
    return out


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def rev_codes(lengths):
    return [_rev(c, n) for c, n in zip(canonical(lengths), lengths)]


def kraft(lengths):
    """sum of 2^-len in units of 2^-15"""
    return sum(1 << (15 - n) for n in lengths if n)


def expand(tokens, out=None):
    """the plain expander: ('lit', b) | ('match', len, dist[, alt]) -> bytes"""
    out = bytearray() if out is None else out
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            ln, d = t[1], t[2]
            assert 1 <= d <= len(out), (d, len(out))
            if d >= ln:
                s = len(out) - d
                out += out[s:s + ln]
            else:
                for _ in range(ln):
                    out.append(out[-d])
    return out


def lits(data):
    return [("lit", b) for b in data]


# --------------------------------------------------------------------------- complete code length sets

def complete_lengths(rng, k, maxlen=15, deep=0):
    """k >= 2 code lengths with Kraft sum exactly 1 and maximum <= maxlen; deep: at least one code of that length (a chain
    of splits down to it first; needs k > deep)"""
    assert 2 <= k <= (1 << maxlen) and deep <= maxlen and (deep == 0 or k > deep)
    leaves = [1, 1]
    while len(leaves) < k and max(leaves) < deep:
        d = max(leaves)
        leaves.remove(d)
        leaves += [d + 1, d + 1]
    if deep:
        leaves.remove(deep)                       # (kept aside: the random splits leave this one alone)
    balanced = rng.rand() < 0.5
    while len(leaves) + (1 if deep else 0) < k:
        open_ = [d for d in leaves if d < maxlen]
        if balanced:
            w = np.array([2.0 ** -d for d in open_])
            d = open_[int(rng.choice(len(open_), p=w / w.sum()))]
        else:
            d = open_[int(rng.randint(len(open_)))]
        leaves.remove(d)
        leaves += [d + 1, d + 1]
    if deep:
        leaves.append(deep)
    assert len(leaves) == k and kraft(leaves) == 1 << 15 and max(leaves) <= maxlen
    rng.shuffle(leaves)
    return leaves


def balanced_lengths(k):
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    return [m - 1] * short + [m] * (k - short)


def spread(nsym, symbols, lengths):
    out = [0] * nsym
    for s, n in zip(symbols, lengths):
        out[s] = n
    return out


def rle_lengths(seq, rng=None):
    """the code length alphabet's symbols for a list of lengths: [(0..15,) | (16, n) | (17, n) | (18, n)], n the repeat
    count.  Without rng greedy; with rng every legal choice is taken at random (repeats split, literals instead of repeats,
    runs that cross from the literal to the distance lengths -- the list is one list)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and (rng is None or rng.rand() < 0.85):
            r = min(run, 138) if rng is None else int(rng.randint(3, min(run, 138) + 1))
            out.append((18, r) if r >= 11 else (17, r))
            i += r
        elif i > 0 and seq[i - 1] == v and run >= 3 and (rng is None or rng.rand() < 0.85):
            r = min(run, 6) if rng is None else int(rng.randint(3, min(run, 6) + 1))
            out.append((16, r))
            i += r
        else:
            out.append((v,))
            i += 1
    return out


# --------------------------------------------------------------------------- the bit writer and the stream

class Coverage:
    def __init__(self):
        self.len_syms = set()        # (symbol, 'zero' | 'one' | 'mid' | 'none') of the extra bits
        self.dist_syms = set()
        self.lit_code_lens = set()   # lengths of literal codes written (dynamic blocks)
        self.len_code_lens = set()   # of length / end-of-block codes
        self.dist_code_lens = set()
        self.matches = set()         # (length, distance) of interest: distance >= NEAR - 1 or overlapping
        self.stored_at = set()       # bit offset (0 - 7) of a stored block's header
        self.stored_lens = set()
        self.nlit = set()
        self.ndist = set()
        self.cl_syms = set()         # (symbol, repeat) written in dynamic headers
        self.block_types = {0: 0, 1: 0, 2: 0}
        self.inflated = 0


def _extra_kind(ext, val):
    if ext == 0:
        return "none"
    return "zero" if val == 0 else ("one" if val == (1 << ext) - 1 else "mid")


class Stream:
    """One zlib stream being written.  Bits go LSB first into a Python int that is drained to bytes as it grows; Huffman
    codes are stored bit-reversed so that they go out most significant bit first."""

    def __init__(self, cinfo=7, cov=None):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0
        self.out = bytearray()                     # the expected bytes
        self.cov = cov
        self.lit = self.dist = None                # (lengths, reversed codes) of the open block
        cmf = (cinfo << 4) | 8
        flg = 2 << 6
        flg += 31 - ((cmf << 8) | flg) % 31
        self.bits(cmf, 8)
        self.bits(flg & 0xff, 8)

    # ---- bits
    def bits(self, v, n):
        assert 0 <= v < (1 << n)
        self.acc |= v << self.n
        self.n += n
        if self.n >= 512:
            self._drain()

    def _drain(self):
        k = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def align(self):
        self.bits(0, -self.bitpos & 7)

    def raw(self, data):
        assert self.bitpos & 7 == 0
        self._drain()
        self.buf += data

    # ---- blocks
    def stored(self, data, final=False, length=None, nlength=None, body=True):
        """a stored block at the current bit position; length / nlength: what the two words say, when not the truth"""
        assert len(data) <= 65535
        if self.cov:
            self.cov.stored_at.add(self.bitpos & 7)
            self.cov.stored_lens.add(len(data))
            self.cov.block_types[0] += 1
        self.bits(int(final), 1)
        self.bits(0, 2)
        self.align()
        ln = len(data) if length is None else length
        self.bits(ln, 16)
        self.bits((ln ^ 0xffff) if nlength is None else nlength, 16)
        if body:
            self.raw(bytes(data))
            self.out += data

    def begin_fixed(self, final=False):
        if self.cov:
            self.cov.block_types[1] += 1
        self.bits(int(final), 1)
        self.bits(1, 2)
        self.lit = (FIXED_LIT, rev_codes(FIXED_LIT))
        self.dist = (FIXED_DIST, rev_codes(FIXED_DIST))
        self.dynamic = False

    def begin_dynamic(self, lit_lens, dist_lens, final=False, cl_syms=None, cl_lens=None, hlit=None, hdist=None, hclen=None,
                      rng=None, btype=2):
        """a dynamic block's header.  cl_syms: the code length alphabet's symbols for lit_lens + dist_lens (see
        rle_lengths; anything may be written, e.g. (16, 3) first); cl_lens: the 19 lengths of that alphabet's own code
        (default: a complete code over the symbols used, random with rng); hlit / hdist / hclen: the header's counts when
        they are not to be len(lit_lens) - 257, len(dist_lens) - 1 and the minimum"""
        if self.cov:
            self.cov.block_types[2] += 1
            self.cov.nlit.add(len(lit_lens))
            self.cov.ndist.add(len(dist_lens))
        seq = list(lit_lens) + list(dist_lens)
        if cl_syms is None:
            cl_syms = rle_lengths(seq, rng)
        if cl_lens is None:
            used = sorted({t[0] for t in cl_syms})
            extra = [s for s in range(19) if s not in used]
            if rng is not None:
                rng.shuffle(extra)
                used += extra[:int(rng.randint(0, 4))]
            if len(used) < 2:
                used.append(extra[-1])
            lens = complete_lengths(rng, len(used), 7, 7 if rng.rand() < 0.3 and len(used) > 7 else 0) if rng is not None \
                else balanced_lengths(len(used))
            cl_lens = spread(19, used, lens)
        assert len(cl_lens) == 19 and max(cl_lens) <= 7
        ncl = max([4] + [k + 1 for k in range(19) if cl_lens[CLORDER[k]]]) if hclen is None else hclen
        self.bits(int(final), 1)
        self.bits(btype, 2)
        self.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
        self.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
        self.bits(ncl - 4, 4)
        for k in range(ncl):
            self.bits(cl_lens[CLORDER[k]], 3)
        cl_rev = rev_codes(cl_lens)
        for t in cl_syms:
            s = t[0]
            assert cl_lens[s], "code length symbol %d has no code" % s
            self.bits(cl_rev[s], cl_lens[s])
            if s == 16:
                self.bits(t[1] - 3, 2)
            elif s == 17:
                self.bits(t[1] - 3, 3)
            elif s == 18:
                self.bits(t[1] - 11, 7)
            if self.cov:
                self.cov.cl_syms.add((s, t[1] if s >= 16 else 1))
        self.lit = (list(lit_lens), rev_codes(lit_lens))
        self.dist = (list(dist_lens), rev_codes(dist_lens))
        self.dynamic = True

    def symbol(self, s):
        """one literal / length code, whatever it means"""
        assert self.lit[0][s]
        self.bits(self.lit[1][s], self.lit[0][s])

    def dsymbol(self, s):
        assert self.dist[0][s]
        self.bits(self.dist[1][s], self.dist[0][s])

    def put(self, tokens, model=True):
        """the tokens' codes; model=False: written only, not expanded into the expected bytes (a match that reaches in
        front of the stream has none)"""
        llen, lrev = self.lit
        dlen, drev = self.dist
        cov = self.cov
        acc, n = self.acc, self.n
        for t in tokens:
            if t[0] == "lit":
                b = t[1]
                assert llen[b], "literal %d has no code" % b
                acc |= lrev[b] << n
                n += llen[b]
                if cov and self.dynamic:
                    cov.lit_code_lens.add(llen[b])
            else:
                ln, d = t[1], t[2]
                s, e, v = length_symbol(ln, len(t) > 3 and t[3])
                ds, de, dv = dist_symbol(d)
                assert llen[s] and dlen[ds], "match (%d, %d) has no code" % (ln, d)
                acc |= lrev[s] << n
                n += llen[s]
                acc |= v << n
                n += e
                acc |= drev[ds] << n
                n += dlen[ds]
                acc |= dv << n
                n += de
                if cov:
                    cov.len_syms.add((s, _extra_kind(e, v)))
                    cov.dist_syms.add((ds, _extra_kind(de, dv)))
                    if self.dynamic:
                        cov.len_code_lens.add(llen[s])
                        cov.dist_code_lens.add(dlen[ds])
                    if d >= NEAR - 1 or d < ln:
                        cov.matches.add((ln, d))
            if n >= 512:
                k = n >> 3
                self.buf += (acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
                acc >>= 8 * k
                n -= 8 * k
        self.acc, self.n = acc, n
        if model:
            expand(tokens, self.out)

    def end_block(self):
        self.symbol(256)
        if self.cov and self.dynamic:
            self.cov.len_code_lens.add(self.lit[0][256])

    def fixed(self, tokens, final=False, model=True):
        self.begin_fixed(final)
        self.put(tokens, model)
        self.end_block()

    def dynamic_block(self, tokens, lit_lens, dist_lens, final=False, model=True, **kw):
        self.begin_dynamic(lit_lens, dist_lens, final, **kw)
        self.put(tokens, model)
        self.end_block()

    def finish(self, adler_xor=0):
        self.align()
        self._drain()
        if self.cov:
            self.cov.inflated += len(self.out)
        return bytes(self.buf) + ((zlib.adler32(bytes(self.out)) ^ adler_xor) & 0xffffffff).to_bytes(4, "big")


# --------------------------------------------------------------------------- codes for a set of tokens

def symbols_of(tokens):
    ls, ds = {256}, set()
    for t in tokens:
        if t[0] == "lit":
            ls.add(t[1])
        else:
            ls.add(length_symbol(t[1], len(t) > 3 and t[3])[0])
            ds.add(dist_symbol(t[2])[0])
    return ls, ds


def codes_for(rng, tokens, deep_lit=0, deep_dist=0, nlit=None, ndist=None, extra_lit=0, extra_dist=0):
    """random complete literal / length and distance length sets that cover the tokens; deep_*: force a code of that
    length; extra_*: that many more symbols get codes (more still where the forced depth needs them)"""
    ls, ds = symbols_of(tokens)
    ls, ds = sorted(ls), sorted(ds)

    def grow(used, limit, want):
        rest = [s for s in range(limit) if s not in used]
        rng.shuffle(rest)
        return sorted(used + rest[:max(0, want - len(used))])
    ls = grow(ls, nlit or 286, max(2, deep_lit + 1, len(ls) + extra_lit))
    lit = spread(max(257, ls[-1] + 1) if nlit is None else nlit, ls, complete_lengths(rng, len(ls), 15, deep_lit))
    if not ds and not deep_dist and not extra_dist:
        dist = [[0], [1], [0, 0, 0]][int(rng.randint(3))]        # no code at all / one code nobody uses
    elif len(ds) == 1 and not deep_dist and not extra_dist and rng.rand() < 0.5:
        dist = spread(ds[0] + 1, ds, [1])                         # the one incomplete set zlib accepts
    else:
        ds = grow(ds, ndist or 30, max(2, deep_dist + 1, len(ds) + extra_dist))
        dist = spread(ds[-1] + 1 if ndist is None else ndist, ds, complete_lengths(rng, len(ds), 15, deep_dist))
    if ndist is not None and len(dist) < ndist:
        dist += [0] * (ndist - len(dist))
    return lit, dist


# --------------------------------------------------------------------------- the valid catalogue: named cases

def _rand_bytes(rng, n):
    return rng.bytes(n) if n else b""


def _shift_to(s, off):
    """fixed blocks until the next block's header starts at bit `off` of a byte: an empty one is 10 bits, one with a 9-bit
    literal 19"""
    while s.bitpos & 7 != off:
        s.fixed(lits(b"\xf0") if (off - s.bitpos) & 1 else [])


def _named_valid(cov):
    cases = []
    rng = np.random.RandomState(1951)

    def done(name, s):
        cases.append((name, s.finish(), bytes(s.out)))

    # ---- distance codes longer than DB = 8 bits: a chain 1, 2, ... 15, 15 over 16 symbols, every length used, short
    # literal codes in between (so the long walk starts at every bit offset); and 30 symbols with a forced 15
    for variant in range(3):
        s = Stream(cov=cov)
        s.stored(_rand_bytes(rng, 300))
        chain = list(range(1, 16)) + [15]
        if variant:
            rng.shuffle(chain)
        toks = []
        for k in range(3):
            for ds in range(16):                   # (distances up to 255)
                d = DBASE[ds] + int(rng.randint(1 << DEXT[ds]))
                toks += lits(_rand_bytes(rng, int(rng.randint(0, 4)))) + [("match", int(rng.randint(3, 259)), d)]
        lit, _ = codes_for(rng, toks)
        s.dynamic_block(toks, lit, chain, final=True, rng=rng)
        done("dist_codes_chain_1_to_15_v%d" % variant, s)
    s = Stream(cov=cov)
    s.stored(_rand_bytes(rng, 33000))
    toks = []
    for ds in list(range(30)) * 2:
        toks += lits(_rand_bytes(rng, 2)) + [("match", int(rng.randint(3, 259)), DBASE[ds] + int(rng.randint(1 << DEXT[ds])))]
    lit, dist = codes_for(rng, toks, deep_dist=15, deep_lit=15, extra_lit=40)
    s.dynamic_block(toks, lit, dist, final=True, rng=rng)
    done("dist_codes_30_symbols_deep_15", s)

    # ---- literal / length codes of 11 to 15 bits; all 286 symbols with the full 15 bits
    for name, nsym, deep in (("lit_codes_deep_11", 120, 11), ("lit_codes_deep_13", 200, 13), ("lit_codes_286_deep_15", 286, 15),
                             ("lit_codes_286_deep_15_b", 286, 15)):
        s = Stream(cov=cov)
        syms = list(range(286))
        rng.shuffle(syms)
        syms = sorted(set(syms[:nsym]) | {256})
        lens = complete_lengths(rng, len(syms), 15, deep)
        lit = spread(286 if nsym == 286 else max(257, syms[-1] + 1), syms, lens)
        toks = lits([x for x in syms if x < 256][:8])
        for rep in range(3):
            for sym in syms:                       # every symbol that has a code, hence every code length of the set
                if sym < 256:
                    toks.append(("lit", sym))
                elif sym > 256:
                    k = sym - 257
                    toks.append(("match", LBASE[k] + int(rng.randint(1 << LEXT[k])), int(rng.randint(1, 9))))
        _, dist = codes_for(rng, toks, deep_dist=9)
        s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done(name, s)

    # ---- the seams of the ring: NEAR and NEAR + 1 with length 258, behind 0 / 1 / 1023 / 1024 / 1025 literals, with the
    # match's destination (body 4096) or its source (body NEAR + 1024) on a flush boundary; 32768 at 32768; distance == position
    for pre in (0, 1, 1023, 1024, 1025):
        for body in (4096, NEAR + FLUSH):
            for d in (NEAR, NEAR + 1):
                s = Stream(cov=cov)
                s.fixed(lits(_rand_bytes(rng, pre)))
                s.stored(_rand_bytes(rng, body))
                toks = [("match", 258, d), ("lit", 7), ("match", 258, d), ("match", 258, 2 * NEAR + 1 - d), ("lit", 9)]
                lit, dist = codes_for(rng, toks, deep_dist=12, deep_lit=11)
                s.dynamic_block(toks, lit, dist, final=True, rng=rng)
                done("seam_ring_d%d_body%d_pre%d" % (d, body, pre), s)
        s = Stream(cov=cov)
        s.fixed(lits(_rand_bytes(rng, pre)))
        s.stored(_rand_bytes(rng, 32768))
        toks = [("match", 258, 32768), ("match", 258, 32768), ("lit", 1), ("match", 3, 32768), ("match", 258, 32767)]
        s.fixed(toks, final=True)
        done("seam_far_d32768_pre%d" % pre, s)
    for p in (1, 2, 257, 258, NEAR - 1, NEAR, NEAR + 1, 4095, 4096, 4097, 32767, 32768):
        s = Stream(cov=cov)
        s.stored(_rand_bytes(rng, p))
        toks = [("match", 258, p)]
        lit, dist = codes_for(rng, toks, deep_dist=10)
        s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done("seam_dist_equals_position_%d" % p, s)

    # ---- overlapping matches: i mod dist
    for d in (1, 2, 3, 63, 64, 65, 257):
        s = Stream(cov=cov)
        s.fixed(lits(_rand_bytes(rng, 300)))
        toks = []
        for ln in (3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 194, 257, 258):
            if ln > d:
                toks += [("match", ln, d), ("lit", ln & 255)]
        lit, dist = codes_for(rng, toks)
        s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done("overlap_dist_%d" % d, s)

    # ---- every length symbol and every distance symbol, extra bits all zero and all one (and 258 as 284 + 31)
    for kind in ("fixed", "dynamic"):
        s = Stream(cov=cov)
        s.stored(_rand_bytes(rng, 32768))
        toks = []
        for ones in (0, 1):
            for k in range(30):
                lk, dk = k % 29, k % 30
                ln = LBASE[lk] + (((1 << LEXT[lk]) - 1) if ones else 0)
                d = DBASE[dk] + (((1 << DEXT[dk]) - 1) if ones else 0)
                toks += [("match", ln, d, lk == 27), ("lit", k)]
        toks += [("match", 258, 1), ("match", 258, 32768, True)]
        if kind == "fixed":
            s.fixed(toks, final=True)
        else:
            lit, dist = codes_for(rng, toks, deep_lit=14, deep_dist=13, extra_lit=30)
            s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done("every_length_and_distance_symbol_%s" % kind, s)

    # ---- the literal-run path: 1-bit and 2-bit literal codes (more than RUN symbols in a 64-bit window)
    s = Stream(cov=cov)
    lit = spread(257, [97, 98, 256], [1, 2, 2])
    toks = [("lit", 97 + int(x)) for x in (rng.rand(9000) < 0.15)]
    s.dynamic_block(toks, lit, [0], final=True)
    done("run_1bit_literals", s)
    s = Stream(cov=cov)
    lit = spread(258, [0, 255, 256, 257], [2, 2, 2, 2])
    toks = []
    for k in range(400):
        toks += [("lit", 255 * int(x)) for x in rng.randint(0, 2, size=int(rng.randint(0, 70)))] + [("match", 3, 1)]
    toks = toks[next(i for i, t in enumerate(toks) if t[0] == "lit"):]
    s.dynamic_block(toks, lit, [1], final=True)                    # (and a single 1-bit distance code)
    done("run_2bit_literals_and_matches", s)
    # a run of k short literals that ends at a match / the end of the block / a literal of more than LB bits / nothing
    # (the window's end: more short literals), for every k around RUN and around a 64-bit window
    short = [10, 20, 30, 40, 50, 60]
    for deep in (11, 12, 15):
        # six 3-bit literals, and under the code space's last quarter a complete set of deep + 3 more codes, up to deep bits
        syms = short + list(range(100, 100 + deep)) + [256, 257, 258]
        s = Stream(cov=cov)
        for attempt in range(200):
            lit = spread(259, syms, [3] * 6 + [2 + x for x in complete_lengths(rng, deep + 3, 13, deep - 2)])
            longs = [x for x in range(100, 100 + deep) if lit[x] > LB]
            if longs and max(lit[256], lit[257], lit[258]) <= LB:
                break
        assert longs and max(lit[256], lit[257], lit[258]) <= LB and kraft(lit) == 1 << 15
        s.begin_dynamic(lit, [1, 1], rng=rng)
        s.put(lits(b"\x0a\x14"))
        for k in list(range(0, 24)) + [31, 32, 33, 40, 63, 64, 65]:
            for ender in ("match", "long", "short"):
                s.put([("lit", short[int(x)]) for x in rng.randint(0, 6, size=k)])
                if ender == "match":
                    s.put([("match", 3 + int(rng.randint(2)), 1 + int(rng.randint(2)))])
                elif ender == "long":
                    s.put([("lit", longs[int(rng.randint(len(longs)))])])
        s.end_block()
        for k in (0, 1, 15, 16, 17, 21):                           # ... and at the end of a block
            s.begin_dynamic(lit, [1, 1], rng=rng)
            s.put([("lit", short[int(x)]) for x in rng.randint(0, 6, size=k)])
            s.end_block()
        s.fixed([], final=True)
        done("run_enders_deep_%d" % deep, s)
    # a run that ends exactly where the input window moves on: the stream sits at any byte offset, so for each of the four
    # alignments of its first byte (lead) the 1-bit literals stop at the 256-byte seam, and one bit either side of it
    for lead in range(4):
        for delta in (-1, 0, 1):
            for ender in ("match", "literals"):
                s = Stream(cov=cov)
                lit = spread(258, [65, 66, 256, 257], [1, 2, 3, 3])
                s.begin_dynamic(lit, [1], final=True)
                s.put([("lit", 66)])
                for seam in (1, 2, 3):
                    target = (CHUNK_BYTES * seam - lead) * 8 + delta
                    while s.bitpos < target:
                        s.put([("lit", 65)])
                    s.put([("match", 3, 1)] if ender == "match" else [("lit", 66)] * 3)
                s.end_block()
                done("run_ends_at_input_seam_lead%d_%+d_%s" % (lead, delta, ender), s)

    # ---- the code length encoding
    s = Stream(cov=cov)                         # 16 carries a length from the literal lengths into the distance lengths
    lit = spread(257, [10, 11, 254, 255, 256], [3, 3, 2, 2, 2])
    cl = [(17, 10), (3,), (3,), (18, 138), (18, 104), (2,), (16, 5), (2,)]
    #      0 - 9     10    11    12 - 149   150 - 253  254   255, 256, distance 0, 1, 2    3
    s.begin_dynamic(lit, [2, 2, 2, 2], cl_syms=cl)
    s.put(lits(bytes([10, 11, 254, 255, 254, 10])))
    s.end_block()
    s.stored(b"0123456789")
    lit2 = spread(258, [48, 49, 256, 257], [2, 2, 2, 2])
    s.begin_dynamic(lit2, [2, 2, 2, 2], final=True, cl_syms=[(18, 48), (2,), (2,), (18, 138), (18, 68), (2,), (16, 5)])
    #                                                        0 - 47    48    49    50 - 187   188 - 255  256   257, d0 - d3
    s.put([("lit", 48), ("match", 3, 1), ("match", 3, 2), ("match", 3, 3), ("match", 3, 4), ("lit", 49)])
    s.end_block()
    done("cl_repeat_16_across_the_literal_distance_boundary", s)
    s = Stream(cov=cov)                         # 18 with 138 zeros, first; 17 / 18 runs that end exactly at nlit + ndist
    lit = spread(258, [138, 139, 256, 257], [2, 2, 2, 2])
    head = [(18, 138), (2,), (2,), (18, 116), (2,), (2,)]          # 0 - 137, 138, 139, 140 - 255, 256, 257
    s.begin_dynamic(lit, [1, 1, 0, 0, 0], cl_syms=head + [(1,), (1,), (17, 3)])
    s.put(lits(bytes([138, 139, 138])) + [("match", 3, 2)])
    s.end_block()
    s.begin_dynamic(lit, [1, 1] + [0] * 11, cl_syms=head + [(1,), (1,), (18, 11)])
    s.put([("match", 3, 1)])
    s.end_block()
    s.begin_dynamic(lit, [1, 1] + [0] * 28, cl_syms=head + [(1,), (1,), (17, 10), (18, 18)])
    s.put([("match", 3, 2)])
    s.end_block()
    s.begin_dynamic(lit, [0] * 29 + [1], final=True, cl_syms=head + [(18, 29), (1,)])
    s.end_block()
    done("cl_18_with_138_zeros_and_runs_that_end_at_the_end", s)
    for nlit, ndist in ((286, 30), (286, 1), (257, 30)):            # HLIT 29 and HDIST 29: the most the header may say
        s = Stream(cov=cov)
        s.stored(_rand_bytes(rng, 25000))
        toks = ([("match", 258, 24577 if ndist == 30 else 1)] if nlit == 286 else []) + [("lit", 3)]
        lit, dist = codes_for(rng, toks, nlit=nlit, ndist=ndist, extra_lit=5, extra_dist=30 if ndist == 30 else 0)
        s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done("cl_hlit_%d_hdist_%d" % (nlit - 257, ndist - 1), s)
    s = Stream(cov=cov)                         # one distance code of length 0: a block of literals
    toks = lits(b"no distance code at all")
    lit, _ = codes_for(rng, toks)
    s.dynamic_block(toks, lit, [0], final=True, rng=rng)
    done("dynamic_one_distance_code_of_length_0", s)
    s = Stream(cov=cov)                         # a single 1-bit distance code: the incomplete set zlib accepts
    toks = lits(b"ab") + [("match", 200, 1), ("lit", 99), ("match", 3, 1)]
    lit, _ = codes_for(rng, toks)
    s.dynamic_block(toks, lit, [1], rng=rng)
    toks = lits(b"cd") + [("match", 17, 25), ("match", 258, 32)]
    lit, _ = codes_for(rng, toks)
    s.dynamic_block(toks, lit, [0, 0, 0, 0, 0, 0, 0, 0, 0, 1], final=True, rng=rng)      # (distance symbol 9: 25 - 32)
    done("dynamic_single_1bit_distance_code", s)
    s = Stream(cov=cov)                         # ... and a single 1-bit literal / length code: the end of the block
    s.fixed(lits(b"x"))
    s.dynamic_block([], spread(257, [256], [1]), [0])
    s.dynamic_block([], spread(257, [256], [1]), [1], final=True)
    done("dynamic_single_1bit_end_of_block_code", s)

    # ---- stored blocks: the lengths, the header at every bit offset, matches that reach back into stored data
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 65535):
        s = Stream(cov=cov)
        s.stored(_rand_bytes(rng, n), final=True)
        done("stored_%d" % n, s)
    s = Stream(cov=cov)
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 0, 0, 5):
        s.stored(_rand_bytes(rng, n))
    s.stored(b"", final=True)
    done("stored_lengths_in_a_row", s)
    for off in range(8):
        s = Stream(cov=cov)
        _shift_to(s, off)
        s.stored(_rand_bytes(rng, 700 + off))
        _shift_to(s, (off + 3) & 7)
        s.stored(_rand_bytes(rng, 5000))
        toks = [("match", 258, 100), ("match", 258, NEAR), ("match", 258, NEAR + 1), ("match", 100, 5700)]
        lit, dist = codes_for(rng, toks, deep_dist=11)
        s.dynamic_block(toks, lit, dist, final=True, rng=rng)
        done("stored_header_at_bit_%d_then_matches_into_it" % off, s)

    # ---- empty blocks
    s = Stream(cov=cov)
    for k in range(9):
        s.fixed([])
    s.fixed([], final=True)
    done("empty_fixed_blocks", s)
    s = Stream(cov=cov)
    lit, dist = codes_for(rng, [], extra_lit=20, extra_dist=7)
    for k in range(5):
        s.dynamic_block([], lit, dist, rng=rng)
        s.fixed([])
        s.stored(b"")
    s.fixed(lits(b"between"))
    s.dynamic_block([], lit, dist, final=True, rng=rng)
    done("empty_dynamic_fixed_and_stored_blocks", s)

    # ---- Adler-32 where its sums are largest, as stored blocks only
    for name, data in (("ff", b"\xff" * 70000), ("ff00", b"\xff\x00" * 35000)):
        s = Stream(cov=cov)
        for i in range(0, 70000, 65535):
            s.stored(data[i:i + 65535], final=i + 65535 >= 70000)
        done("adler_%s_70000_stored" % name, s)
    for cinfo in (0, 3, 7):                                          # the header's window size is of no consequence
        s = Stream(cinfo=cinfo, cov=cov)
        s.fixed(lits(b"abc") + [("match", 30, 3)], final=True)
        done("cinfo_%d" % cinfo, s)
    return cases


# --------------------------------------------------------------------------- the valid catalogue: the differential set

_EDGE_LENS = (3, 4, 10, 11, 12, 63, 64, 65, 127, 128, 129, 191, 192, 193, 227, 257, 258)
_EDGE_DISTS = (1, 2, 3, 4, 63, 64, 65, 256, 257, 1023, 1024, 1025, NEAR - 1, NEAR, NEAR + 1, 4095, 4096, 4097, 8192, 16384,
               24576, 24577, 32767, 32768)


def random_tokens(rng, size):
    """tokens that inflate to about `size` bytes: literal runs over alphabets of 2 to 256 bytes, near, far and overlapping
    matches, the kernel's seam distances among them"""
    toks, pos = [], 0
    alpha = np.frombuffer(rng.bytes(int(rng.choice([2, 3, 5, 16, 64, 256]))), dtype=np.uint8)
    big = size > 20000
    while pos < size:
        if pos == 0 or rng.rand() < (0.3 if big else 0.5):
            n = int(rng.randint(1, 300)) if rng.rand() < 0.1 else int(rng.randint(1, 30))
            toks += [("lit", int(b)) for b in alpha[rng.randint(0, alpha.size, size=n)]]
            pos += n
            continue
        r = rng.rand()
        if r < 0.3:
            ln = int(_EDGE_LENS[rng.randint(len(_EDGE_LENS))])
        else:
            ln = int(rng.randint(3, 259)) if r < 0.7 or big else int(rng.randint(3, 20))
        r = rng.rand()
        if r < 0.25:
            d = int(_EDGE_DISTS[rng.randint(len(_EDGE_DISTS))])
        elif r < 0.45:
            d = int(rng.randint(1, ln + 1))                       # overlapping
        elif r < 0.75:
            d = int(rng.randint(1, NEAR + 2))
        elif r < 0.95:
            d = int(rng.randint(NEAR, 32769))
        else:
            d = pos
        d = min(max(d, 1), pos, 32768)
        toks.append(("match", ln, d))
        pos += ln
    return toks


def random_stream(rng, size, cov=None):
    toks = random_tokens(rng, size) if size else []
    s = Stream(cinfo=int(rng.randint(0, 8)), cov=cov)
    i, n = 0, len(toks)
    nblocks = int(rng.randint(1, 7))
    while True:
        k = n - i if nblocks <= 1 else (0 if rng.rand() < 0.1 else int(rng.randint(0, n - i + 1)))
        seg = toks[i:i + k]
        i += k
        nblocks -= 1
        final = i >= n and nblocks <= 0
        kind = rng.rand()
        if kind < 0.2:
            at = len(s.out)
            data = bytes(expand(seg, bytearray(s.out))[at:])
            parts = [data[j:j + 65535] for j in range(0, len(data), 65535)] or [b""]
            for j, p in enumerate(parts):
                s.stored(p, final=final and j == len(parts) - 1)
        elif kind < 0.4:
            s.fixed(seg, final=final)
        else:
            r = rng.rand()
            lit, dist = codes_for(rng, seg, deep_lit=int(rng.randint(11, 16)) if r < 0.5 else 0,
                                  deep_dist=int(rng.randint(9, 16)) if 0.25 < r < 0.75 else 0,
                                  extra_lit=int(rng.randint(0, 40)) if rng.rand() < 0.5 else 0,
                                  extra_dist=int(rng.randint(0, 6)) if rng.rand() < 0.3 else 0)
            s.dynamic_block(seg, lit, dist, final=final, rng=rng)
        if final:
            break
    return s.finish(), bytes(s.out)


def _random_valid(cov):
    rng = np.random.RandomState(19510)
    sizes = [0, 0, 1, 2, 3]
    for lo, hi, count in ((1, 300, 60), (300, 6000, 120), (6000, 40000, 12), (40000, 100000, 12)):
        sizes += [int(x) for x in rng.randint(lo, hi, size=count)]
    out = []
    for k, size in enumerate(sizes):
        stream, want = random_stream(rng, size, cov)
        out.append(("random_%03d_%d" % (k, len(want)), stream, want))
    return out


def lead_of(name):
    """the alignment (address % 4) of its first byte that a run_ends_at_input_seam_* stream is built for, else None"""
    k = name.find("_seam_lead")
    return int(name[k + 10]) if k >= 0 else None


_VALID = None


def _build_valid():
    global _VALID
    if _VALID is None:
        cov = Coverage()
        _VALID = (_named_valid(cov) + _random_valid(cov), cov)
    return _VALID


def valid_streams():
    return list(_build_valid()[0])


def coverage():
    return _build_valid()[1]


# --------------------------------------------------------------------------- given bytes as a crafted stream

def tokenize(data, start, end, index):
    """greedy LZ77 over data[start:end]; index: {three bytes: their last position}, kept up to date on the way (index_span
    does that for bytes that go out some other way)"""
    toks, i = [], start
    while i < end:
        key = data[i:i + 3]
        j = index.get(key)
        if j is not None and i + 3 <= end and i - j <= 32768:
            n = 3
            while n < 258 and i + n < end and data[j + n] == data[i + n]:
                n += 1
            toks.append(("match", n, i - j))
            index_span(data, i, i + n, index)
            i += n
        else:
            toks.append(("lit", data[i]))
            index[key] = i
            i += 1
    return toks


def index_span(data, a, b, index):
    for k in range(a, b):
        index[data[k:k + 3]] = k


def recode(rng, data):
    """the bytes as a zlib stream no compressor writes: a dynamic block with literal codes of 13 and distance codes of 12
    bits, stored blocks for the middle, a fixed block, an empty block, and a last dynamic block with 15-bit codes whose
    matches reach back into the stored bytes"""
    n = len(data)
    a = min(n, 600)
    b = max(a, n - 1200)
    c = max(b, n - 800)
    s, index = Stream(cinfo=int(rng.randint(0, 8))), {}
    toks = tokenize(data, 0, a, index)
    lit, dist = codes_for(rng, toks, deep_lit=13, deep_dist=12, extra_lit=20)
    s.dynamic_block(toks, lit, dist, rng=rng)
    for i in range(a, b, 65535):
        s.stored(data[i:min(b, i + 65535)])
    index_span(data, a, b, index)
    s.fixed(tokenize(data, b, c, index))
    s.fixed([])
    toks = tokenize(data, c, n, index)
    lit, dist = codes_for(rng, toks, deep_lit=15, deep_dist=15, extra_lit=40)
    s.dynamic_block(toks, lit, dist, final=True, rng=rng)
    assert bytes(s.out) == bytes(data)
    return s.finish()


# --------------------------------------------------------------------------- the invalid catalogue

def invalid_streams():
    """(name, stream, sgk_inflate status, fragment of zlib's message); every stream has exactly one fault"""
    rng = np.random.RandomState(1950)
    out = []
    LITSET, DISTSET, CLSET = "invalid literal/lengths set", "invalid distances set", "invalid code lengths set"
    TRUNC = "incomplete or truncated stream"
    ab = spread(257, [97, 98, 256], [1, 2, 2])                      # a complete little literal code

    def add(name, s, status, msg, cut=None, adler_xor=0):
        data = s.finish(adler_xor)
        out.append((name, data if cut is None else data[:cut], status, msg))

    # incomplete sets
    s = Stream(); s.dynamic_block(lits(b"aaa"), spread(257, [97, 256], [2, 2]), [0], final=True)
    add("incomplete_literal_set_two_2bit_codes", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"ab"), spread(257, [97, 98, 256], [1, 2, 3]), [0], final=True)
    add("incomplete_literal_set_1_2_3", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"a"), spread(257, [97, 256], [1, 15]), [0], final=True)
    add("incomplete_literal_set_1_15", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"aa"), spread(257, [97, 256], [2, 1]), [0], final=True)
    add("incomplete_literal_set_a_1bit_and_a_2bit_code", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"ab") + [("match", 3, 1)], spread(258, [97, 98, 256, 257], [2] * 4), [2, 2], final=True)
    add("incomplete_distance_set_two_2bit_codes", s, 3, DISTSET)
    s = Stream(); s.dynamic_block(lits(b"ab") + [("match", 3, 2)], spread(258, [97, 98, 256, 257], [2] * 4), [1, 2], final=True)
    add("incomplete_distance_set_1_2", s, 3, DISTSET)
    s = Stream(); s.dynamic_block(lits(b"ab") + [("match", 3, 1)], spread(258, [97, 98, 256, 257], [2] * 4), [2], final=True)
    add("incomplete_distance_set_one_2bit_code", s, 3, DISTSET)
    s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0], final=True, cl_lens=spread(19, [0, 1, 2, 18], [2, 2, 2, 3]))
    add("incomplete_code_length_code", s, 3, CLSET)
    s = Stream(); s.dynamic_block(lits(b"a"), spread(257, [97, 256], [1, 1]), [0], final=True,
                                  cl_lens=spread(19, [0, 1, 18], [2, 2, 2]),
                                  cl_syms=[(18, 97), (1,), (18, 138), (18, 20), (1,), (0,)])
    add("incomplete_code_length_code_three_2bit_codes", s, 3, CLSET)
    s = Stream(); s.dynamic_block(lits(b"a"), spread(257, [97, 256], [1, 1]), [0], final=True,
                                  cl_lens=spread(19, [1], [1]),
                                  cl_syms=[(1,)] * 258)
    add("incomplete_code_length_code_single_1bit_code", s, 3, CLSET)
    # over-subscribed sets
    s = Stream(); s.dynamic_block(lits(b"ab"), spread(257, [97, 98, 256], [1, 1, 1]), [0], final=True)
    add("oversubscribed_literal_set", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"ab"), spread(257, [97, 98, 99, 256], [1, 2, 2, 15]), [0], final=True)
    add("oversubscribed_literal_set_by_one_15bit_code", s, 3, LITSET)
    s = Stream(); s.dynamic_block(lits(b"ab"), ab, [1, 1, 1], final=True)
    add("oversubscribed_distance_set", s, 3, DISTSET)
    s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0], final=True, cl_lens=spread(19, [0, 1, 2, 18], [1, 2, 2, 2]))
    add("oversubscribed_code_length_code", s, 3, CLSET)
    # the header's counts
    many = "too many length or distance symbols"
    for hlit in (30, 31):
        s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0], final=True, hlit=hlit)
        add("hlit_%d" % hlit, s, 3, many)
    for hdist in (30, 31):
        s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0], final=True, hdist=hdist)
        add("hdist_%d" % hdist, s, 3, many)
    # the code length symbols
    rep = "invalid bit length repeat"
    s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0], final=True,
                                  cl_lens=spread(19, [0, 1, 2, 16, 18], [2, 2, 2, 3, 3]),
                                  cl_syms=[(16, 3)] + rle_lengths(ab + [0]))
    add("repeat_16_first", s, 3, rep)
    tail = rle_lengths(ab[:256])                                    # symbols 0 - 255; then 256 and nd distance lengths
    for name, nd, last in (("repeat_16_one_past_the_end", 2, [(2,), (16, 3)]),
                           ("repeat_17_one_past_the_end", 3, [(2,), (0,), (17, 3)]),
                           ("repeat_18_one_past_the_end", 11, [(2,), (0,), (18, 11)]),
                           ("repeat_18_far_past_the_end", 30, [(2,), (18, 138)])):
        s = Stream(); s.dynamic_block(lits(b"ab"), ab, [0] * nd, final=True, cl_syms=tail + last)
        add(name, s, 3, rep)
    s = Stream(); s.begin_dynamic(spread(257, [97, 98], [1, 1]), [0], final=True); s.put(lits(b"ab"))
    add("no_end_of_block_code", s, 3, "invalid code -- missing end-of-block")
    # invalid codes
    s = Stream(); s.begin_dynamic(spread(258, [97, 98, 256, 257], [2] * 4), [1], final=True)
    s.put(lits(b"ab")); s.symbol(257); s.bits(1, 1); s.end_block()
    add("single_distance_code_other_bit", s, 4, "invalid distance code")
    for sym in (286, 287):
        s = Stream(); s.begin_fixed(final=True); s.put(lits(b"fixed")); s.symbol(sym); s.bits(0, 5); s.end_block()
        add("fixed_literal_length_symbol_%d" % sym, s, 4, "invalid literal/length code")
    for sym in (30, 31):
        s = Stream(); s.begin_fixed(final=True); s.put(lits(b"fixed")); s.symbol(257); s.dsymbol(sym); s.end_block()
        add("fixed_distance_symbol_%d" % sym, s, 4, "invalid distance code")
    s = Stream(); s.fixed(lits(b"before")); s.begin_dynamic(spread(257, [256], [1]), [0], final=True)
    s.bits(0x7fff, 15); s.bits(0, 17)
    add("pattern_no_code_owns_single_end_of_block_code", s, 4, "invalid literal/length code")
    s = Stream(); s.begin_dynamic(spread(258, [97, 256, 257], [1, 2, 2]), [1], final=True)
    s.put(lits(b"aaaa")); s.symbol(257); s.bits(0x7fff, 15); s.bits(0, 17)
    add("pattern_no_code_owns_single_distance_code_long", s, 4, "invalid distance code")
    # distances in front of the stream
    far = "invalid distance too far back"
    s = Stream(); s.fixed([("match", 3, 1)], final=True, model=False)
    add("distance_1_at_position_0", s, 5, far)
    for p, kind in ((1, "fixed"), (5, "fixed"), (NEAR, "dynamic"), (NEAR + 1, "dynamic"), (6000, "dynamic"),
                    (32767, "fixed")):
        s = Stream(); s.stored(_rand_bytes(rng, p))
        toks = [("match", 258, p + 1)]
        if kind == "fixed":
            s.fixed(toks, final=True, model=False)
        else:
            lit, dist = codes_for(rng, toks, deep_dist=10)
            s.dynamic_block(toks, lit, dist, final=True, model=False, rng=rng)
        add("distance_%d_at_position_%d" % (p + 1, p), s, 5, far)
    # blocks
    s = Stream(); s.stored(b"stored", final=True, nlength=(6 ^ 0xffff) ^ 0x0100)
    add("stored_len_nlen_mismatch", s, 2, "invalid stored block lengths")
    s = Stream(); s.fixed(lits(b"x")); s.stored(b"stored", final=True, length=7, nlength=6 ^ 0xffff)
    add("stored_len_nlen_mismatch_at_bit_offset", s, 2, "invalid stored block lengths")
    s = Stream(); s.bits(1, 1); s.bits(3, 2); s.bits(0, 29)
    add("block_type_3", s, 2, "invalid block type")
    s = Stream(); s.fixed(lits(b"x")); s.bits(0, 1); s.bits(3, 2); s.bits(0, 29)
    add("block_type_3_second_block", s, 2, "invalid block type")
    # truncations
    s = Stream(); s.stored(_rand_bytes(rng, 40), final=True, length=60)
    add("stored_length_past_the_input", s, 6, TRUNC, cut=-4)
    s = Stream(); s.stored(_rand_bytes(rng, 2000), final=True)
    add("stored_cut_in_the_data", s, 6, TRUNC, cut=1500)
    s = Stream(); s.fixed(lits(b"abcdef")); at = (s.bitpos + 3 + 7) // 8; s.stored(_rand_bytes(rng, 20), final=True)
    add("stored_cut_in_the_length_words", s, 6, TRUNC, cut=at + 3)
    toks = random_tokens(rng, 3000)
    lit, dist = codes_for(rng, toks, deep_lit=12, deep_dist=10, extra_lit=60)
    s = Stream(); s.fixed(lits(b"head")); s.dynamic_block(toks, lit, dist, final=True, rng=np.random.RandomState(3))
    whole = s.finish()
    probe = Stream(); probe.fixed(lits(b"head"))
    probe.begin_dynamic(lit, dist, final=True, rng=np.random.RandomState(3))
    hdr_end = probe.bitpos // 8
    for name, cut in (("cut_in_hlit_hdist_hclen", 9), ("cut_in_the_code_length_code_lengths", 12),
                      ("cut_in_the_code_lengths", (12 + hdr_end) // 2), ("cut_in_the_code_lengths_late", hdr_end - 2)):
        out.append(("dynamic_header_" + name, whole[:cut], 6, TRUNC))
    for name, cut in (("just_behind_the_header", hdr_end + 1), ("in_the_middle", (hdr_end + len(whole)) // 2),
                      ("last_byte", len(whole) - 5)):
        out.append(("dynamic_symbols_cut_" + name, whole[:cut], 6, TRUNC))
    s = Stream(); s.fixed(random_tokens(rng, 2500), final=True)
    fx = s.finish()
    out.append(("fixed_symbols_cut_in_the_middle", fx[:len(fx) // 2], 6, TRUNC))
    for k in (1, 2, 3, 4):
        out.append(("adler_word_cut_%d" % k, whole[:-k], 6, TRUNC))
    # the check value, wrong by one bit, on streams no compressor writes
    valid = {n: st for n, st, _ in valid_streams()}
    for n, bit in (("every_length_and_distance_symbol_dynamic", 0), ("run_enders_deep_15", 16),
                   ("seam_ring_d3838_body4096_pre1023", 31), ("adler_ff_70000_stored", 7), ("empty_fixed_blocks", 0)):
        st = valid[n]
        check = (int.from_bytes(st[-4:], "big") ^ (1 << bit)).to_bytes(4, "big")
        out.append(("adler_bit_%d_%s" % (bit, n), st[:-4] + check, 7, "incorrect data check"))
    return out
