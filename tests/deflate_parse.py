"""An independent judge of the zlib streams k_deflate and its model write (tests/test_deflate_edges_cpu.py on the model,
tests/test_gpu_deflate_edges.py on the kernel): a bit-by-bit RFC 1950 / 1951 reader that keeps everything it reads, the
tokenizer of the format as a literal loop, and the checks of what the format comment in csrc/deflate_kernels.hip states.
Plain loops over Python lists; nothing here comes from tools/proto, and the tables are RFC 1951's, not arithmetic."""
import heapq
import zlib

CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_EXTRA = {16: 2, 17: 3, 18: 7}


class FormatError(ValueError):
    """the stream is not what RFC 1950 / 1951 allow"""


class _Bits:
    def __init__(self, z: bytes):
        self.bits = []
        for byte in z:
            for k in range(8):
                self.bits.append((byte >> k) & 1)
        self.pos = 0

    def take(self, n: int) -> int:
        if self.pos + n > len(self.bits):
            raise FormatError("the stream ends inside a field")
        v = 0
        for k in range(n):
            v |= self.bits[self.pos + k] << k
        self.pos += n
        return v


def kraft(lens, maxbits: int) -> int:
    """sum of 2^(maxbits - length) over the used codes: 2^maxbits for a complete code"""
    return sum(1 << (maxbits - v) for v in lens if v)


def _decoder(lens, what: str, one_code_ok: bool = False):
    """canonical code -> {(length, code): symbol}; over-subscribed and incomplete codes are refused (a distance code of
    one single code may be incomplete, RFC 1951 3.2.7)"""
    used = [v for v in lens if v]
    if not used:
        if one_code_ok:
            return {}
        raise FormatError("%s: no code at all" % what)
    k = kraft(lens, 15)
    if k > 1 << 15:
        raise FormatError("%s: over-subscribed" % what)
    if k < 1 << 15 and not (one_code_ok and len(used) == 1 and used[0] == 1):
        raise FormatError("%s: incomplete" % what)
    count = [0] * 17
    for v in used:
        count[v] += 1
    nxt = [0] * 17
    code = 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, v in enumerate(lens):
        if v:
            table[(v, nxt[v])] = s
            nxt[v] += 1
    return table


def _symbol(bits: _Bits, table, what: str) -> int:
    code = n = 0
    while n < 15:
        code = (code << 1) | bits.take(1)
        n += 1
        s = table.get((n, code))
        if s is not None:
            return s
    raise FormatError("%s: no such code" % what)


def _tokens(bits: _Bits, lit, dist, out: bytearray):
    toks = []
    while True:
        s = _symbol(bits, lit, "literal/length")
        if s < 256:
            toks.append(("L", s))
            out.append(s)
        elif s == 256:
            return toks
        else:
            if s > 285:
                raise FormatError("length symbol %d" % s)
            ln = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
            if not dist:
                raise FormatError("a match in a block without distance codes")
            d = _symbol(bits, dist, "distance")
            if d > 29:
                raise FormatError("distance symbol %d" % d)
            d = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
            if d > len(out):
                raise FormatError("distance %d at output byte %d" % (d, len(out)))
            toks.append(("M", ln, d))
            for _ in range(ln):
                out.append(out[-d])


def parse(z: bytes):
    """-> dict: header (2 bytes), blocks (a list of dicts, see below), out (the inflated bytes), pad_bits (the bits between
    the last block and the check value, as an integer), adler (the check value as stored).  A block:
    type 'stored' / 'fixed' / 'dynamic', final, start and nbits (bit position in z, size), first and nbytes (its piece of
    out); stored: len, nlen, pad_zero; dynamic: hlit, hdist, hclen (the fields), cllens (19, by symbol), items
    [(code length symbol, extra value)], litlens, distlens; fixed and dynamic: tokens [('L', byte) | ('M', len, dist)]."""
    z = bytes(z)
    if len(z) < 6:
        raise FormatError("shorter than a header and a check value")
    if z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] * 256 + z[1]) % 31 or z[1] & 32:
        raise FormatError("zlib header %02x %02x" % (z[0], z[1]))
    bits = _Bits(z)
    bits.pos = 16
    out = bytearray()
    blocks = []
    while True:
        blk = dict(start=bits.pos, first=len(out))
        blk["final"] = bits.take(1)
        btype = bits.take(2)
        if btype == 0:
            blk["type"] = "stored"
            pad = bits.take((-bits.pos) % 8)
            blk["pad_zero"] = pad == 0
            blk["len"], blk["nlen"] = bits.take(16), bits.take(16)
            if blk["len"] ^ blk["nlen"] != 0xFFFF:
                raise FormatError("LEN %04x NLEN %04x" % (blk["len"], blk["nlen"]))
            p = bits.pos // 8
            if p + blk["len"] > len(z):
                raise FormatError("the stream ends inside a stored block")
            out += z[p:p + blk["len"]]
            bits.pos += 8 * blk["len"]
        elif btype == 1:
            blk["type"] = "fixed"
            lit = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "fixed literal/length")
            blk["tokens"] = _tokens(bits, lit, _decoder([5] * 32, "fixed distance"), out)
        elif btype == 2:
            blk["type"] = "dynamic"
            blk["hlit"], blk["hdist"], blk["hclen"] = bits.take(5), bits.take(5), bits.take(4)
            nlit, ndist = blk["hlit"] + 257, blk["hdist"] + 1
            if nlit > 286 or ndist > 30:
                raise FormatError("HLIT %d HDIST %d" % (blk["hlit"], blk["hdist"]))
            cllens = [0] * 19
            for k in range(blk["hclen"] + 4):
                cllens[CLORDER[k]] = bits.take(3)
            blk["cllens"] = cllens
            cl = _decoder(cllens, "code length code")
            lens, items = [], []
            while len(lens) < nlit + ndist:
                s = _symbol(bits, cl, "code length")
                x = bits.take(CL_EXTRA[s]) if s >= 16 else 0
                items.append((s, x))
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    if not lens:
                        raise FormatError("a 16 with nothing before it")
                    lens += [lens[-1]] * (3 + x)
                else:
                    lens += [0] * ((3 if s == 17 else 11) + x)
            if len(lens) > nlit + ndist:
                raise FormatError("code lengths run past HLIT + HDIST")
            blk["items"] = items
            blk["litlens"], blk["distlens"] = lens[:nlit], lens[nlit:]
            if blk["litlens"][256] == 0:
                raise FormatError("no end-of-block code")
            lit = _decoder(blk["litlens"], "literal/length")
            dist = _decoder(blk["distlens"], "distance", one_code_ok=True)
            blk["tokens"] = _tokens(bits, lit, dist, out)
        else:
            raise FormatError("block type 3")
        blk["nbits"] = bits.pos - blk["start"]
        blk["nbytes"] = len(out) - blk["first"]
        blocks.append(blk)
        if blk["final"]:
            break
    pad_bits = bits.take((-bits.pos) % 8)
    if len(z) - bits.pos // 8 != 4:
        raise FormatError("%d bytes behind the last block" % (len(z) - bits.pos // 8))
    return dict(header=z[:2], blocks=blocks, out=bytes(out), pad_bits=pad_bits, adler=int.from_bytes(z[-4:], "big"))


def ref_tokens(block_bytes: bytes):
    """the tokens of one block as the format states them: a maximal run is its first byte as a literal, then matches of
    distance 1 over the others, 258 at a time while 258 are left, then the rest as one match if it is 3 or more, else as
    literals"""
    toks = []
    i, n = 0, len(block_bytes)
    while i < n:
        c = block_bytes[i]
        j = i
        while j < n and block_bytes[j] == c:
            j += 1
        toks.append(("L", c))
        rest = j - i - 1
        while rest >= 258:
            toks.append(("M", 258, 1))
            rest -= 258
        if rest >= 3:
            toks.append(("M", rest, 1))
        else:
            toks += [("L", c)] * rest
        i = j
    return toks


def length_symbol(ln: int):
    """match length -> (symbol, extra bits), by RFC 1951's table"""
    for k in range(28, -1, -1):
        if ln >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k]
    raise ValueError(ln)


def token_counts(toks):
    """-> the 286 literal/length counts of a block (the end-of-block code once)"""
    freq = [0] * 286
    for t in toks:
        freq[t[1] if t[0] == "L" else length_symbol(t[1])[0]] += 1
    freq[256] = 1
    return freq


def greedy_items(seq):
    """the code length sequence as the format run-length codes it: zeros as 18 (11 - 138 at a time) while 11 or more are
    left, then one 17 for 3 - 10, else themselves; another length once, then 16 (3 - 6 at a time) while 3 or more of its
    copies are left, then themselves"""
    items = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        r = j - i
        i = j
        if v == 0:
            while r >= 11:
                items.append((18, min(r, 138) - 11))
                r -= min(r, 138)
            if r >= 3:
                items.append((17, r - 3))
                r = 0
        else:
            items.append((v, 0))
            r -= 1
            while r >= 3:
                items.append((16, min(r, 6) - 3))
                r -= min(r, 6)
        items += [(v, 0)] * r
    return items


def huffman_cost(freq):
    """-> (the least sum(freq * length) any prefix code has, the depth of the tree found).  Of equal weights the deeper
    subtree is merged first, so the depth is that of a deep optimal tree: a code that counts as within a limit here is so
    whichever way the writer breaks its ties (the cost does not depend on them at all)."""
    heap = [(f, 0) for f in freq if f]
    if len(heap) < 2:
        return sum(f for f, _ in heap), 1
    heap = [(f, -d) for f, d in heap]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, min(da, db) - 1))
    return cost, -heap[0][1]


def check_stream(z: bytes, data: bytes, B: int):
    """asserts everything the format promises of the stream z written for data with blocks of B bytes; -> parse(z)"""
    data = bytes(data)
    assert z[:2] == b"\x78\x9c", z[:2]
    p = parse(z)
    assert p["out"] == data, "inflates to other bytes"
    blocks = p["blocks"]
    assert len(blocks) == max(1, -(-len(data) // B)), len(blocks)
    for bi, blk in enumerate(blocks):
        last = bi == len(blocks) - 1
        assert blk["final"] == (1 if last else 0), bi
        assert blk["first"] == bi * B and blk["nbytes"] == (len(data) - bi * B if last else B), (bi, blk["nbytes"])
        assert blk["type"] in ("stored", "dynamic"), (bi, blk["type"])
        assert len(data) or blk["type"] == "stored", "empty input: one stored block of length 0"
        if blk["type"] == "stored":
            assert blk["pad_zero"] and blk["len"] == blk["nbytes"], bi
            continue
        piece = data[blk["first"]:blk["first"] + blk["nbytes"]]
        want = ref_tokens(piece)
        if blk["tokens"] != want:
            k = next((i for i, (a, b) in enumerate(zip(blk["tokens"], want)) if a != b), min(len(want), len(blk["tokens"])))
            raise AssertionError("block %d, token %d: %r written, the format asks for %r"
                                 % (bi, k, blk["tokens"][k:k + 3], want[k:k + 3]))
        assert all(t[2] == 1 for t in want if t[0] == "M")
        has_match = any(t[0] == "M" for t in want)
        assert blk["hdist"] == 0 and blk["distlens"] == [1 if has_match else 0], (bi, blk["hdist"], blk["distlens"])
        freq = token_counts(want)
        lens = blk["litlens"]
        used = [s for s in range(286) if freq[s]]
        assert [s for s, v in enumerate(lens) if v] == used, (bi, "codes for other symbols than the block uses")
        assert len(lens) == max(257, used[-1] + 1), (bi, blk["hlit"])
        ncl = blk["hclen"] + 4
        assert ncl == 4 or blk["cllens"][CLORDER[ncl - 1]] != 0, (bi, "HCLEN not trimmed", ncl)
        assert max(lens) <= 15 and kraft(lens, 15) == 1 << 15, (bi, "literal/length code")
        assert max(blk["cllens"]) <= 7 and kraft(blk["cllens"], 7) == 1 << 7, (bi, "code length code")
        assert blk["items"] == greedy_items(lens + blk["distlens"]), (bi, "code length items")
        clfreq = [0] * 19
        for s, _ in blk["items"]:
            clfreq[s] += 1
        assert all(blk["cllens"][s] for s in range(19) if clfreq[s]), bi
        for f, ln, limit, what in ((freq, lens, 15, "literal/length"), (clfreq, blk["cllens"], 7, "code length")):
            best, depth = huffman_cost(f)
            cost = sum(f[s] * ln[s] for s in range(len(ln)))
            assert cost >= best, (bi, what, cost, best)
            if depth <= limit and sum(1 for x in f if x) >= 2:
                assert cost == best, (bi, what, "costs %d bits, a Huffman code %d" % (cost, best))
    assert p["pad_bits"] == 0, "padding in front of the check value"
    assert p["adler"] == zlib.adler32(data), "%08x" % p["adler"]
    return p


def dynamic_bits(piece: bytes, plan) -> int:
    """the size of the dynamic block that writes ref_tokens(piece) with the codes of plan (a dict with lens, cllens, ncl and
    items as (code length symbol, ...)): counted here token by token"""
    lens, cllens = plan["lens"], plan["cllens"]
    n = 3 + 5 + 5 + 4 + 3 * plan["ncl"]
    for it in plan["items"]:
        n += cllens[it[0]] + CL_EXTRA.get(it[0], 0)
    for t in ref_tokens(piece):
        if t[0] == "L":
            n += lens[t[1]]
        else:
            sym, xb = length_symbol(t[1])
            n += lens[sym] + xb + 1    # (the one distance code has one bit)
    return n + lens[256]


def stored_bits(start: int, nbytes: int) -> int:
    """the size of a stored block that starts at bit `start` of the stream"""
    return 3 + (-(start + 3)) % 8 + 32 + 8 * nbytes


def block_choice(z: bytes, data: bytes, B: int, plan_of):
    """-> per block (type, bits as written, bits of the other form); plan_of(piece) gives the codes of the piece's dynamic
    form.  Asserts that the smaller form was written, the stored one when they are equal."""
    data = bytes(data)
    res = []
    for bi, blk in enumerate(parse(z)["blocks"]):
        piece = data[blk["first"]:blk["first"] + blk["nbytes"]]
        st = stored_bits(blk["start"], len(piece))
        dy = dynamic_bits(piece, plan_of(piece))
        if blk["type"] == "stored":
            assert blk["nbits"] == st, (bi, blk["nbits"], st)
            assert dy >= st, "block %d is stored in %d bits, its dynamic form has %d" % (bi, st, dy)
            res.append(("stored", st, dy))
        else:
            assert blk["nbits"] == dy, (bi, blk["nbits"], dy)
            assert dy < st, "block %d is dynamic in %d bits, its stored form has %d" % (bi, dy, st)
            res.append(("dynamic", dy, st))
    return res
