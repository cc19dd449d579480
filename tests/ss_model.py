"""The Python restatement of `sigtk ss paf2tsv` (the reference's src/ss.c as the issue of this feature words it), with the
statuses of sgk_ss_decode.  test_ss_cpu.py proves it equal to every recorded output of the reference; the GPU tests use it
where the reference is undefined (st_k >= 2000, long D runs, numbers out of range)."""
import gzip
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = b"read_id\tkmer_idx\tstart_raw_idx\tend_raw_idx\n"
INT32_MAX = 2 ** 31 - 1
SAT = 2 ** 31

MESSAGES = {1: b"Bad ss: Preceding digit missing", 2: b"Bad ss: A non-digit found when expected a digit",
            3: b"Bad ss: Signal end mismatch", 4: b"Bad ss: Kmer end mismatch", 5: b"Bad ss: Number out of range"}

#: fixture -> (exit status, the stderr line or None)
FIXTURES = {"ss_dna.paf": (0, None), "ss_rna.paf": (0, None),
            "ss_bad_digit.paf": (1, MESSAGES[1]), "ss_bad_byte.paf": (1, MESSAGES[2]),
            "ss_bad_signal.paf": (1, MESSAGES[3]), "ss_bad_kmer.paf": (1, MESSAGES[4])}


def golden(name: str) -> bytes:
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path + ".gz"):
        return gzip.open(path + ".gz", "rb").read()
    return open(path, "rb").read()


def expected(name: str) -> bytes:
    """what the reference printed for tests/golden/<name>"""
    return golden(name[:-4] + ".tsv")


class Record:
    def __init__(self, rid, ss, start_raw, end_raw, start_kmer, end_kmer, tlen):
        self.rid, self.ss = bytes(rid), bytes(ss)
        self.start_raw, self.end_raw, self.tlen = int(start_raw), int(end_raw), int(tlen)
        self.rna = int(start_kmer > end_kmer)
        self.st_k, self.end_k = min(start_kmer, end_kmer), max(start_kmer, end_kmer)

    @property
    def rows(self):
        return self.end_k - self.st_k


def decode(rec: Record):
    """-> (status, (i_raw, i_k) or (-1, -1), {k-mer: (start, end)})"""
    i_raw, i_k = rec.start_raw, rec.st_k
    pairs = {}
    val = ndig = 0
    rng = False
    for c in rec.ss:
        if 48 <= c <= 57:
            val = val * 10 + (c - 48)
            ndig += 1
        elif c in b",ID":
            if ndig == 0:
                return 1, (-1, -1), pairs
            if ndig > 10 or val > INT32_MAX:
                rng = True
            if c == 73:
                i_raw += val
            elif c == 68:
                i_k += val
            else:
                pairs[i_k] = (i_raw, i_raw + val)
                i_raw += val
                i_k += 1
            val = ndig = 0
        else:
            return 2, (-1, -1), pairs
    if rng or i_raw > INT32_MAX or i_k > INT32_MAX:
        return 5, (-1, -1), pairs
    if i_raw != rec.end_raw:
        return 3, (i_raw, i_k), pairs
    if i_k != rec.end_k:
        return 4, (i_raw, i_k), pairs
    return 0, (i_raw, i_k), pairs


def rows_text(rec: Record, pairs, first=0, count=None) -> bytes:
    """rows of k-mers st_k + first .. + count"""
    count = rec.rows - first if count is None else count
    out = []
    for i in range(rec.st_k + first, rec.st_k + first + count):
        idx = rec.tlen - i - 1 if rec.rna else i
        p = pairs.get(i)
        out.append(b"%s\t%d\t%s\n" % (rec.rid, idx, b"%d\t%d" % p if p is not None else b".\t."))
    return b"".join(out)


def atoi(s: bytes) -> int:
    s = s.lstrip(b" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in (b"+", b"-"):
        sign, i = (-1 if s[:1] == b"-" else 1), 1
    j = i
    while j < len(s) and 48 <= s[j] <= 57:
        j += 1
    return sign * int(s[i:j]) if j > i else 0


class PafError(Exception):
    pass


def parse_line(line: bytes) -> Record:
    line = line.split(b"\0")[0]
    f = [x for x in line.replace(b"\r", b"\t").replace(b"\n", b"\t").split(b"\t") if x]
    if len(f) < 12:
        raise PafError("fewer than 12 fields")
    if f[4] not in (b"+", b"-"):
        raise PafError("strand")
    v = [atoi(f[i]) for i in (2, 3, 6, 7, 8)]
    if any(not -2 ** 31 <= x <= INT32_MAX for x in v):
        raise PafError("does not fit an int")
    if v[0] < 0 or v[3] < 0 or v[4] < 0:
        raise PafError("is negative")
    ss = [x[5:] for x in f[12:] if x.startswith(b"ss:Z:")]
    if not ss:
        raise PafError("ss:Z: tag not found in paf record for %s" % f[0].decode("latin1"))
    return Record(f[0], ss[-1], v[0], v[1], v[3], v[4], v[2])


def paf2tsv(data: bytes):
    """-> (stdout, exit status, the stderr words or None)"""
    out = [HEADER]
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        try:
            rec = parse_line(line + b"\n")
        except PafError as e:
            return b"".join(out), 1, str(e).encode("latin1")
        st, _, pairs = decode(rec)
        if st:
            return b"".join(out), 1, MESSAGES[st]
        out.append(rows_text(rec, pairs))
    return b"".join(out), 0, None


def paf_line(rid, ss, start_raw, end_raw, start_kmer, end_kmer, tlen, strand=b"+", tags_before=(), tags_after=(), eol=b"\n"):
    f = [rid, b"%d" % max(end_raw, 0), b"%d" % start_raw, b"%d" % end_raw, strand, b"ref", b"%d" % tlen,
         b"%d" % start_kmer, b"%d" % end_kmer, b"%d" % abs(end_kmer - start_kmer), b"%d" % abs(end_kmer - start_kmer), b"60"]
    return b"\t".join(f + list(tags_before) + [b"ss:Z:" + ss] + list(tags_after)) + eol


def random_ss(rs, n_kmers, p_del=0.05, p_ins=0.05, max_del=5, zero=0.02, lead_zero=0.05):
    """a DNA-like string covering n_kmers k-mers -> (ss, raw samples consumed): every k-mer is a ',' token (dwell
    geometric around 9, `zero` of them 0) or falls into a D run of 1..max_del; I tokens in between"""
    out, raw, k = [], 0, 0
    while k < n_kmers:
        u = rs.random_sample()
        if u < p_del:
            d = int(min(rs.randint(1, max_del + 1), n_kmers - k))
            out.append(b"%dD" % d)
            k += d
            continue
        if u < p_del + p_ins:
            n = int(rs.randint(1, 40))
            out.append(b"%dI" % n)
            raw += n
        n = 0 if rs.random_sample() < zero else int(rs.geometric(1 / 9.0))
        tok = b"%d" % n
        if rs.random_sample() < lead_zero:
            tok = b"0" * int(rs.randint(1, 4)) + tok
        out.append(tok + b",")
        raw += n
        k += 1
    return b"".join(out), raw
