"""Shared by tests/test_sref_cpu.py and tests/test_gpu_sref.py: a kseq-rule FASTA parser, the pore models recovered from
the de Bruijn goldens, model-file writers and a numpy model of `sigtk sref` (src/sref.c:100-210, src/ref.h).

The reference's models are not in the tree.  Position j of the '+' row of sref_db6.dna.tsv / sref_db5.rna.tsv is the
level of the k-mer at position j of the de Bruijn sequence, and every k-mer occurs there exactly once."""
import gzip
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = b"ref_name\tref_len\tstrand\tsig_len\tsig_mean\n"
_SPACE = re.compile(rb"[ \t\n\r\v\f]")


def golden(name: str) -> bytes:
    """a fixture's bytes; the long recorded outputs are kept as <name>.gz"""
    path = os.path.join(GOLDEN, name)
    if not os.path.exists(path):
        return gzip.decompress(open(path + ".gz", "rb").read())
    with open(path, "rb") as f:
        return f.read()


def parse_fasta(data: bytes):
    """kseq's rules (src/kseq.h:185-225) -> [(name, sequence bytes)]; ValueError for a FASTQ record"""
    recs, n, pos = [], len(data), 0
    while pos < n and data[pos] not in b">@":
        pos += 1
    while pos < n:
        if data[pos] == ord("@"):
            raise ValueError("FASTQ")
        pos += 1
        if pos >= n:
            break
        m = _SPACE.search(data, pos)
        e = m.start() if m else n
        name, pos = data[pos:e], e
        if pos < n:
            c = data[pos]
            pos += 1
            if c != 10:                       # the description
                j = data.find(b"\n", pos)
                pos = n if j < 0 else j + 1
        seq = bytearray()
        while pos < n and data[pos] not in b">+@":
            j = data.find(b"\n", pos)
            line = data[pos:(n if j < 0 else j)]
            if line:
                seq += line
                # one '\r' goes when the sequence so far is longer than one byte (ks_getuntil2); a one-byte last line
                # without a line end is appended by kseq_read itself and stays
                if len(seq) > 1 and seq[-1] == 13 and not (len(line) == 1 and j < 0):
                    seq.pop()
            pos = n if j < 0 else j + 1
        if pos < n and data[pos] == ord("+"):
            raise ValueError("FASTQ")
        recs.append((bytes(name), bytes(seq)))
    return recs


def fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for v in data:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


_CODE = np.zeros(256, dtype=np.uint32)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def strand_codes(seq: bytes, strand: int) -> np.ndarray:
    """2-bit codes of the strand's bases: every non-ACGT byte is 0 on '+'; '-' is the reverse with 3 - code"""
    c = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    return (3 - c[::-1]) if strand else c


def ranks(seq: bytes, k: int, strand: int = 0) -> np.ndarray:
    c = strand_codes(seq, strand).astype(np.int64)
    n = len(seq) + 1 - k
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    r = np.zeros(n, dtype=np.int64)
    for m in range(k):
        r = (r << 2) | c[m:m + n]
    return r


def rows_of(text: bytes, header: bool = True):
    """the rows of an sref output as (name, l, strand, sig_len, [value texts]); understands the head-only rows, which
    end with a tab and no newline"""
    if header:
        assert text.startswith(HEADER)
        text = text[len(HEADER):]
    out, pos, n = [], 0, len(text)
    while pos < n:
        f = text[pos:].split(b"\t", 4)
        name, l, strand, sig_len = f[0], int(f[1]), f[2], int(f[3])
        pos += len(name) + len(f[1]) + len(f[2]) + len(f[3]) + 4
        vals = []
        if sig_len > 0:
            e = text.index(b"\n", pos)
            vals = text[pos:e].split(b",")
            assert len(vals) == sig_len
            pos = e + 1
        out.append((name, l, strand, sig_len, vals))
    return out


def golden_levels(k: int) -> np.ndarray:
    """the reference's model for k = 6 (DNA) or 5 (RNA), float32 by k-mer rank, from the de Bruijn golden"""
    fa, tsv = ("sref_db6.fa", "sref_db6.dna.tsv") if k == 6 else ("sref_db5.fa", "sref_db5.rna.tsv")
    (_, seq), = parse_fasta(golden(fa))
    row = rows_of(golden(tsv))[0]
    assert row[2] == b"+" and row[3] == 4 ** k
    r = ranks(seq, k)
    assert np.array_equal(np.sort(r), np.arange(4 ** k))      # every k-mer exactly once
    levels = np.zeros(4 ** k, dtype=np.float32)
    levels[r] = np.array([float(v) for v in row[4]], dtype=np.float32)
    assert all(b"%f" % float(levels[r[j]]) == row[4][j] for j in range(0, 4 ** k, 7))   # the round trip loses nothing
    return levels


def kmer(rank: int, k: int) -> str:
    return "".join("ACGT"[(rank >> (2 * (k - 1 - m))) & 3] for m in range(k))


def write_model(path, levels: np.ndarray, k: int, order=None, k_line: bool = True, header: bool = True,
                extra_cols: bool = False, fmt=None) -> str:
    """a k-mer model file in the reference's format (src/model.c:39-140)"""
    fmt = fmt or (lambda v: "%f" % float(v))
    lines = ["#model_name\ttest"]
    if k_line:
        lines.append("#k\t%d" % k)
    if header:
        lines.append("kmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv" if extra_cols else "kmer\tlevel_mean")
    for r in (range(4 ** k) if order is None else order):
        lines.append("%s\t%s%s" % (kmer(int(r), k), fmt(levels[r]), "\t1.5\t0.9\t0.1" if extra_cols else ""))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


def sref_text(records, levels: np.ndarray, k: int, rna: bool = False, header: bool = True) -> bytes:
    """what `sigtk sref` prints for the records [(name, sequence)] with the model `levels`"""
    table = [b"%f" % float(v) for v in np.asarray(levels, dtype=np.float32)]
    out = [HEADER] if header else []
    for name, seq in records:
        n = len(seq) + 1 - k
        for strand in ((0,) if rna else (0, 1)):
            out.append(b"%s\t%d\t%s\t%d\t" % (name, len(seq), b"-" if strand else b"+", n))
            if n > 0:
                out.append(b",".join([table[r] for r in ranks(seq, k, strand).tolist()]))
                out.append(b"\n")
    return b"".join(out)


FIXTURES = {   # golden output -> (input, options)
    "sref_db6.dna.tsv": ("sref_db6.fa", ()), "sref_db5.rna.tsv": ("sref_db5.fa", ("--rna",)),
    "sref_edge.dna.tsv": ("sref_edge.fa", ()), "sref_edge.rna.tsv": ("sref_edge.fa", ("--rna",)),
    "sref_edge.dna_n.tsv": ("sref_edge.fa", ("-n",)),
    "sref_crlf.dna.tsv": ("sref_crlf.fa", ()), "sref_crlf.rna.tsv": ("sref_crlf.fa", ("--rna",)),
    "sref_multi.dna.tsv": ("sref_multi.fa", ()), "sref_multi.rna.tsv": ("sref_multi.fa", ("--rna",)),
}
FASTAS = sorted({v[0] for v in FIXTURES.values()})
