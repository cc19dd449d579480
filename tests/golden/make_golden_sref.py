#!/usr/bin/env python3
"""Writes the sref fixtures: the FASTA inputs (deterministic) and, next to each, what the compiled reference
(`oracle/_ref/sigtk_ref sref`, built by oracle.build(ref=True)) prints for it.  The .tsv files are the reference's recorded
results (those above 8 KB gzipped); nothing here or in them is reference program text.

    python tests/golden/make_golden_sref.py

sref_db6.fa / sref_db5.fa   de Bruijn sequences over ACGT of order 6 / 5 plus k - 1 wrap-around bases: every k-mer once.
                            Position j of the '+' row of sref_db6.dna.tsv / sref_db5.rna.tsv is the level of the k-mer
                            at j -- the tests build their model files from these two rows (tests/sref_model.py).
sref_edge.fa                lengths 0, 3, 6, 7; lower case; N, R, Y; a sequence over two lines with an empty line behind
                            it; a header with a description; a space inside a sequence line; no final newline
sref_crlf.fa                CRLF line ends, with an empty (CRLF) line inside a sequence
sref_multi.fa               ~9 000 random bases in 12 records around the tile size of 256 positions, one of 3 000 bases,
                            two with N-runs
"""
import gzip
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")


def de_bruijn(order: int, alphabet: str = "ACGT") -> str:
    """the lexicographically least de Bruijn sequence (Lyndon words, FKM algorithm), cyclic length 4^order"""
    k, n = len(alphabet), order
    a = [0] * (k * n)
    out = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return "".join(alphabet[i] for i in out)


def wrap(seq: str, width: int = 70) -> str:
    return "\n".join(seq[i:i + width] for i in range(0, len(seq), width))


def inputs():
    files = {}
    for order in (6, 5):
        s = de_bruijn(order)
        assert len(s) == 4 ** order
        files["sref_db%d.fa" % order] = (">db%d de Bruijn order %d\n%s\n" % (order, order, wrap(s + s[:order - 1]))).encode()
    files["sref_edge.fa"] = (
        ">empty\n"
        ">len3\nACG\n"
        ">len6\nACGTAC\n"
        ">len7 a header with a description\nACGTACG\n"
        ">lower\nacgtacgtacgtttgaca\n"
        ">iupac\tTAB description\nACGTNNACGRYACGTNACGT\n"
        ">twolines\nACGTACGTAC\nGTACGGTTAA\n\n"
        ">space\nACGTAC GTACGTTGCA\n"
        ">len5\nACGTA\n"
        ">nofinalnewline\nTTGACCATGACCA").encode()
    files["sref_crlf.fa"] = (">crlf1 with description\r\nACGTACGTAC\r\nGTACGGTTAA\r\n\r\nCCATG\r\n"
                             ">crlf2\r\nACG\r\n>crlf3\r\nTTGACAGGCATTAGC\r\n").encode()
    rs = random.Random(20240611)
    recs = []
    for i, n in enumerate((255 + 5, 256 + 5, 257 + 5, 511 + 5, 512 + 5, 3000, 700, 901, 64, 1300, 300, 1024 + 5)):
        s = [rs.choice("ACGT") for _ in range(n)]
        if i in (6, 9):   # N-runs
            for lo, ln in ((100, 40), (n - 30, 12)):
                s[lo:lo + ln] = "N" * ln
        recs.append(">multi%02d\n%s\n" % (i, wrap("".join(s), 60 + i)))
    files["sref_multi.fa"] = "".join(recs).encode()
    return files


def run_ref(path, *opts):
    return subprocess.run([REF, "sref", *opts, path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it with oracle.build(ref=True)" % REF)
    for name, data in inputs().items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
    outs = {"sref_db6.dna.tsv": ("sref_db6.fa",), "sref_db5.rna.tsv": ("sref_db5.fa", "--rna"),
            "sref_edge.dna.tsv": ("sref_edge.fa",), "sref_edge.rna.tsv": ("sref_edge.fa", "--rna"),
            "sref_edge.dna_n.tsv": ("sref_edge.fa", "-n"),
            "sref_crlf.dna.tsv": ("sref_crlf.fa",), "sref_crlf.rna.tsv": ("sref_crlf.fa", "--rna"),
            "sref_multi.dna.tsv": ("sref_multi.fa",), "sref_multi.rna.tsv": ("sref_multi.fa", "--rna")}
    for out, (src, *opts) in outs.items():
        data = run_ref(os.path.join(HERE, src), *opts)
        if len(data) > 8192:    # the long rows are kept gzipped (mtime 0: the same bytes on every run)
            out += ".gz"
            with open(os.path.join(HERE, out), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
                f.write(data)
        else:
            with open(os.path.join(HERE, out), "wb") as f:
                f.write(data)
        print("%-28s %8d bytes" % (out, len(data)))


if __name__ == "__main__":
    main()
