#!/usr/bin/env python3
"""A k-mer model file for `sigtk-amd sref --kmer-model`, recovered from what an `sref` prints.

sigtk-amd carries no pore model.  Someone who has built the reference can export the models it computes with:

    python tools/kmer_model_from_sref.py --fasta 6 > db6.fa          # a de Bruijn sequence: every 6-mer exactly once
    sigtk sref db6.fa > db6.tsv                                      # (--rna with order 5)
    python tools/kmer_model_from_sref.py --model 6 db6.fa db6.tsv > r9.4_dna.model

Position j of the '+' row is the level of the k-mer at position j of the sequence, so the row is the model in de Bruijn
order.  The levels are copied as text: nothing is rounded.  This tool ships no model and generates none."""
import argparse
import sys


def de_bruijn(order: int, alphabet: str = "ACGT") -> str:
    """lexicographically least de Bruijn sequence (concatenated Lyndon words), cyclic length 4^order"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fasta", type=int, metavar="K", help="print the de Bruijn FASTA of order K (1..6)")
    ap.add_argument("--model", type=int, metavar="K", help="print the model of order K from FASTA and TSV")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    k = a.fasta or a.model
    if not k or not 1 <= k <= 6 or (a.model and len(a.files) != 2):
        ap.error("give --fasta K, or --model K ref.fa sref.tsv")
    if a.fasta:
        s = de_bruijn(k)
        s += s[:k - 1]
        print(">db%d" % k)
        for i in range(0, len(s), 70):
            print(s[i:i + 70])
        return
    seq = "".join(ln.strip() for ln in open(a.files[0]) if not ln.startswith(">")).upper()
    rows = [ln.rstrip("\n").split("\t") for ln in open(a.files[1])]
    plus = [r for r in rows if len(r) == 5 and r[2] == "+" and r[0] != "ref_name"]
    if len(plus) != 1:
        sys.exit("expected one '+' row in %s" % a.files[1])
    values = plus[0][4].split(",")
    if len(values) != 4 ** k or len(seq) != 4 ** k + k - 1:
        sys.exit("%d values for a sequence of %d bases: not the output of sref on the order-%d de Bruijn FASTA"
                 % (len(values), len(seq), k))
    model = {}
    for j, v in enumerate(values):
        kmer = seq[j:j + k]
        float(v)
        if kmer in model or set(kmer) - set("ACGT"):
            sys.exit("k-mer %s at position %d: not a de Bruijn sequence over ACGT" % (kmer, j))
        model[kmer] = v
    print("#k\t%d" % k)
    print("kmer\tlevel_mean")
    for kmer in sorted(model):
        print("%s\t%s" % (kmer, model[kmer]))


if __name__ == "__main__":
    main()
