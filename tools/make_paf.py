#!/usr/bin/env python3
"""A synthetic resquiggle PAF for `ss paf2tsv` (tools/bench_ss.py; also usable on its own):

    python tools/make_paf.py out.paf [--records 10000] [--kmers 10000] [--seed 1]

Every record covers --kmers k-mers, has a 36-byte read id (a UUID) and a DNA-like ss:Z: string.  The op mix, per k-mer:
  5 %   start a deletion run "<n>D" over n = 1..5 k-mers (uniform)
  else  a mapping "<n>," with n geometric, mean 9 samples (2 % of the mappings are "0,"); 5 % of the mappings are
        preceded by an insertion "<n>I", n = 1..39 (uniform)
which gives about 2.2 bytes of string and 55 bytes of TSV per k-mer.  start_kmer stays below 1000, inside the domain where the
reference is defined, so the same file can be timed with it.  Formatting 10^8 tokens one by one is slow in Python, so the strings come
from a pool of --pool (32) distinct ones, used in turn with fresh ids, start offsets and k-mer offsets; every 7th record is
RNA-style (start_kmer > end_kmer).  The defaults give 10^8 rows, about 5.5 GB of TSV."""
import argparse
import sys

import numpy as np


def one_string(rs, n_kmers):
    out, raw, k = [], 0, 0
    while k < n_kmers:
        if rs.random_sample() < 0.05:
            d = int(min(rs.randint(1, 6), n_kmers - k))
            out.append(b"%dD" % d)
            k += d
            continue
        if rs.random_sample() < 0.05:
            n = int(rs.randint(1, 40))
            out.append(b"%dI" % n)
            raw += n
        n = 0 if rs.random_sample() < 0.02 else int(rs.geometric(1 / 9.0))
        out.append(b"%d," % n)
        raw += n
        k += 1
    return b"".join(out), raw


def uuid(rs):
    h = "%032x" % int.from_bytes(rs.bytes(16), "big")
    return ("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()


def records(n_records, n_kmers, seed=1, pool=32):
    """yields (rid, ss, start_raw, end_raw, start_kmer, end_kmer, tlen)"""
    rs = np.random.RandomState(seed)
    strings = [one_string(rs, n_kmers) for _ in range(min(pool, n_records))]
    for i in range(n_records):
        ss, raw = strings[i % len(strings)]
        start_raw, st_k = int(rs.randint(0, 100000)), int(rs.randint(0, 1000))
        a, b = (st_k + n_kmers, st_k) if i % 7 == 6 else (st_k, st_k + n_kmers)
        yield uuid(rs), ss, start_raw, start_raw + raw, a, b, st_k + n_kmers + 50


def line(rid, ss, start_raw, end_raw, start_kmer, end_kmer, tlen):
    n = abs(end_kmer - start_kmer)
    return b"%s\t%d\t%d\t%d\t+\tref\t%d\t%d\t%d\t%d\t%d\t60\tss:Z:%s\n" % (rid, end_raw, start_raw, end_raw, tlen, start_kmer,
                                                                        end_kmer, n, n, ss)


def write(path, n_records, n_kmers, seed=1, pool=32):
    """-> (bytes of the ss strings, rows)"""
    ss_bytes = 0
    with open(path, "wb") as f:
        for r in records(n_records, n_kmers, seed, pool):
            f.write(line(*r))
            ss_bytes += len(r[1])
    return ss_bytes, n_records * n_kmers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pool", type=int, default=32)
    a = ap.parse_args()
    ss_bytes, rows = write(a.out, a.records, a.kmers, a.seed, a.pool)
    print("%s: %d records, %d rows, %d bytes of ss strings" % (a.out, a.records, rows, ss_bytes), file=sys.stderr)


if __name__ == "__main__":
    main()
