#!/usr/bin/env python3
"""Writes the `ss paf2tsv` fixtures: deterministic PAF inputs and, next to each, what the compiled reference
(`oracle/_ref/sigtk_ref ss paf2tsv`, built by oracle.build(ref=True)) prints for it.  The .tsv files are the reference's
recorded results (those above 8 KB gzipped); nothing here or in them is reference program text.

    python tests/golden/make_golden_ss.py

All records stay inside the domain where the reference is defined: st_k < 2000 and every D run <= 5.

ss_dna.paf      rows 0, 1, 2, 255, 256, 257, 513 and 3000; "0," mappings, runs of I tokens, leading zeros, digits behind the
                last op, two ss:Z: fields (the last wins), other tags before and after, an empty field, a CRLF line
ss_rna.paf      start_kmer > end_kmer: rows 1, 2, 255, 256, 257, 513, 1000, a record with tlen 3 (negative indices), one
                with tlen negative, a DNA record of 0 rows with an empty string; the last line has no line end
ss_bad_*.paf    a good record, a bad one, a good one: the reference prints the first record's rows and exits 1 with
                Preceding digit missing / A non-digit found / Signal end mismatch / Kmer end mismatch
"""
import gzip
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ss_model as M  # noqa: E402


def rid(rs):
    h = "%032x" % int.from_bytes(rs.bytes(16), "big")
    return ("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()


def record(rs, rows, rna=False, st_k=None, start_raw=None, tlen=None, ss_edit=None, **kw):
    ss, raw = M.random_ss(rs, rows)
    st_k = int(rs.randint(0, 1500)) if st_k is None else st_k
    start_raw = int(rs.randint(0, 5000)) if start_raw is None else start_raw
    tlen = st_k + rows + int(rs.randint(0, 100)) if tlen is None else tlen
    if ss_edit:
        ss, raw = ss_edit(ss, raw)
    a, b = (st_k + rows, st_k) if rna else (st_k, st_k + rows)
    return M.paf_line(rid(rs), ss, start_raw, start_raw + raw, a, b, tlen, **kw)


def inputs():
    files = {}
    rs = np.random.RandomState(20250313)
    dna = [
        record(rs, 0, ss_edit=lambda s, r: (b"7I", 7)),
        record(rs, 1),
        record(rs, 2, ss_edit=lambda s, r: (s + b"123", r)),                       # digits behind the last op
        record(rs, 255, tags_before=[b"ss:Z:1,,x"], tags_after=[b"sh:f:2.0"]),      # two ss:Z: fields: the last wins
        record(rs, 256, tags_before=[b"tp:A:P", b"sc:f:1.5"], tags_after=[b"sm:f:0.5", b"rest:Z:ss:Z:"]),
        record(rs, 257, ss_edit=lambda s, r: (b"3I4I005I" + s, r + 12), st_k=1000),
        record(rs, 513, eol=b"\r\n"),
        record(rs, 3000, st_k=1999),
        record(rs, 40, strand=b"-"),
        record(rs, 300, start_raw=0, st_k=0),
    ]
    dna[7] = dna[7].replace(b"\t", b"\t\t", 1)   # an empty field: it vanishes
    # leading zeros in the columns, and a token of ten digits with leading zeros in the string
    dna.append(M.paf_line(rid(rs), b"0000000012,0,00,3D004,", 5, 21, 7, 14, 20).replace(b"\t5\t21\t", b"\t005\t0021\t"))
    files["ss_dna.paf"] = b"".join(dna)
    rs = np.random.RandomState(20250314)
    rna = [record(rs, n, rna=True) for n in (1, 2, 255, 256, 257, 513, 1000)]
    rna.append(record(rs, 9, rna=True, st_k=0, tlen=3))       # indices 2, 1, 0, -1 .. -6
    rna.append(record(rs, 5, rna=True, st_k=10, tlen=-4))
    rna.append(M.paf_line(rid(rs), b"", 17, 17, 33, 33, 100))  # no rows at all
    rna.append(record(rs, 64, rna=True, eol=b""))              # no final newline
    files["ss_rna.paf"] = b"".join(rna)
    rs = np.random.RandomState(20250315)
    good = [record(rs, 20), record(rs, 300, rna=True)]

    def bad(name, line):
        files["ss_bad_%s.paf" % name] = good[0] + line + good[1]

    bad("digit", M.paf_line(rid(rs), b"5,3,,4,", 0, 12, 0, 4, 10))
    bad("byte", M.paf_line(rid(rs), b"5,3x4,,", 0, 12, 0, 3, 10))   # the non-digit stands in front of the empty token
    bad("signal", M.paf_line(rid(rs), b"5,3,2D4,", 10, 21, 3, 8, 10))
    bad("kmer", M.paf_line(rid(rs), b"5,3,2D4,", 10, 22, 3, 9, 10))
    return files


def run_ref(path):
    p = subprocess.run([REF, "ss", "paf2tsv", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.stdout, p.returncode, p.stderr


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it with oracle.build(ref=True)" % REF)
    for name, data in inputs().items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        out, rc, err = run_ref(os.path.join(HERE, name))
        want_rc, want_err = M.FIXTURES[name]
        assert rc == want_rc, (name, rc, err)
        assert want_err is None or err.strip().splitlines()[0] == want_err, (name, err)
        tsv = name[:-4] + ".tsv"
        if len(out) > 8192:    # kept gzipped (mtime 0: the same bytes on every run)
            tsv += ".gz"
            with open(os.path.join(HERE, tsv), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
                f.write(out)
        else:
            with open(os.path.join(HERE, tsv), "wb") as f:
                f.write(out)
        print("%-24s exit %d %8d bytes of rows  %s" % (tsv, rc, len(out), err.strip()[:60]))


if __name__ == "__main__":
    main()
