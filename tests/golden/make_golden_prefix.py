#!/usr/bin/env python3
"""Writes the `prefix` fixtures of the hand-made catalogue (tests/prefix_cases.py): the reads whose scaling a BLOW5 file
can hold go into one RNA-headed BLOW5 for R9 (sqk-rna002) and one for RNA004 (sqk-rna004), in a temporary directory; what
the compiled reference (`oracle/_ref/sigtk_ref prefix --print-stat`, built by oracle.build(ref=True)) prints for each is
stored next to this script.  The .tsv files are the reference's recorded results (one row per read); nothing here or in
them is reference program text.  tests/test_gpu_prefix_cases.py writes the same two files and compares the CLI's output.

    python tests/golden/make_golden_prefix.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prefix_cases  # noqa: E402
from sigtk_amd import blow5  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
KITS = {"prefix_cases_r9.prefix_stat.tsv": "sqk-rna002", "prefix_cases_rna004.prefix_stat.tsv": "sqk-rna004"}


def write_catalogue_blow5(path, kit):
    recs = [blow5.Read(k.name, 0, k.dig, k.off, k.rng, 4000.0, k.raw) for k in prefix_cases.finite_cases(prefix_cases.catalogue())]
    blow5.write_blow5(path, recs, {"experiment_type": "rna", "sequencing_kit": kit})
    return len(recs)


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it with oracle.build(ref=True)" % REF)
    with tempfile.TemporaryDirectory() as tmp:
        for out, kit in KITS.items():
            f = os.path.join(tmp, "cases.blow5")
            n = write_catalogue_blow5(f, kit)
            data = subprocess.run([REF, "prefix", "--print-stat", f], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                  check=True, cwd=tmp).stdout
            with open(os.path.join(HERE, out), "wb") as fh:
                fh.write(data)
            print("%-40s %3d reads %6d bytes" % (out, n, len(data)))


if __name__ == "__main__":
    main()
