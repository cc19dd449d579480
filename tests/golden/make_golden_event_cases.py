#!/usr/bin/env python3
"""Writes the `event` fixtures of the hand-made catalogue (tests/event_cases.py): the reads of event_cases.cli_cases() go into
one DNA-headed and one RNA-headed BLOW5 in a temporary directory; what the compiled reference (`oracle/_ref/sigtk_ref event`
and `event -c`, built by oracle.build(ref=True)) prints for each is stored next to this script.  The .tsv files are the
reference's recorded results (a row per event, or per read with -c); nothing here or in them is reference program text.
tests/test_gpu_event_cases.py writes the same two files and compares the CLI's output.

    python tests/golden/make_golden_event_cases.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import event_cases  # noqa: E402
from sigtk_amd import blow5  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
HEADERS = {"dna": {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"},
           "rna": {"experiment_type": "rna", "sequencing_kit": "sqk-rna002"}}


def write_catalogue_blow5(path, kind):
    dig, off, rng = event_cases.SCALE
    recs = [blow5.Read(k.name, 0, dig, off, rng, 4000.0, k.raw) for k in event_cases.cli_cases() if k.raw.size > 0]
    blow5.write_blow5(path, recs, HEADERS[kind])
    return len(recs)


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it with oracle.build(ref=True)" % REF)
    with tempfile.TemporaryDirectory() as tmp:
        for kind in HEADERS:
            f = os.path.join(tmp, "cases.blow5")
            n = write_catalogue_blow5(f, kind)
            for out, opts in (("event_cases_%s.event.tsv" % kind, []), ("event_cases_%s.event_c.tsv" % kind, ["-c"])):
                data = subprocess.run([REF, "event", *opts, f], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True,
                                      cwd=tmp).stdout
                with open(os.path.join(HERE, out), "wb") as fh:
                    fh.write(data)
                print("%-36s %3d reads %7d bytes" % (out, n, len(data)))


if __name__ == "__main__":
    main()
