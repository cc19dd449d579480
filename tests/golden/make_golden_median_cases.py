#!/usr/bin/env python3
"""Writes the fixtures of the median catalogue (tests/median_cases.py), all of them results recorded from the compiled
reference (oracle/_ref, built by oracle.build(ref=True)):

  median_cases.json       per case n, the CRC32 of the sample bytes, the raw median and the five float statistics as bit
                          patterns (ref_stat); per float case n, CRC32 and the bits of mean / stdv / median (ref_statf);
                          per region case the adaptor / polyA coordinates and the six region statistics
  median_range0.stat.tsv  what `sigtk_ref stat` prints for six short reads under `range 0` in a text SLOW5 file
  median_prefix.prefix_stat.tsv   what `sigtk_ref prefix --print-stat` prints for the region reads, under degenerate and
                          negative scales, in a text SLOW5 file
The two SLOW5 files are written into a temporary directory (write_range0_slow5 / write_prefix_slow5);
tests/test_gpu_median_cases.py writes the same files and compares the CLI's output.

Nothing here or in the files is reference program text.

    python tests/golden/make_golden_median_cases.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import median_cases  # noqa: E402
from sigtk_amd import blow5  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def stat_entry(lib, k):
    s = lib.stat(k.raw, k.dig, k.off, k.rng)
    return {"n": int(k.raw.size), "crc": median_cases.crc(k.raw), "raw_median": int(s[4]),
            "bits": [bits(s[i]) for i in (0, 1, 2, 3, 5)]}   # raw_mean, pa_mean, raw_std, pa_std, pa_median


def region_entry(lib, k, rna, pore):
    """prefix as the reference's cfunc.c forms it: find_adaptor, the statistics of pA[x:y], find_polya on pA[y:] with the
    thresholds from the adaptor's mean, the statistics of that region"""
    with np.errstate(all="ignore"):
        pa = lib.pa(k.raw, k.dig, k.off, k.rng)
        ax, ay = lib.find_adaptor(k.raw, pore)
        e = {"n": int(k.raw.size), "crc": median_cases.crc(k.raw), "adapt": [int(ax), int(ay)], "polya": [-1, -1],
             "adapt_bits": [0, 0, 0], "polya_bits": [0, 0, 0]}
        if ay > 0:
            st = lib.statf(pa[ax:ay])
            e["adapt_bits"] = [bits(v) for v in st]
            if rna:
                mid = np.float32(st[0]) + np.float32(30)
                px, py = lib.find_polya(pa[ay:], mid + np.float32(20), mid - np.float32(20), pore)
                e["polya"] = [int(px), int(py)]
                if py > 0:
                    e["polya_bits"] = [bits(v) for v in lib.statf(pa[ay + px:ay + py])]
    return e


def _reads(cases):
    return [blow5.Read(k.name, 0, k.dig, k.off, k.rng, 4000.0, k.raw) for k in cases]


def write_range0_slow5(path):
    blow5.write_slow5(path, _reads(median_cases.range0_reads()), {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"})


def write_prefix_slow5(path):
    blow5.write_slow5(path, _reads(median_cases.region_file_cases()), {"experiment_type": "rna", "sequencing_kit": "sqk-rna002"})


def main():
    from oracle.oracle import RefLib
    if not RefLib.available() or not os.path.exists(REF):
        sys.exit("oracle/_ref is missing: build it with oracle.build(ref=True)")
    lib = RefLib()
    doc = {"stat": {k.name: stat_entry(lib, k) for k in median_cases.cases()}, "float": {}, "region": {}}
    for k in median_cases.float_cases():
        st = lib.statf(k.x)
        doc["float"][k.name] = {"n": int(k.x.size), "crc": median_cases.crc(k.x), "bits": [bits(v) for v in st]}
    for k in median_cases.region_cases():
        doc["region"][k.name] = region_entry(lib, k, 1, median_cases.REGION_PORE)
    written = {}
    with open(os.path.join(HERE, "median_cases.json"), "w") as fh:   # one case per line
        fh.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (grp, ",\n".join(
            "%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in sorted(doc[grp].items())))
            for grp in sorted(doc)) + "\n}\n")
    written["median_cases.json"] = None
    with tempfile.TemporaryDirectory() as tmp:
        for write, out, args in ((write_range0_slow5, "median_range0.stat.tsv", ["stat"]),
                                 (write_prefix_slow5, "median_prefix.prefix_stat.tsv", ["prefix", "--print-stat"])):
            f = os.path.join(tmp, "cases.slow5")
            write(f)
            data = subprocess.run([REF] + args + [f], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, cwd=tmp).stdout
            with open(os.path.join(HERE, out), "wb") as fh:
                fh.write(data)
            written[out] = None
    mpath = os.path.join(HERE, "MANIFEST.json")
    manifest = json.load(open(mpath))
    for name in written:
        manifest[name] = hashlib.sha256(open(os.path.join(HERE, name), "rb").read()).hexdigest()
        print("%-34s %8d bytes" % (name, os.path.getsize(os.path.join(HERE, name))))
    with open(mpath, "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
