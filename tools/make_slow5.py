#!/usr/bin/env python3
"""Write a synthetic text SLOW5 file for the end-to-end timings of profiles/sigtext.md: `--distinct` synthetic DNA reads
(the generator of bench.py) turned into text once, written `--reads` times in all under different read ids."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=100000)
    ap.add_argument("--distinct", type=int, default=100)
    a = ap.parse_args()
    from sigtk_amd import api, blow5
    reads, dig, off, rng = api.synth_reads_host(a.distinct, a.read_len, 9, 0)
    tails = []
    for i, r in enumerate(reads):
        head = "\t".join(["0", blow5._plain_double(dig[i]), blow5._plain_double(off[i]), blow5._plain_double(rng[i]), "4000",
                          str(r.size)])
        tails.append(b"\t" + head.encode() + b"\t" + blow5.slow5_signal_text(r) + b"\n")
    with open(a.out, "wb") as fh:
        fh.write(b"#slow5_version\t0.2.0\n#num_read_groups\t1\n@experiment_type\tgenomic_dna\n@sequencing_kit\tsqk-lsk109\n")
        fh.write((blow5._TYPES + blow5._NAMES).encode())
        for k in range(a.reads):
            fh.write(b"synth-%08d" % k)
            fh.write(tails[k % a.distinct])
    print("%s: %d reads, %d samples, %d bytes" % (a.out, a.reads, a.reads * a.read_len, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
