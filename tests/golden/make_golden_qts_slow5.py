#!/usr/bin/env python3
"""Writes the fixtures of `qts` on text SLOW5 files: a hand-made input and what the compiled reference
(`oracle/_ref/sigtk_ref qts`, built by oracle.build(ref=True)) writes for it, one output per method; and, in
qts_slow5.json, the sha256 of the reference's outputs for the 100 reads of sp1_dna.blow5 written as text by
sigtk_amd.blow5.write_slow5.  The .slow5 files are an input and the reference's recorded results; nothing here or in
them is reference program text.

    python tests/golden/make_golden_qts_slow5.py

qts_aux.slow5   two header attributes and six auxiliary columns (uint8_t, int32_t, float, double, char*, uint16_t*),
                6 reads: 300 samples, the int16 edge values around every -b 3 rounding step, a 0-sample read, a read of
                one sample, 700 samples with '.' in every auxiliary column, 257 samples.  The doubles of the main columns
                come in spellings slow5lib would not write (8192.0, -0.50, 4000., 1402.88232421875, -0, -0.0), which the
                reference re-prints; the auxiliary columns hold no type-max literal and their floats are spelt as slow5lib
                spells them, so that the reference writes them back as they stand.
qts_aux.b3_<method>.slow5   `sigtk_ref qts -b 3 -m <method>` of it
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
REF = os.path.join(ROOT, "oracle", "_ref", "sigtk_ref")
METHODS = ("floor", "round", "fill-ones")

HEADER = ("#slow5_version\t0.2.0\n#num_read_groups\t1\n@asic_id\t4175987214\n@exp_start_time\t2020-10-27T05:28:45Z\n"
          "#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\tuint8_t\tint32_t\tfloat\tdouble\tchar*\tuint16_t*\n"
          "#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\t"
          "channel\tstart_mux\tmedian_before\tdrift\tnote\ttrace\n")


def aux_input() -> bytes:
    rs = np.random.RandomState(20261019)
    edges = np.array([-32768, -32767, -32765, -32764, -32761, -9, -8, -5, -4, -3, -1, 0, 1, 3, 4, 5, 7, 8, 9, 32756, 32759,
                      32760, 32763, 32764, 32766, 32767], dtype=np.int64)
    sigs = [rs.randint(-600, 1400, 300), edges, np.zeros(0, np.int64), np.array([32767]), rs.randint(-32768, 32768, 700),
            rs.randint(200, 900, 257)]
    main = [("8192.0", "-0.50", "1467.610000", "4000."), ("8192", "3", "1402.88232421875", "4000"),
            ("2048", "-0", "748.5801", "3012"), ("8192", "-0.0", "1402.882324", "4000"),
            ("8192", "6", "1467.61", "4000.000"), ("8192.000000", "-243", "1402.882324", "4000")]
    aux = [("12", "-5", "201.5", "0.001953", "a note with spaces", "1,2,3,65534"),
           ("0", "2147483646", "-1.25", "-3", "x", "7"),
           ("254", "-2147483648", "0", "0", ".", "."),
           ("7", "1", "1467.609985", "12345.678", "tabs are not possible, commas are", "0"),
           (".", ".", ".", ".", ".", "."),
           ("1", "0", "3.1", "100", "last", "10,20")]
    out = HEADER
    for k, (s, m, a) in enumerate(zip(sigs, main, aux)):
        out += "\t".join(["read_%d-aux" % k, "0", *m, str(len(s)), ",".join(str(int(v)) for v in s), *a]) + "\n"
    return out.encode("ascii")


def ref_qts(inp: str, outp: str, method: str, bits: int = 3) -> bytes:
    subprocess.run([REF, "qts", "-b", str(bits), "-m", method, inp, "-o", outp], check=True, capture_output=True)
    return open(outp, "rb").read()


def main() -> None:
    from sigtk_amd import blow5
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/sigtk_ref is not built (oracle.build(ref=True))")
    inp = os.path.join(HERE, "qts_aux.slow5")
    with open(inp, "wb") as fh:
        fh.write(aux_input())
    digests = {}
    with tempfile.TemporaryDirectory() as d:
        for m in METHODS:
            got = ref_qts(inp, os.path.join(d, "o.slow5"), m)
            with open(os.path.join(HERE, "qts_aux.b3_%s.slow5" % m), "wb") as fh:
                fh.write(got)
            print("qts_aux.b3_%s.slow5: %d bytes" % (m, len(got)))
        sp1 = blow5.read_blow5(os.path.join(HERE, "sp1_dna.blow5"))
        text = os.path.join(d, "sp1_dna.slow5")
        blow5.write_slow5(text, sp1.reads, {k: v[0] for k, v in sp1.attrs.items()})
        digests["sp1_dna.slow5.sha256"] = hashlib.sha256(open(text, "rb").read()).hexdigest()
        for m in METHODS:
            for bits in (1, 3, 8):
                got = ref_qts(text, os.path.join(d, "o.slow5"), m, bits)
                digests["sp1_dna.qts_b%d_%s.slow5.sha256" % (bits, m)] = hashlib.sha256(got).hexdigest()
    with open(os.path.join(HERE, "qts_slow5.json"), "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
