"""Records tests/golden/segmenter_params.json: the seeds of the window grid's reads, the parameter sets at their
decision edges, and the REFERENCE's own answers (positions only): its exported jnnv2 with each window, ref_jnn_raw_param
with the jnn sets on seeded reads, and ref_jnn_pa_param with the polyA sets on the pA tails of the catalogue's RNA reads.
Needs oracle/_ref (the reference built by oracle.build).  Run from the repository root:  python tests/golden/make_golden_segmenter_params.py"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import segmenter_params_model as M  # noqa: E402
from oracle.oracle import RefLib, _JnnPair, _Jnnv2Param, _p  # noqa: E402

STD_SCALE = 0.5
GOALS = ("open_at_0", "close_on_last", "open_at_end", "straddles_tile", "straddles_lane", "end==0", "merge_at_seg_dist-1",
         "no_merge_at_seg_dist", "len==lo-1", "len==lo", "len==hi", "len==hi+1")


def ref_jnnv2(ref, raw, p: M.AdaptW):
    f = ref.lib.jnnv2
    f.restype = _JnnPair
    f.argtypes = [C.POINTER(C.c_int16), C.c_int64, _Jnnv2Param]
    raw = np.ascontiguousarray(raw, dtype=np.int16)
    r = f(_p(raw, C.c_int16), raw.size, _Jnnv2Param(p.std_scale, p.seg_dist, p.window, 0.0, p.hi, p.lo))
    return [int(r.x), int(r.y)]


def reads_for(w):
    reads = []
    for e in M.EXTRA:
        for seed in ((0,) if e <= 2 else (0, 1, 2)):
            reads.append(M.GridRead(w, e, seed, 0))
    # a run that closes on the last window index: slide a read along its signal until the model says so
    for e in (1023, 3000):
        hit = None
        for seed in range(3, 9):
            for shift in range(0, 64):
                raw = M.gen_read(w, e, seed, shift)
                _, tags = M.runs_of(M.flags(raw, w, STD_SCALE), 0)
                if "close_on_last" in tags:
                    hit = M.GridRead(w, e, seed, shift)
                    break
            if hit:
                break
        if hit:
            reads.append(hit)
    return reads


def record_jnn(ref):
    """ref_jnn_raw_param: the reference's jnn_raw with every set of M.JNN_SETS on the seeded reads -> [set][read] = [xs, ys]"""
    reads = M.jnn_reads()
    out = []
    for kw in M.JNN_SETS:
        p = ref.jnn_param(**kw)
        row = []
        for raw in reads:
            x, y = ref.jnn_raw_param(raw, p)
            row.append([x.tolist(), y.tolist()])
        assert sum(len(r[0]) for r in row) > 0, kw
        out.append(row)
    return {"reads": [list(r) for r in M.JNN_READS], "segments": out}


def record_polya(ref):
    """ref_jnn_pa_param: the reference's jnn_pa with every polyA set on the pA tails of the catalogue's RNA reads, at the
    thresholds (m_a + shift) +- band -> [set][read] = first segment, [-1, -1] if none or if there is no adaptor"""
    cat = M.polya_reads()
    adaptors = [M.jnnv2_model(k.raw, M.POLYA_ADAPTOR)[0] for k in cat]
    sets = M.polya_sets(cat)
    first = []
    for q in sets:
        row = []
        for k, ad in zip(cat, adaptors):
            inp = M.polya_inputs(k, q, ad)
            if inp is None:
                row.append([-1, -1])
                continue
            tail, top, bot = inp
            p = ref.jnn_param(std_scale=-1.0, corrector=q.corrector, seg_dist=q.seg_dist, window=q.window,
                              stall_len=q.stall_len, error=q.error, top=float(top), bot=float(bot))
            x, y = ref.jnn_pa(tail, p)
            row.append([int(x[0]), int(y[0])] if len(x) else [-1, -1])
        first.append(row)
    return {"reads": [k.name for k in cat], "sets": [list(q) for q in sets], "first": first}


def main():
    ref = RefLib()
    gold = {"std_scale": STD_SCALE, "windows": {}}
    seen = set()
    n_cases = n_real = 0
    for w in M.WINDOWS:
        reads = reads_for(w)
        raws = [M.gen_read(*r) for r in reads]
        variants = []
        for r, raw in zip(reads, raws):
            if (r.extra, r.seed) in ((3000, 0), (1025, 1), (1023, 2)):
                for v in M.variants_for(w, raw, STD_SCALE):
                    if v not in variants:
                        variants.append(v)
        fls = [M.flags(raw, w, STD_SCALE) for raw in raws]
        answers = []
        for v in variants:
            row = []
            for raw, fl in zip(raws, fls):
                got = ref_jnnv2(ref, raw, v)
                ans, tags = M.jnnv2_model(raw, v, fl)
                assert list(ans) == got, (w, v, ans, got)
                seen |= tags
                n_cases += 1
                n_real += 0 if M.trivial(ans) else 1
                row.append(got)
            answers.append(row)
        gold["windows"][str(w)] = {"reads": [[r.extra, r.seed, r.shift] for r in reads],
                                   "variants": [[v.std_scale, v.seg_dist, v.hi, v.lo] for v in variants], "answers": answers}
        print(w, len(reads), "reads", len(variants), "variants", file=sys.stderr)
    missing = [g for g in GOALS if g not in seen]
    print("cases", n_cases, "with an answer", n_real, "missing goals", missing, file=sys.stderr)
    assert not missing and 2 * n_real >= n_cases
    gold["n_cases"], gold["n_with_answer"] = n_cases, n_real
    gold["jnn"] = record_jnn(ref)
    gold["polya"] = record_polya(ref)
    with open(M.GOLDEN, "w") as f:
        json.dump(gold, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
