#!/usr/bin/env python3
"""The host pipes of `sref` and `ss paf2tsv` (sgk_sref_pipe_*, sgk_ss_pipe_*) timed inside one process, from create to
destroy, the way the CLI drives them: begin, fill the staging, submit, wait for the batch before, two slots in turn.

  --lib PATH   the library to load (default: the tree's); run the tool once per build and alternate the builds
  --reps N     timed runs per setting (a first, untimed one warms the process up)

Per pipe two settings: large batches (the CLI's default --batch) and small ones (many slot turnovers).  Batch sizes vary
from 60 % to 100 % of the setting's size, seeded, so that buffers grow where a growth rule lets them.  One JSON line per
setting: seconds per run, text bytes per run."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import make_paf


def put(dst, arr):
    C.memmove(dst, arr.ctypes.data, arr.nbytes)


def run_sref(L, api, levels, bases, sizes):
    pipe, st, text, n = C.c_void_p(), api.SrefStage(), C.c_void_p(), C.c_uint64()
    name, offs = np.frombuffer(b"chr1", dtype=np.uint8), np.array([0, 4], dtype=np.uint32)
    t0, total, pending = time.perf_counter(), 0, -1
    api.check(L.sgk_sref_pipe_create(0, levels.ctypes.data, 6, C.byref(pipe)), "create")
    for i, nb in enumerate(sizes):
        slot = i & 1
        spans, _ = api.sref_spans([nb], 6)
        api.check(L.sgk_sref_pipe_begin(pipe, slot, nb, len(spans), 1, 4, C.byref(st)), "begin")
        put(st.bases, bases[:nb]); put(st.spans, spans); put(st.name_bytes, name); put(st.name_offsets, offs)
        api.check(L.sgk_sref_pipe_submit(pipe, slot), "submit")
        if pending >= 0:
            api.check(L.sgk_sref_pipe_wait(pipe, pending, C.byref(text), C.byref(n)), "wait")
            total += n.value
        pending = slot
    api.check(L.sgk_sref_pipe_wait(pipe, pending, C.byref(text), C.byref(n)), "wait")
    total += n.value
    L.sgk_sref_pipe_destroy(pipe)
    return time.perf_counter() - t0, total


def run_ss(L, api, ss, recs, ids, id_offs, sizes):
    """recs: the records of the largest batch, strings back to back in ss; a batch is a prefix of them, a span each"""
    pipe, st, text, n = C.c_void_p(), api.SsStage(), C.c_void_p(), C.c_uint64()
    bad, status = C.c_uint32(), C.c_uint32()
    spans = api.ss_spans(recs["end_k"] - recs["st_k"])
    t0, total, pending = time.perf_counter(), 0, -1

    def wait(slot):
        api.check(L.sgk_ss_pipe_wait(pipe, slot, C.byref(text), C.byref(n), C.byref(bad), C.byref(status)), "wait")
        assert bad.value == 0xffffffff
        return n.value

    api.check(L.sgk_ss_pipe_create(0, C.byref(pipe)), "create")
    for i, nr in enumerate(sizes):
        slot = i & 1
        n_ss, n_id = int(recs["ss_offset"][nr - 1]) + int(recs["ss_len"][nr - 1]), int(id_offs[nr])
        api.check(L.sgk_ss_pipe_begin(pipe, slot, n_ss, nr, nr, nr, n_id, C.byref(st)), "begin")
        put(st.ss, ss[:n_ss]); put(st.records, recs[:nr]); put(st.spans, spans[:nr])
        put(st.id_bytes, ids[:n_id]); put(st.id_offsets, id_offs[:nr + 1])
        api.check(L.sgk_ss_pipe_submit(pipe, slot), "submit")
        if pending >= 0:
            total += wait(pending)
        pending = slot
    total += wait(pending)
    L.sgk_ss_pipe_destroy(pipe)
    return time.perf_counter() - t0, total


def ss_records(api, n, kmers):
    rows = list(make_paf.records(n, kmers))
    recs = np.zeros(n, dtype=api.SS_RECORD_DTYPE)
    pos = 0
    for i, (rid, s, start_raw, end_raw, sk, ek, tlen) in enumerate(rows):
        recs[i] = (pos, len(s), start_raw, end_raw, min(sk, ek), max(sk, ek), tlen, int(sk > ek), i)
        pos += len(s)
    id_offs = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum([len(r[0]) for r in rows], out=id_offs[1:])
    return (np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8), recs,
            np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8), id_offs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="batches per run, relative to the defaults")
    a = ap.parse_args()
    if a.lib:
        os.environ["SIGTK_AMD_LIB"] = os.path.abspath(a.lib)
    from sigtk_amd import api
    L = api.load_library()
    rs = np.random.RandomState(3)
    levels = (60 + 70 * rs.rand(4096)).astype(np.float32)
    bases = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=8 << 20)      # 2 strands: 16 Mi positions
    ss = ss_records(api, 105, 10000)                                             # 1.05 M rows

    def sizes(n, top, seed):
        return [int(x) for x in np.random.RandomState(seed).randint(int(0.6 * top), top + 1, size=max(2, int(n * a.scale)))]

    settings = [("sref, batches of up to 16 Mi positions", lambda: run_sref(L, api, levels, bases, sizes(300, 8 << 20, 1))),
                ("sref, batches of up to 256 Ki positions", lambda: run_sref(L, api, levels, bases, sizes(12000, 128 << 10, 2))),
                ("ss, batches of up to 105 records (1.05 M rows)", lambda: run_ss(L, api, *ss, sizes(600, 105, 3))),
                ("ss, batches of up to 6 records (60 000 rows)", lambda: run_ss(L, api, *ss, sizes(12000, 6, 4)))]
    for what, run in settings:
        run()
        res = [run() for _ in range(a.reps)]
        print(json.dumps({"what": what, "lib": a.lib or "tree", "seconds": [round(t, 4) for t, _ in res],
                          "text_bytes": res[0][1]}), flush=True)


if __name__ == "__main__":
    main()
