"""GPU: the two-slot host pipes of the CLI (sgk_sref_pipe_*, sgk_ss_pipe_*) driven directly through the C ABI: the slot
state machine by return code, two slots in flight, buffers that grow and are reused, and what each pipe checks or reports
on its own.  Expected bytes are the numpy / Python models' (tests/sref_model.py, tests/ss_model.py)."""
import ctypes as C

import numpy as np
import pytest

import sref_model as SM
import ss_model as XM
from sigtk_amd import api

pytestmark = pytest.mark.gpu

OK, ERR_ARG = api.SGK_OK, api.SGK_ERR_ARG
NONE = 0xffffffff


def put(dst, arr):
    """the bytes of a numpy array (or bytes) to the staging pointer dst"""
    raw = arr if isinstance(arr, bytes) else np.ascontiguousarray(arr).tobytes()
    if raw:
        C.memmove(dst, raw, len(raw))


def offsets_of(items):
    offs = np.zeros(len(items) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in items], out=offs[1:])
    return offs


class SrefBatch:
    def __init__(self, recs, k, rna, max_span=None):
        self.spans, _ = api.sref_spans([len(s) for _, s in recs], k, rna, max_span=max_span)
        self.bases = b"".join(s for _, s in recs)
        self.names = b"".join(n for n, _ in recs)
        self.name_offs = offsets_of([n for n, _ in recs])
        self.n_names = len(recs)
        self.want = SM.sref_text(recs, SM.golden_levels(k), k, rna, header=False)


class SrefPipe:
    def __init__(self, L, k):
        self.L, self.h = L, C.c_void_p()
        levels = np.ascontiguousarray(SM.golden_levels(k), dtype=np.float32)
        assert L.sgk_sref_pipe_create(0, levels.ctypes.data, k, C.byref(self.h)) == OK

    def close(self):
        self.L.sgk_sref_pipe_destroy(self.h)

    def begin(self, slot, b):
        st = api.SrefStage()
        rc = self.L.sgk_sref_pipe_begin(self.h, slot, len(b.bases), len(b.spans), b.n_names, len(b.names), C.byref(st))
        if rc == OK:
            put(st.bases, b.bases)
            put(st.spans, b.spans)
            put(st.name_bytes, b.names)
            put(st.name_offsets, b.name_offs)
        return rc

    def submit(self, slot):
        return self.L.sgk_sref_pipe_submit(self.h, slot)

    def wait(self, slot):
        """-> (rc, address of the text, its bytes)"""
        text, n = C.c_void_p(), C.c_uint64(0xdead)
        rc = self.L.sgk_sref_pipe_wait(self.h, slot, C.byref(text), C.byref(n))
        return rc, text.value, n.value


class SsBatch:
    """records (ss_model.Record) back to back in one string buffer, one id per record, spans in record order"""

    def __init__(self, records, max_span=None, stop_at=None):
        self.ss = b"".join(r.ss for r in records)
        self.ids = b"".join(r.rid for r in records)
        self.id_offs = offsets_of([r.rid for r in records])
        self.recs = np.zeros(len(records), dtype=api.SS_RECORD_DTYPE)
        pos = 0
        for i, r in enumerate(records):
            self.recs[i] = (pos, len(r.ss), r.start_raw, r.end_raw, r.st_k, r.end_k, r.tlen, r.rna, i)
            pos += len(r.ss)
        self.spans = api.ss_spans([r.rows for r in records], max_span=max_span)
        self.n_ids = len(records)
        good = records if stop_at is None else records[:stop_at]
        self.want = b"".join(XM.rows_text(r, XM.decode(r)[2]) for r in good)


class SsPipe:
    def __init__(self, L):
        self.L, self.h = L, C.c_void_p()
        assert L.sgk_ss_pipe_create(0, C.byref(self.h)) == OK
        self.bad = (NONE, 0)

    def close(self):
        self.L.sgk_ss_pipe_destroy(self.h)

    def begin(self, slot, b):
        st = api.SsStage()
        rc = self.L.sgk_ss_pipe_begin(self.h, slot, len(b.ss), len(b.recs), len(b.spans), b.n_ids, len(b.ids), C.byref(st))
        if rc == OK:
            put(st.ss, b.ss)
            put(st.records, b.recs)
            put(st.spans, b.spans)
            put(st.id_bytes, b.ids)
            put(st.id_offsets, b.id_offs)
        return rc

    def submit(self, slot):
        return self.L.sgk_ss_pipe_submit(self.h, slot)

    def wait(self, slot):
        text, n, bad, st = C.c_void_p(), C.c_uint64(0xdead), C.c_uint32(7), C.c_uint32(7)
        rc = self.L.sgk_ss_pipe_wait(self.h, slot, C.byref(text), C.byref(n), C.byref(bad), C.byref(st))
        self.bad = (bad.value, st.value)
        return rc, text.value, n.value


def random_seq(rs, n):
    return rs.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=n, p=[.24, .24, .24, .24, .04]).tobytes()


def ss_record(rs, rows, rid, rna=False):
    """a record whose columns agree with its string"""
    s, raw = XM.random_ss(rs, rows, p_del=0.1, max_del=3)
    st_k, start_raw = int(rs.randint(0, 5000)), int(rs.randint(0, 1000))
    a, b = (st_k + rows, st_k) if rna else (st_k, st_k + rows)
    r = XM.Record(rid, s, start_raw, start_raw + raw, a, b, st_k + rows + 3)
    assert XM.decode(r)[0] == 0
    return r


def sref_batch(seed, n, max_span=None, k=6, rna=False):
    rs = np.random.RandomState(seed)
    return SrefBatch([(b"seq%d_%d" % (seed, i), random_seq(rs, int(x))) for i, x in enumerate(np.atleast_1d(n))], k, rna, max_span)


def ss_batch(seed, rows, max_span=None):
    rs = np.random.RandomState(seed)
    return SsBatch([ss_record(rs, int(x), b"read-%d-%d" % (seed, i), rna=bool(i % 2)) for i, x in enumerate(np.atleast_1d(rows))],
                   max_span)


@pytest.fixture(scope="module")
def lib(gpu):
    return api.load_library()


@pytest.fixture(params=["sref", "ss"])
def pipe(request, lib):
    """(a fresh pipe, a function (seed, size, max_span) -> batch; size: bases of a sequence / k-mers of a record)"""
    p = SrefPipe(lib, 6) if request.param == "sref" else SsPipe(lib)
    yield p, (sref_batch if request.param == "sref" else ss_batch)
    p.close()


def run(p, slot, b):
    assert p.begin(slot, b) == OK and p.submit(slot) == OK
    rc, addr, n = p.wait(slot)
    assert rc == OK
    return C.string_at(addr, n)


# ------------------------------------------------------------------------------------------------ both pipes

def test_slot_state_machine(pipe):
    p, make = pipe
    b = make(1, [40, 7])
    for slot in (-1, 2):
        assert p.begin(slot, b) == ERR_ARG and p.submit(slot) == ERR_ARG and p.wait(slot)[0] == ERR_ARG
    assert p.wait(0)[0] == ERR_ARG                       # idle
    assert p.submit(0) == ERR_ARG                        # never begun
    assert p.submit(1) == ERR_ARG
    assert p.begin(0, b) == OK and p.submit(0) == OK
    assert p.begin(0, b) == ERR_ARG and p.submit(0) == ERR_ARG      # busy
    rc, addr, n = p.wait(0)
    assert rc == OK and C.string_at(addr, n) == b.want
    assert p.wait(0)[0] == ERR_ARG                       # a second wait
    assert p.wait(1)[0] == ERR_ARG                       # the other slot was never used
    assert p.begin(0, b) == OK and p.submit(0) == OK     # after wait the slot is free again
    rc, addr, n = p.wait(0)
    assert rc == OK and C.string_at(addr, n) == b.want


def test_two_slots_in_flight(pipe):
    p, make = pipe
    a, b, c = make(2, [300, 20]), make(3, [700]), make(4, [5, 150, 90])
    assert p.begin(0, a) == OK and p.submit(0) == OK
    assert p.begin(1, b) == OK and p.submit(1) == OK
    rc0, addr0, n0 = p.wait(0)
    assert rc0 == OK and C.string_at(addr0, n0) == a.want
    rc1, addr1, n1 = p.wait(1)
    assert rc1 == OK
    assert p.begin(0, c) == OK and p.submit(0) == OK     # slot 0 works on while slot 1's text is still being read
    assert C.string_at(addr1, n1) == b.want
    rc0, addr0, n0 = p.wait(0)
    assert rc0 == OK and C.string_at(addr0, n0) == c.want
    assert C.string_at(addr1, n1) == b.want
    assert len({a.want, b.want, c.want}) == 3


def test_buffers_grow_and_are_reused(pipe):
    """small, large, small, then larger still and cut into spans of 256.  A buffer sized for the small batch has a few
    KiB of slack (sref's workspace, which holds the 64 KiB text table: some 20 KiB).  The large batch outgrows that for
    the staging and the text, the last one for the workspace and the per-span and per-record arrays too (more than
    1100 of each)."""
    p, make = pipe
    small, small2 = make(5, [60, 9]), make(6, [33])
    if isinstance(p, SrefPipe):
        large, larger = make(7, [70000]), make(8, [150000], 256)
    else:
        large = make(7, [50000])
        rs = np.random.RandomState(8)
        records = [ss_record(rs, 1, b"one%d" % i) for i in range(1100)] + [ss_record(rs, 20000, b"long", rna=True)]
        records.append(XM.Record(b"deleted", b"4,279990D7,", 3, 14, 10, 280002, 0))       # 279 992 rows, two of them mapped
        assert XM.decode(records[-1])[0] == 0
        larger = SsBatch(records, 256)
    assert len(large.want) > 900000 and len(larger.spans) > 1100
    for b in (small, large, small2, larger, small):
        assert run(p, 0, b) == b.want
    assert run(p, 1, larger) == larger.want              # the other slot's buffers are its own


# ------------------------------------------------------------------------------------------------ sref only

@pytest.fixture(scope="module", params=[(6, False), (5, True)], ids=["k6", "k5rna"])
def sref_pipe(request, lib):
    k, rna = request.param
    p = SrefPipe(lib, k)
    yield p, k, rna
    p.close()


def test_sref_sequence_shorter_than_k(sref_pipe):
    p, k, rna = sref_pipe
    b = SrefBatch([(b"tiny", b"ACG")], k, rna)
    assert len(b.spans) == (1 if rna else 2) and not b.spans["count"].any()
    assert b.want == (b"tiny\t3\t+\t%d\t" % (4 - k)) + (b"" if rna else b"tiny\t3\t-\t%d\t" % (4 - k))
    assert run(p, 0, b) == b.want


def test_sref_span_counts(sref_pipe):
    """1, 3 and 257 spans per strand"""
    p, k, rna = sref_pipe
    rs = np.random.RandomState(9)
    for n_spans, slot in ((1, 0), (3, 1), (257, 0)):
        ref_len = 7 * n_spans - 3
        b = SrefBatch([(b"chr", random_seq(rs, ref_len + k - 1))], k, rna, max_span=None if n_spans == 1 else 7)
        assert len(b.spans) == n_spans * (1 if rna else 2)
        assert run(p, slot, b) == b.want


def test_sref_several_sequences(sref_pipe):
    p, k, rna = sref_pipe
    b = sref_batch(10, [0, 1, k - 1, k, k + 1, 255 + k, 256 + k, 600], max_span=256, k=k, rna=rna)
    assert run(p, 1, b) == b.want


# ------------------------------------------------------------------------------------------------ ss only

@pytest.fixture(scope="module")
def ss_pipe(lib):
    p = SsPipe(lib)
    yield p
    p.close()


def test_ss_no_records(ss_pipe):
    b = SsBatch([])
    assert ss_pipe.begin(0, b) == OK and ss_pipe.submit(0) == OK
    rc, _, n = ss_pipe.wait(0)
    assert rc == OK and n == 0 and ss_pipe.bad == (NONE, 0)


def _beyond_the_strings(b):
    b.recs["ss_len"][1] = len(b.ss) - int(b.recs["ss_offset"][1]) + 1


def _offset_beyond_the_strings(b):
    b.recs["ss_offset"][2] = len(b.ss) + 1
    b.recs["ss_len"][2] = 0


def _id_out_of_range(b):
    b.recs["id"][0] = b.n_ids


def _k_range_reversed(b):
    b.recs["st_k"][1] = b.recs["end_k"][1] + 1


def _span_of_no_record(b):
    b.spans["record"][-1] = len(b.recs)


def _spans_not_ascending(b):
    b.spans["record"][2] = 0
    b.spans["count"][2] = 0


def _span_beyond_the_rows(b):
    b.spans["count"][1] += 1


@pytest.mark.parametrize("spoil", [_beyond_the_strings, _offset_beyond_the_strings, _id_out_of_range, _k_range_reversed,
                                   _span_of_no_record, _spans_not_ascending, _span_beyond_the_rows])
def test_ss_submit_checks_the_staging_on_the_host(ss_pipe, spoil):
    good = ss_batch(11, [10, 20, 5])
    b = ss_batch(11, [10, 20, 5])
    spoil(b)
    assert ss_pipe.begin(1, b) == OK
    assert ss_pipe.submit(1) == ERR_ARG
    assert ss_pipe.wait(1)[0] == ERR_ARG                 # nothing was submitted: the slot is idle ...
    assert ss_pipe.begin(1, good) == OK                  # ... and free
    assert ss_pipe.submit(1) == OK
    rc, addr, n = ss_pipe.wait(1)
    assert rc == OK and C.string_at(addr, n) == good.want and ss_pipe.bad == (NONE, 0)


@pytest.mark.parametrize("bad_at", [2, 0])
def test_ss_first_bad_record_ends_the_text(gpu, ss_pipe, bad_at):
    from sigtk_amd import device
    rs = np.random.RandomState(12)
    records = [ss_record(rs, rows, b"r%d" % i) for i, rows in enumerate((30, 300, 12))]
    bad = XM.Record(b"bad", b"5,,3,", 0, 0, 0, 2, 5)     # status 1 (test_decode_every_status of test_gpu_ss.py)
    records.insert(bad_at, bad)
    status = int(device.ss_decode([bad], validate=True)[1][0])
    assert status == XM.decode(bad)[0] == 1
    b = SsBatch(records, stop_at=bad_at)
    assert ss_pipe.begin(0, b) == OK and ss_pipe.submit(0) == OK
    rc, addr, n = ss_pipe.wait(0)
    assert rc == OK and n == len(b.want) and ss_pipe.bad == (bad_at, status)
    assert (n == 0) == (bad_at == 0)
    if n:
        assert C.string_at(addr, n) == b.want
