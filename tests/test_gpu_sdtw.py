"""GPU parity: sgk_sdtw_f32 against the numpy model of its definition (tools/proto/sdtw_proto.py): score as a bit pattern
(a NaN for a NaN), end, start and flags exactly, for every pair of every batch.  The model's records of a batch are
computed once and shared by the tests that use the batch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import sdtw_proto as sp  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CANARY = 0x7FC12345   # a quiet NaN with a payload nobody computes
BAND = 1024           # rows of one pass (64 lanes x 16 rows): longer queries run in several
# 64 R - 1, 64 R, 64 R + 1 for every R the dispatch uses (1, 2, 4, 8, 16), and the smallest queries
EDGE_M = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
EDGE_N = (1, 2, 63, 64, 65, 200)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _values(kind, rs, n):
    if kind == "gauss":
        return rs.normal(0.0, 1.0, size=n).astype(F)
    return rs.randint(0, 3, size=n).astype(F)   # {0, 1, 2}: ties everywhere


def _run(queries, targets, options=0, q_leads=None, t_leads=None, max_q=None, max_t=None):
    """one call through the device layer -> records [n_queries, n_targets]"""
    import torch
    from sigtk_amd import api, device
    qb = device.upload_float_reads(queries, _dev(), leads=q_leads, fill=np.float32(np.nan))
    tb = device.upload_float_reads(targets, _dev(), leads=t_leads, fill=np.float32(np.nan))
    if max_q is not None:
        qb.max_read_len = max_q
    if max_t is not None:
        tb.max_read_len = max_t
    out = device.sdtw_f32(qb, tb, options)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(api.SDTW_DTYPE)[:len(queries) * len(targets)].reshape(len(queries), len(targets)).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    g, w = got.reshape(-1), want.reshape(-1)
    nan = np.isnan(w["score"])
    ok = np.where(nan, np.isnan(g["score"]), _bits(g["score"]) == _bits(w["score"]))
    ok &= (g["end"] == w["end"]) & (g["start"] == w["start"]) & (g["flags"] == w["flags"])
    bad = np.flatnonzero(~ok)
    nt = got.shape[1]
    assert bad.size == 0, "%s: %d of %d pairs differ; first (query %d, target %d): gpu %r model %r" % (
        what, bad.size, g.size, bad[0] // nt, bad[0] % nt, g[bad[0]], w[bad[0]])


class _Batch:
    def __init__(self, queries, targets):
        self.queries, self.targets = queries, targets
        self.want = sp.sdtw_batch(queries, targets)

    def want_no_start(self):
        w = self.want.copy()
        w["start"] = -1
        return w


@pytest.fixture(scope="module", params=["gauss", "ties"])
def edges(request):
    """1. every length at which the array fills, wraps or changes its rows per lane, against targets shorter than the
    array (n < 64), shorter than the query and longer"""
    rs = np.random.RandomState(7)
    return _Batch([_values(request.param, rs, m) for m in EDGE_M], [_values(request.param, rs, n) for n in EDGE_N])


def test_pipeline_edges(edges):
    _assert_same(_run(edges.queries, edges.targets), edges.want, "edges")


def test_no_start_keeps_score_and_end(edges):
    """6."""
    from sigtk_amd import api
    got = _run(edges.queries, edges.targets, api.SDTW_NO_START)
    assert (got["start"] == -1).all()
    _assert_same(got, edges.want_no_start(), "edges, no start")


@pytest.fixture(scope="module")
def passes():
    """2. queries of more than one band: band + 1, two bands, two bands + 1, three bands"""
    rs = np.random.RandomState(8)
    return _Batch([_values("gauss", rs, m) for m in (BAND + 1, 2 * BAND, 2 * BAND + 1, 3 * BAND)],
                  [_values("gauss", rs, n) for n in (1, 65, 700)])


def test_several_passes(passes):
    from sigtk_amd import api
    _assert_same(_run(passes.queries, passes.targets), passes.want, "passes")
    _assert_same(_run(passes.queries, passes.targets, api.SDTW_NO_START), passes.want_no_start(), "passes, no start")


def test_a_query_alone_and_in_a_mixed_batch(passes):
    """the band rows of one pair are nobody else's: alone, and between short queries of every kernel"""
    rs = np.random.RandomState(9)
    for r, q in enumerate(passes.queries):
        _assert_same(_run([q], passes.targets), passes.want[r:r + 1], "query %d alone" % r)
    short = [_values("gauss", rs, m) for m in (10, 300, 64, 1000)]
    mixed = [short[0], passes.queries[0], short[1], passes.queries[1], short[2], passes.queries[2], passes.queries[3], short[3]]
    got = _run(mixed, passes.targets)
    _assert_same(got[[1, 3, 5, 6]], passes.want, "long queries of the mixed batch")
    _assert_same(got[[0, 2, 4, 7]], sp.sdtw_batch(short, passes.targets), "short queries of the mixed batch")


def test_more_pairs_than_slots(passes):
    """1 100 queries x 2 targets is more pairs than there are band-row slots (2 048): a wave takes a second pair on the
    slot of its first; and from 1 024 queries on the pairs are dispatched by the queries' lengths"""
    rs = np.random.RandomState(10)
    kinds = [passes.queries[0], passes.queries[1][:BAND + 7], _values("gauss", rs, 40), passes.queries[0][:BAND + 1][::-1].copy()]
    targets = passes.targets[1:]
    want_kind = sp.sdtw_batch(kinds, targets)
    pick = rs.randint(0, len(kinds), size=1100)
    got = _run([kinds[k] for k in pick], targets)
    _assert_same(got, want_kind[pick], "1 100 queries")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_planted_match(where):
    """3. the query is a window of 120 levels, each repeated 1 - 3 times, with noise of a tenth of the levels' spread"""
    rs = np.random.RandomState(11)
    t = rs.normal(0.0, 1.0, size=3000).astype(F)
    w0 = {"first": 0, "middle": 1200, "last": 3000 - 120}[where]
    q = np.repeat(t[w0:w0 + 120], rs.randint(1, 4, size=120)).astype(F)
    q = (q + rs.normal(0.0, 0.1, size=q.size)).astype(F)
    want = sp.sdtw_batch([q], [t])
    _assert_same(_run([q], [t]), want, "planted " + where)
    # the window is found: an end of the path may slip by a level where the neighbouring level is within the noise
    assert abs(int(want["start"][0, 0]) - w0) <= 2 and abs(int(want["end"][0, 0]) - (w0 + 119)) <= 2, want


@pytest.fixture(scope="module")
def ragged():
    """4. 7 queries x 3 targets, lengths 0 .. 300"""
    rs = np.random.RandomState(12)
    return _Batch([_values("gauss", rs, m) for m in (0, 1, 300, 17, 64, 129, 255)], [_values("gauss", rs, n) for n in (300, 0, 33)])


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("touch", [True, False])
def test_layout_and_canaries(ragged, phase, touch):
    """every 16-byte phase of the first query and, the other way round, of the first target; reads that touch and reads
    with gaps; nothing outside `out` and the workspace is written, and every record of `out` is"""
    import torch
    from sigtk_amd import api, device
    nq, nt = len(ragged.queries), len(ragged.targets)
    q_leads = [phase] + ([0] * (nq - 1) if touch else [(3 * r + 1) % 5 for r in range(1, nq)])
    t_leads = [3 - phase] + ([0] * (nt - 1) if touch else [(2 * r + 3) % 5 for r in range(1, nt)])
    canary = np.array([CANARY], dtype=np.uint32).view(F)[0]
    qb = device.upload_float_reads(ragged.queries, _dev(), leads=q_leads, fill=canary)
    tb = device.upload_float_reads(ragged.targets, _dev(), leads=t_leads, fill=canary)
    q_before, t_before = qb.x.cpu().numpy().copy(), tb.x.cpu().numpy().copy()
    L = api._float_lib()
    need = int(L.sgk_sdtw_f32_workspace_bytes(qb.n_reads, qb.max_read_len, tb.n_reads, tb.max_read_len))
    rec_bytes = nq * nt * api.SDTW_DTYPE.itemsize
    out_all = torch.full((64 + rec_bytes + 64,), 0xA5, dtype=torch.uint8, device=_dev())
    ws_all = torch.full((64 + need + 64,), 0x5A, dtype=torch.uint8, device=_dev())
    assert out_all.data_ptr() % 16 == 0 and ws_all.data_ptr() % 16 == 0
    api.check(L.sgk_sdtw_f32(*qb.view(), *tb.view(), 0, out_all.data_ptr() + 64, ws_all.data_ptr() + 64, need,
                             int(torch.cuda.current_stream().cuda_stream)), "sgk_sdtw_f32")
    torch.cuda.synchronize()
    out = out_all.cpu().numpy()
    ws = ws_all.cpu().numpy()
    assert (out[:64] == 0xA5).all() and (out[64 + rec_bytes:] == 0xA5).all(), "written around out"
    assert (ws[:64] == 0x5A).all() and (ws[64 + need:] == 0x5A).all(), "written around the workspace"
    assert np.array_equal(_bits(qb.x.cpu().numpy()), _bits(q_before)) and np.array_equal(_bits(tb.x.cpu().numpy()), _bits(t_before))
    got = out[64:64 + rec_bytes].view(api.SDTW_DTYPE).reshape(nq, nt)
    assert not (got["flags"] == 0xA5A5A5A5).any(), "a record was not written"
    _assert_same(got, ragged.want, "ragged phase %d touch %d" % (phase, touch))


def test_flags():
    """5. a NaN or an infinity at the first, a middle or the last value of a query and of a target (a read of more than
    one tile of the sweep among them); no values at all; finite values whose sums overflow follow the formula"""
    rs = np.random.RandomState(13)
    big = np.finfo(F).max

    def hostile(n, at, what):
        x = _values("gauss", rs, n)
        x[at] = what
        return x

    queries = [_values("gauss", rs, 50), hostile(40, 0, np.nan), hostile(1100, 1099, np.nan), hostile(70, 35, np.inf),
               hostile(2000, 1500, -np.inf), np.zeros(0, dtype=F), np.full(5, big, dtype=F), hostile(1, 0, np.nan),
               np.array([big, -big, big * F(0.75)], dtype=F)]
    targets = [_values("gauss", rs, 80), hostile(30, 0, np.nan), hostile(1100, 1099, np.inf), hostile(90, 41, -np.inf),
               np.zeros(0, dtype=F), np.full(7, -big, dtype=F), np.array([-big, big, big * F(0.5)], dtype=F)]
    want = sp.sdtw_batch(queries, targets)
    assert want["flags"][0, 0] == 0 and want["flags"][5, 4] == sp.EMPTY and want["flags"][5, 1] == sp.EMPTY | sp.NONFINITE
    assert np.isinf(want["score"][6, 5]) and want["flags"][6, 5] == 0 and tuple(want[6, 5])[1:3] == (0, 0)
    _assert_same(_run(queries, targets), want, "flags")


def test_a_read_longer_than_its_max_is_flagged_not_read():
    from sigtk_amd import api
    rs = np.random.RandomState(14)
    queries = [_values("gauss", rs, m) for m in (20, 65, 1030)]
    targets = [_values("gauss", rs, n) for n in (100, 40)]
    got = _run(queries, targets, max_q=1029, max_t=99)
    want = np.zeros((3, 2), dtype=sp.REC_DTYPE)
    for a, q in enumerate(queries):
        for b, t in enumerate(targets):
            want[a, b] = sp.sdtw(q, t, max_q=1029, max_t=99)
    assert want["flags"].tolist() == [[api.SDTW_TOO_LONG, 0], [api.SDTW_TOO_LONG, 0], [api.SDTW_TOO_LONG, api.SDTW_TOO_LONG]]
    _assert_same(got, want, "too long")


def test_end_to_end_through_the_library():
    """7. sgk_sref_levels of a random sequence, both strands -> sgk_normalise_f32 of the strands and of a query planted on
    the '-' strand -> sgk_sdtw_f32: the better score is on the planted strand, inside the window, and what the model
    gives on the same normalised arrays"""
    import torch
    from sigtk_amd import api, device
    rs = np.random.RandomState(15)
    k = 6
    levels = rs.permutation(np.linspace(60.0, 120.0, 4 ** k)).astype(F)   # distinct
    seq = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=2000))
    plus, minus = device.sref_levels([seq], levels, k, device=_dev())
    assert plus.size == minus.size == 2000 + 1 - k
    w0, w1 = 700, 820
    q = np.repeat(minus[w0:w1], rs.randint(1, 4, size=w1 - w0)).astype(F)
    q = (q + rs.normal(0.0, 0.1 * float(levels.std()), size=q.size)).astype(F)
    fb = device.upload_float_reads([q, plus, minus], _dev(), leads=[1, 2, 0])
    y, _ = fb.normalise_f32(api.NORM_ZSCORE)
    off, ln = fb.offsets_host.astype(np.int64), fb.lengths_host.astype(np.int64)
    out = device.sdtw_f32(device.float_reads(y, off[:1], ln[:1]), device.float_reads(y, off[1:], ln[1:]))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(api.SDTW_DTYPE)[:2].reshape(1, 2)
    yh = y.cpu().numpy()
    norm = [yh[o:o + n].copy() for o, n in zip(off.tolist(), ln.tolist())]
    _assert_same(got, sp.sdtw_batch(norm[:1], norm[1:]), "end to end")
    assert got["score"][0, 1] < got["score"][0, 0]
    assert w0 - 2 <= got["start"][0, 1] <= got["end"][0, 1] <= w1 + 1
    assert abs(int(got["start"][0, 1]) - w0) <= 2 and abs(int(got["end"][0, 1]) - (w1 - 1)) <= 2
