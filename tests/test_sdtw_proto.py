"""CPU: tools/proto/sdtw_proto.py -- the numpy model of sgk_sdtw_f32.  Its two forms (the definition cell by cell, and one
anti-diagonal at a time) agree bit for bit, and hand-checked cases pin the definition: the tie rule (diagonal, then up,
then left) and the smallest end column."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto"))
import sdtw_proto as sp  # noqa: E402

F = np.float32
MS = (1, 2, 3, 7, 65)
NS = (1, 2, 5, 64, 70)


def _values(kind, rs, n):
    if kind == "gauss":
        return rs.normal(0.0, 1.0, size=n).astype(F)
    return rs.randint(0, 3, size=n).astype(F)   # {0, 1, 2}: ties everywhere


@pytest.mark.parametrize("kind", ["gauss", "ties"])
@pytest.mark.parametrize("m", MS)
def test_the_two_forms_agree(kind, m):
    rs = np.random.RandomState(1000 + m)
    for n in NS:
        q, t = _values(kind, rs, m), _values(kind, rs, n)
        dl, sl = sp.last_row_loops(q, t)
        dd, sd = sp.last_row_diagonals(q, t)
        assert np.array_equal(dl.view(np.uint32), dd.view(np.uint32)), (kind, m, n)
        assert np.array_equal(sl, sd), (kind, m, n)
        a, b = sp.sdtw_loops(q, t), sp.sdtw_diagonals(q, t)
        assert a[0].view(np.uint32) == b[0].view(np.uint32) and a[1:] == b[1:], (kind, m, n)


@pytest.mark.parametrize("form", [sp.sdtw_loops, sp.sdtw_diagonals])
def test_a_query_of_one_value(form):
    t = np.array([5.0, 3.0, 1.5, 3.0, 1.5], dtype=F)
    score, end, start = form(np.array([1.0], dtype=F), t)
    assert (float(score), end, start) == (0.5, 2, 2)       # the first of the two columns at distance 0.5


@pytest.mark.parametrize("form", [sp.sdtw_loops, sp.sdtw_diagonals])
def test_a_target_of_one_value_gives_the_column_sum(form):
    q = np.array([1.0, 2.5, -4.0, 0.25], dtype=F)
    score, end, start = form(q, np.array([1.0], dtype=F))
    assert float(score) == 0.0 + 1.5 + 5.0 + 0.75 and (end, start) == (0, 0)


@pytest.mark.parametrize("form", [sp.sdtw_loops, sp.sdtw_diagonals])
def test_a_query_that_is_a_window_of_the_target(form):
    t = np.array([9.0, 8.0, 7.0, 1.0, 2.0, 3.0, 4.0, 9.5, 8.5], dtype=F)
    score, end, start = form(t[3:7].copy(), t)
    assert (float(score), end, start) == (0.0, 6, 3)


@pytest.mark.parametrize("form", [sp.sdtw_loops, sp.sdtw_diagonals])
@pytest.mark.parametrize("m,n", [(1, 1), (1, 6), (4, 1), (4, 6), (6, 4), (5, 5)])
def test_all_equal_values_pin_the_tie_rule(form, m, n):
    """every D is 0.  Row m - 1 is 0 everywhere: end is its smallest column, 0, and column 0 starts at 0.  Along the row
    the diagonal wins every tie: S(i,j) = max(j - i, 0) -- with "up" or "left" first it would be j or 0."""
    q, t = np.full(m, 2.5, dtype=F), np.full(n, 2.5, dtype=F)
    assert form(q, t) == (F(0.0), 0, 0)
    last = sp.last_row_loops if form is sp.sdtw_loops else sp.last_row_diagonals
    d, s = last(q, t)
    assert not d.any()
    assert s.tolist() == [max(j - (m - 1), 0) for j in range(n)]


def test_each_neighbour_wins_where_it_is_strictly_less():
    # q = (0, 1), t = (0, 1, 1).  Row 0: 0 1 1.  (1,0) = 0 + 1.  (1,1): diagonal 0, up 1, left 1 -> the diagonal, S 0.
    # (1,2): diagonal 1, up 1, left 0 -> left, S 0
    # q = (1, 1), t = (0, 1).  Row 0: 1 0.  (1,0) = 1 + 1.  (1,1): diagonal 1, up 0, left 2 -> up, S 1
    # q = (3, 1), t = (1, 3, 1).  Row 0: 2 0 2.  (1,0) = 2 + 0.  (1,1): diagonal 2, up 0, left 2 -> up: 2 + 0, S 1.
    # (1,2): diagonal 0 (S 1), up 2, left 2 -> the diagonal: 0 + 0, S 1
    cases = (((0, 1), (0, 1, 1), [1.0, 0.0, 0.0], [0, 0, 0]),
             ((1, 1), (0, 1), [2.0, 0.0], [0, 1]),
             ((3, 1), (1, 3, 1), [2.0, 2.0, 0.0], [0, 1, 1]))
    for form in (sp.last_row_loops, sp.last_row_diagonals):
        for q, t, want_d, want_s in cases:
            d, s = form(np.array(q, dtype=F), np.array(t, dtype=F))
            assert d.tolist() == want_d and s.tolist() == want_s, (q, t)


def test_records_of_pairs_that_are_not_aligned():
    q, t = np.array([1.0, 2.0], dtype=F), np.array([1.0, 2.0, 3.0], dtype=F)
    nan_q = np.array([1.0, np.nan], dtype=F)
    inf_t = np.array([-np.inf, 2.0, 3.0], dtype=F)
    empty = np.zeros(0, dtype=F)
    for a, b, flags in ((nan_q, t, sp.NONFINITE), (q, inf_t, sp.NONFINITE), (empty, t, sp.EMPTY), (q, empty, sp.EMPTY),
                        (empty, inf_t, sp.EMPTY | sp.NONFINITE)):
        score, end, start, f = sp.sdtw(a, b)
        assert np.isnan(score) and (end, start, f) == (-1, -1, flags)
    assert sp.sdtw(q, t) == (F(0.0), 1, 0, 0)
    assert sp.sdtw(q, t, sp.NO_START) == (F(0.0), 1, -1, 0)
    assert sp.sdtw(q, t, max_q=1)[3] == sp.TOO_LONG and sp.sdtw(q, inf_t, max_t=2)[3] == sp.TOO_LONG


def test_sums_that_overflow_follow_the_formula():
    big = np.finfo(F).max
    q = np.array([big, big, big], dtype=F)
    t = np.array([-big, -big], dtype=F)
    for form in (sp.sdtw_loops, sp.sdtw_diagonals):
        score, end, start = form(q, t)
        assert np.isinf(score) and score > 0 and (end, start) == (0, 0)
    assert sp.sdtw(q, t)[3] == 0
