"""Numpy model of sgk_sdtw_f32 (include/sigtk_gpu.h): subsequence DTW of a query against a target, the
whole query with a free start and a free end in the target.  Every operation is float32 with one rounding:

    c(i,j) = fabsf(q[i] - t[j])
    D(0,j) = c(0,j)                   S(0,j) = j
    D(i,0) = D(i-1,0) + c(i,0)        S(i,0) = S(i-1,0)   (= 0)
    D(i,j) = c(i,j) + best            S(i,j) = S(best's cell)
             best = D(i-1,j-1); if (D(i-1,j) < best) best = D(i-1,j); if (D(i,j-1) < best) best = D(i,j-1)
    score = min_j D(m-1,j); end = the smallest j with that value; start = S(m-1,end)

Two forms, bit for bit the same: sdtw_loops (the definition, cell by cell) and sdtw_diagonals (one anti-diagonal at a
time, vectorised: fast enough for the tests).  sdtw() adds what the entry point adds around the recurrence: the flags
and the records of pairs that are not aligned.
"""
import numpy as np

F = np.float32
NO_START = 1                       # options
EMPTY, NONFINITE, TOO_LONG = 1, 2, 4   # flags
REC_DTYPE = np.dtype([("score", "<f4"), ("end", "<i4"), ("start", "<i4"), ("flags", "<u4")])


def last_row_loops(q, t):
    """(D(m-1, :), S(m-1, :)) by the definition; m, n >= 1, finite values"""
    q = np.asarray(q, dtype=F)
    t = np.asarray(t, dtype=F)
    m, n = q.size, t.size
    D = np.zeros((m, n), dtype=F)
    S = np.zeros((m, n), dtype=np.int64)
    with np.errstate(over="ignore"):
        for i in range(m):
            for j in range(n):
                c = F(abs(F(q[i] - t[j])))
                if i == 0:
                    D[i, j], S[i, j] = c, j
                elif j == 0:
                    D[i, j], S[i, j] = F(D[i - 1, 0] + c), S[i - 1, 0]
                else:
                    best, s = D[i - 1, j - 1], S[i - 1, j - 1]
                    if D[i - 1, j] < best:
                        best, s = D[i - 1, j], S[i - 1, j]
                    if D[i, j - 1] < best:
                        best, s = D[i, j - 1], S[i, j - 1]
                    D[i, j], S[i, j] = F(c + best), s
    return D[m - 1].copy(), S[m - 1].copy()


def last_row_diagonals(q, t):
    """the same, one anti-diagonal i + j = k at a time: its cells need diagonal k - 1 (up, left) and k - 2 (diagonal)"""
    q = np.asarray(q, dtype=F)
    t = np.asarray(t, dtype=F)
    m, n = q.size, t.size
    inf = F(np.inf)
    # index i + 1 holds row i's cell of a diagonal; index 0 stands for row -1 and is never a neighbour that is used
    d1 = np.full(m + 1, inf, dtype=F)
    d2 = np.full(m + 1, inf, dtype=F)
    s1 = np.zeros(m + 1, dtype=np.int64)
    s2 = np.zeros(m + 1, dtype=np.int64)
    rowD = np.zeros(n, dtype=F)
    rowS = np.zeros(n, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(m + n - 1):
            lo, hi = max(0, k - (n - 1)), min(m - 1, k)
            i = np.arange(lo, hi + 1)
            j = k - i
            c = np.abs(q[i] - t[j]).astype(F)
            dg, sdg = d2[i], s2[i]            # (i - 1, j - 1)
            up, sup = d1[i], s1[i]            # (i - 1, j)
            lf, slf = d1[i + 1], s1[i + 1]    # (i, j - 1)
            best, sb = dg.copy(), sdg.copy()
            w = up < best
            best[w], sb[w] = up[w], sup[w]
            w = lf < best
            best[w], sb[w] = lf[w], slf[w]
            nd = (c + best).astype(F)
            col0 = (j == 0) & (i > 0)         # D(i,0) = D(i-1,0) + c(i,0), S = S(i-1,0)
            nd[col0] = (up[col0] + c[col0]).astype(F)
            sb[col0] = sup[col0]
            row0 = i == 0                     # D(0,j) = c(0,j), S = j
            nd[row0] = c[row0]
            sb[row0] = j[row0]
            d2, s2 = d1, s1
            d1 = np.full(m + 1, inf, dtype=F)
            s1 = np.zeros(m + 1, dtype=np.int64)
            d1[i + 1], s1[i + 1] = nd, sb
            if hi == m - 1:
                rowD[k - (m - 1)], rowS[k - (m - 1)] = nd[-1], sb[-1]
    return rowD, rowS


def _pick(rowD, rowS):
    score = rowD.min()               # (no NaN among them: the values are finite, the sums at worst +inf)
    end = int(np.flatnonzero(rowD == score)[0])
    return F(score), end, int(rowS[end])


def sdtw_loops(q, t):
    """(score, end, start) by the definition"""
    return _pick(*last_row_loops(q, t))


def sdtw_diagonals(q, t):
    return _pick(*last_row_diagonals(q, t))


def sdtw(q, t, options=0, form=sdtw_diagonals, max_q=None, max_t=None):
    """the record of sgk_sdtw_f32 for one pair: (score, end, start, flags)"""
    q = np.asarray(q, dtype=F)
    t = np.asarray(t, dtype=F)
    flags = EMPTY if q.size == 0 or t.size == 0 else 0
    for x, most in ((q, max_q), (t, max_t)):
        if most is not None and x.size > most:
            flags |= TOO_LONG          # (such a read is not looked at)
        elif not np.isfinite(x).all():
            flags |= NONFINITE
    if flags:
        return F(np.nan), -1, -1, flags
    score, end, start = form(q, t)
    return score, end, (-1 if options & NO_START else start), 0


def sdtw_batch(queries, targets, options=0, form=sdtw_diagonals):
    """REC_DTYPE array [n_queries, n_targets]"""
    out = np.zeros((len(queries), len(targets)), dtype=REC_DTYPE)
    for a, q in enumerate(queries):
        for b, t in enumerate(targets):
            out[a, b] = sdtw(q, t, options, form)
    return out
