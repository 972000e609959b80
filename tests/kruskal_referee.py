"""Exact referee for the Kruskal-Wallis tests (helper module, no tests in here).

H comes from the textbook definition evaluated in rational arithmetic (fractions.Fraction) on integer keys, so it has
no rounding at all; p = scipy.stats.chi2.sf(float(H), k - 1).  Keys are any integers that order the values the way the
values order: 1000 * value for 3-decimal PS values, a dense rank for arbitrary float32 values.

The float32 fields are numpy's own (np.mean, np.median).  numpy_sum() restates the order np.sum adds a contiguous float32
array in, so that the tests can show what the kernels have to reproduce; p_exact() is chi2.sf from mpmath at 50 digits,
the licence for scipy's chi2.sf as the p referee.
"""
from fractions import Fraction

import numpy as np

from rank_support import tree_sum

SUM_PIECE = 8192        # np.getbufsize(): add.reduce hands the pairwise loop at most this many elements at a time


def numpy_sum(a):
    """np.sum of a contiguous 1-D float32 array restated: pieces of SUM_PIECE values, each summed by numpy's pairwise
    tree (tree_sum of rank_support), the pieces added left to right onto the identity 0"""
    total = np.float32(0.0)
    for at in range(0, a.size, SUM_PIECE):
        total = np.float32(total + tree_sum(a[at: at + SUM_PIECE]))
    return total


def p_exact(h, df):
    """chi2.sf(h, df) of an exact H (a Fraction) as the regularised upper incomplete gamma function Q(df / 2, h / 2),
    evaluated by mpmath at 50 digits -> mpmath.mpf (far below the float64 range where H is large)"""
    import mpmath
    with mpmath.workdps(50):
        x = mpmath.mpf(h.numerator) / mpmath.mpf(h.denominator) / 2
        return mpmath.gammainc(mpmath.mpf(df) / 2, x, mpmath.inf, regularized=True)


def grid_keys(values):
    """integer keys of float32(k / 1000.0) values"""
    return np.rint(np.asarray(values, dtype=np.float64) * 1000.0).astype(np.int64)


def dense_keys(values):
    """dense rank of arbitrary float32 values (equal values, equal keys)"""
    return np.unique(np.asarray(values, dtype=np.float32), return_inverse=True)[1].astype(np.int64)


def exact_h(key_sets):
    """key_sets: one integer array per set -> the Kruskal-Wallis H with tie correction as a Fraction; None when every
    value is the same (the tie term is 0 there: scipy raises, the engine reports H = 0, p = 1)"""
    allk = np.concatenate(key_sets)
    N = int(allk.size)
    uniq, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
    before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    twice_rank = 2 * before + cnt + 1                       # 2 * average rank of every distinct value: an integer
    tie = sum(int(t) ** 3 - int(t) for t in cnt)
    if tie == N ** 3 - N:
        return None
    total = Fraction(0)
    at = 0
    for g in key_sets:
        r = Fraction(int(twice_rank[inv[at: at + g.size]].sum()), 2)
        total += r * r / int(g.size)
        at += g.size
    h = Fraction(12, N * (N + 1)) * total - 3 * (N + 1)
    return h / (1 - Fraction(tie, N ** 3 - N))


def row_reference(row, sets, grid):
    """One table row (float32) and the sets' column lists -> dict(tested, h (Fraction), hf, p, med, mean, delta) by the rules
    of compare_sample_sets: NaNs dropped per set, tested when every set keeps >= 3 values; numpy for the float32 fields."""
    from scipy.stats import chi2
    k = len(sets)
    kept = []
    for g in sets:
        v = row[np.asarray(g)]
        kept.append(v[~np.isnan(v)])
    if any(v.size < 3 for v in kept):
        return dict(tested=0, h=Fraction(0), hf=0.0, p=0.0, med=np.zeros(k, np.float32), mean=np.zeros(k, np.float32),
                    delta=np.float32(0))
    if grid:
        key_sets = [grid_keys(v) for v in kept]
    else:
        dk = dense_keys(np.concatenate(kept))
        cuts = np.cumsum([v.size for v in kept])[:-1]
        key_sets = np.split(dk, cuts)
    h = exact_h(key_sets)
    if h is None:
        h, p = Fraction(0), 1.0
    else:
        p = float(chi2.sf(float(h), k - 1))
    med = np.array([np.median(v) for v in kept], dtype=np.float32)
    mean = np.array([np.mean(v) for v in kept], dtype=np.float32)
    return dict(tested=1, h=h, hf=float(h), p=p, med=med, mean=mean, delta=np.float32(med.max() - med.min()))


def table_reference(ps, sets, grid):
    """row_reference for every row -> dict of arrays: tested [n], hf, p [n], med, mean [k, n], delta [n]"""
    n, k = ps.shape[0], len(sets)
    out = dict(tested=np.zeros(n, np.uint8), hf=np.zeros(n), p=np.zeros(n), med=np.zeros((k, n), np.float32),
               mean=np.zeros((k, n), np.float32), delta=np.zeros(n, np.float32))
    for r in range(n):
        ref = row_reference(ps[r], sets, grid)
        out["tested"][r] = ref["tested"]
        out["hf"][r], out["p"][r] = ref["hf"], ref["p"]
        out["med"][:, r], out["mean"][:, r], out["delta"][r] = ref["med"], ref["mean"], ref["delta"]
    return out
