"""Referee for the exact p-values of compare_sample_sets --exact (helper module, no tests in here; it does not use the
library).

Per row, by the rules of DESIGN.md section 7, with Python integers: doubled mid-ranks from scipy.stats.rankdata, the
subset-count recurrence in dicts of Python ints, p = count / total (one float64 division of two exact integers).

Rank-sum: the kept values of the two sets, N = n1' + n2' <= 32 or the row is not eligible.  k = min(n1', n2') (set 1 on a
tie), W = the doubled rank sum of that set, D = |W - k(N+1)|, count = the number of k-subsets S of the N doubled ranks with
|sum(S) - k(N+1)| >= D, total = C(N, k) (asserted).
Signed-rank: the differences of tests/signedrank_referee.py (integer thousandths on a grid row, float32 otherwise), n'
non-zero ones, 1 <= n' <= 31 or the row is not eligible (n' = 0: p = 1, exact); doubled mid-ranks of |d|, W = the doubled
rank sum of the positive ones, D = |2W - n'(n'+1)|, count = the number of sign patterns (subsets S) with
|2 sum(S) - n'(n'+1)| >= D, total = 2^n' (asserted)."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signedrank_referee as SR  # noqa: E402

RANKSUM_MAX_N = 32
SIGNEDRANK_MAX_NP = 31


def doubled_ranks(values):
    """2 * average rank as Python ints.  float32 -> float64 is exact and keeps the order, -0.0 == 0.0, subnormals stay
    distinct, +-inf are ordinary values."""
    from scipy.stats import rankdata
    v = np.asarray(values)
    v = v.astype(np.float64) if v.dtype.kind == "f" else v.astype(np.int64)
    return [int(x) for x in np.rint(2.0 * rankdata(v)).astype(np.int64)]


@functools.lru_cache(maxsize=None)
def subset_sum_counts(ranks, k):
    """ranks: a tuple of ints -> {sum: number of k-subsets of the items with that sum}, by the recurrence
    cnt[j][s] += cnt[j-1][s - r] over the items, j descending (a pure function of its arguments, cached)"""
    cnt = [dict() for _ in range(k + 1)]
    cnt[0][0] = 1
    for r in ranks:
        for j in range(k, 0, -1):
            dst = cnt[j]
            for s, c in cnt[j - 1].items():
                dst[s + r] = dst.get(s + r, 0) + c
    return cnt[k]


@functools.lru_cache(maxsize=None)
def sign_sum_counts(ranks):
    """ranks: a tuple of ints -> {sum: number of subsets of the items with that sum} (every sign pattern once)"""
    cnt = {0: 1}
    for r in ranks:
        new = dict(cnt)
        for s, c in cnt.items():
            new[s + r] = new.get(s + r, 0) + c
        cnt = new
    return cnt


def ranksum_counts(x, y):
    """the kept float32 values of the two sets -> (count, total) as Python ints"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n1, n2 = x.size, y.size
    big_n = n1 + n2
    r = doubled_ranks(np.concatenate([x, y]))
    k = min(n1, n2)
    mine = r[:n1] if n1 <= n2 else r[n1:]
    centre = k * (big_n + 1)
    dist = abs(sum(mine) - centre)
    table = subset_sum_counts(tuple(sorted(r)), k)
    total = sum(table.values())
    assert total == math.comb(big_n, k), (total, big_n, k)
    count = sum(c for s, c in table.items() if abs(s - centre) >= dist)
    return count, total


def signedrank_counts(d):
    """the differences (zeros included) -> (n', count, total); n' = 0 -> (0, 1, 1); above 31 non-zero differences
    (n', None, None): the row is not eligible and nothing is counted"""
    d = np.asarray(d)
    d = d[d != 0]
    npairs = int(d.size)
    if npairs == 0:
        return 0, 1, 1
    if npairs > SIGNEDRANK_MAX_NP:
        return npairs, None, None
    mag = np.abs(d.astype(np.float64) if d.dtype.kind == "f" else d)
    r = doubled_ranks(mag)
    w = sum(ri for ri, di in zip(r, d) if di > 0)
    full = npairs * (npairs + 1)
    dist = abs(2 * w - full)
    table = sign_sum_counts(tuple(sorted(r)))
    total = sum(table.values())
    assert total == 2 ** npairs, (total, npairs)
    count = sum(c for s, c in table.items() if abs(2 * s - full) >= dist)
    return npairs, count, total


def ranksum_row(row, g1, g2):
    """one table row -> (eligible, p): eligible False (p None) when the row is not tested or keeps more than 32 values"""
    x, y = row[np.asarray(g1)], row[np.asarray(g2)]
    x, y = x[~np.isnan(x)], y[~np.isnan(y)]
    if x.size < 3 or y.size < 3 or x.size + y.size > RANKSUM_MAX_N:
        return False, None
    count, total = ranksum_counts(x, y)
    return True, count / total


def signedrank_row(row, a, b):
    """one table row -> (eligible, p); a tested row with n' = 0 is eligible with p = 1"""
    x, y = row[np.asarray(a)], row[np.asarray(b)]
    keep = ~(np.isnan(x) | np.isnan(y))
    x, y = x[keep], y[keep]
    if x.size < 3:
        return False, None
    d, _ = SR.differences(x, y)
    npairs, count, total = signedrank_counts(d)
    if npairs > SIGNEDRANK_MAX_NP:
        return False, None
    return True, count / total


def table_reference(ps, c1, c2, paired):
    """-> (exact uint8 [n], p float64 [n]: the exact p on eligible rows, NaN elsewhere)"""
    ps = np.asarray(ps, dtype=np.float32)
    n = ps.shape[0]
    exact, p = np.zeros(n, np.uint8), np.full(n, np.nan)
    one = signedrank_row if paired else ranksum_row
    for r in range(n):
        ok, val = one(ps[r], c1, c2)
        if ok:
            exact[r], p[r] = 1, val
    return exact, p
