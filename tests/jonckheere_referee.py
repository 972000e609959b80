"""Exact referee for the Jonckheere-Terpstra trend test (helper module, no tests in here).

J2 = 2 J, M2 = 2 E[J] and the numerator of the tie-corrected variance are Python ints computed on integer keys, Var(J) is
one fractions.Fraction, z comes from one mpmath square root and p = erfc(|z| / sqrt 2) from mpmath at 50 digits, so nothing
here rounds before the last conversion to float64.  Keys are those of kruskal_referee: 1000 * value for 3-decimal PS
values, a dense rank for arbitrary float32 values.

   J2 = sum_{i<j} sum_{x in set i, y in set j} (2 [x < y] + [x == y])       M2 = sum_{i<j} n_i n_j
   A  = N(N-1)(2N+5) - sum n_i(n_i-1)(2n_i+5) - sum t(t-1)(2t+5)
   B1 = sum n_i(n_i-1)(n_i-2)   B2 = sum t(t-1)(t-2)   C1 = sum n_i(n_i-1)   C2 = sum t(t-1)
   Var(J) = [A N(N-1)(N-2) + 2 B1 B2 + 9 (N-2) C1 C2] / [72 N(N-1)(N-2)],   z = (J2 - M2) / (2 sqrt Var)

J2 is counted by sorted prefix counts (np.searchsorted of each set in the pooled earlier sets), so a row of 16384 columns
costs a few sorts.  The float32 fields (tested, med, mean, delta) are kruskal_referee's numpy values.
"""
from fractions import Fraction

import numpy as np

import kruskal_referee as KR

DPS = 50


def exact_pieces(key_sets):
    """key_sets: one integer array per set, in the order of the sets -> dict(N, J2, M2, num, den) of Python ints; Var(J) =
    num / (72 den)"""
    key_sets = [np.asarray(g, dtype=np.int64) for g in key_sets]
    sizes = [int(g.size) for g in key_sets]
    N = sum(sizes)
    J2 = 0
    pool = np.zeros(0, np.int64)
    for g in key_sets:
        if pool.size:
            J2 += int(np.searchsorted(pool, g, side="left").sum()) + int(np.searchsorted(pool, g, side="right").sum())
        pool = np.sort(np.concatenate([pool, g]))
    M2 = (N * N - sum(m * m for m in sizes)) // 2
    ties = [int(t) for t in np.unique(pool, return_counts=True)[1]]
    A = N * (N - 1) * (2 * N + 5) - sum(m * (m - 1) * (2 * m + 5) for m in sizes) - sum(t * (t - 1) * (2 * t + 5) for t in ties)
    B1, B2 = sum(m * (m - 1) * (m - 2) for m in sizes), sum(t * (t - 1) * (t - 2) for t in ties)
    C1, C2 = sum(m * (m - 1) for m in sizes), sum(t * (t - 1) for t in ties)
    den = N * (N - 1) * (N - 2)
    return dict(N=N, J2=J2, M2=M2, num=A * den + 2 * B1 * B2 + 9 * (N - 2) * C1 * C2, den=den)


def variance(pc):
    """Var(J) of exact_pieces' result as a Fraction"""
    return Fraction(pc["num"], 72 * pc["den"])


def z_and_p(pc):
    """-> (z, p) as mpmath numbers at 50 digits; (0, 1) when the numerator is 0 (every value equal)"""
    import mpmath
    with mpmath.workdps(DPS):
        if pc["num"] == 0:
            return mpmath.mpf(0), mpmath.mpf(1)
        var = variance(pc)
        z = mpmath.mpf(pc["J2"] - pc["M2"]) / (2 * mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator)))
        return z, mpmath.erfc(abs(z) / mpmath.sqrt(2))


def key_sets_of(kept, grid):
    """the kept values of every set -> their integer keys (grid: 1000 * value, else the dense rank over the row)"""
    if grid:
        return [KR.grid_keys(v) for v in kept]
    dk = KR.dense_keys(np.concatenate(kept))
    return np.split(dk, np.cumsum([v.size for v in kept])[:-1])


def row_reference(row, sets, grid):
    """One table row (float32) and the ORDERED sets' column lists -> dict(tested, z, p, j float64, num (int), med, mean,
    delta) by the rules of compare_sample_sets; the float32 fields and `tested` are kruskal_referee's"""
    base = KR.row_reference(row, sets, grid)
    out = dict(tested=base["tested"], med=base["med"], mean=base["mean"], delta=base["delta"], z=0.0, p=0.0, j=0.0, num=0)
    if not base["tested"]:
        return out
    kept = [row[np.asarray(g)] for g in sets]
    kept = [v[~np.isnan(v)] for v in kept]
    pc = exact_pieces(key_sets_of(kept, grid))
    z, p = z_and_p(pc)
    out.update(z=float(z), p=float(p), j=pc["J2"] / 2, num=pc["num"])
    return out


def table_reference(ps, sets, grid):
    """row_reference for every row -> dict of arrays: tested, z, p, j [n], zero_num [n] (tested and numerator 0), med,
    mean [k, n], delta [n]"""
    n, k = ps.shape[0], len(sets)
    out = dict(tested=np.zeros(n, np.uint8), z=np.zeros(n), p=np.zeros(n), j=np.zeros(n), zero_num=np.zeros(n, bool),
               med=np.zeros((k, n), np.float32), mean=np.zeros((k, n), np.float32), delta=np.zeros(n, np.float32))
    for r in range(n):
        ref = row_reference(ps[r], sets, grid)
        out["tested"][r] = ref["tested"]
        out["z"][r], out["p"][r], out["j"][r] = ref["z"], ref["p"], ref["j"]
        out["zero_num"][r] = bool(ref["tested"]) and ref["num"] == 0
        out["med"][:, r], out["mean"][:, r], out["delta"][r] = ref["med"], ref["mean"], ref["delta"]
    return out


def brute_j2(key_sets):
    """J2 by counting every pair (small inputs only)"""
    j2 = 0
    for i in range(len(key_sets)):
        for j in range(i + 1, len(key_sets)):
            x, y = np.asarray(key_sets[i])[:, None], np.asarray(key_sets[j])[None, :]
            j2 += 2 * int((x < y).sum()) + int((x == y).sum())
    return j2
