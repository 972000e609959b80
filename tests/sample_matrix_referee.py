"""Referee for `sample_matrix` (helper module, no tests in here; it does not use the library).

The four integer matrices of sdice_sample_gram from numpy: the integer keys are np.rint(1000 ps) after asserting that every
value is NaN or exactly float32(k / 1000), k = 0 .. 1000; with K the keys (0 where absent), K2 their squares and V the 0/1
presence mask of the selected columns, as float64 matrices,

    shared = V'V,   sum1 = K'V,   sum2 = K2'V,   prod = K'K

by BLAS.  No entry can pass n * 10^6, which the referee asserts to be below 2^53, so every partial sum is an integer that
float64 holds and the products are exact in any order (equal to the int64 matmul on a 10 000 x 64 table).

corr and rmsd of sdice_sample_matrix_finish from Python integers and mpmath at 50 digits, rounded to float64 once.
"""
import numpy as np

DPS = 50
GRID = (np.arange(1001, dtype=np.float64) / 1000.0).astype(np.float32)      # float32(k / 1000)


def keys_of(ps):
    """float32 [n, m] -> (int64 keys, 0 where absent; bool present); asserts that every value is on the grid"""
    ps = np.asarray(ps, dtype=np.float32)
    present = ~np.isnan(ps)
    k = np.zeros(ps.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        k[present] = np.rint(ps[present].astype(np.float64) * 1000.0).astype(np.int64)
    assert np.all((k >= 0) & (k <= 1000)), "a value outside [0, 1]"
    assert np.array_equal(GRID[k][present], ps[present]), "a value off the 3-decimal grid"
    return k, present


def gram(ps, cols):
    """-> dict of int64 [m, m]: shared, sum1, sum2, prod of the columns `cols` of ps"""
    ps = np.asarray(ps, dtype=np.float32)
    k, present = keys_of(ps[:, np.asarray(cols, dtype=np.int64)])
    assert ps.shape[0] * 10 ** 6 < 2 ** 53, "the table outgrows exact float64 sums"
    K = k.astype(np.float64)
    V = present.astype(np.float64)
    out = dict(shared=V.T @ V, sum1=K.T @ V, sum2=(K * K).T @ V, prod=K.T @ K)
    for name, x in out.items():
        assert np.all(x == np.rint(x)) and x.max(initial=0) < 2 ** 53
        out[name] = x.astype(np.int64)
    return out


def finish(shared, sum1, sum2, prod, min_shared):
    """the integer matrices (anything indexable [a][b] that holds Python-convertible integers) -> (corr, rmsd) float64
    [m, m], each the 50-digit value rounded once; NaN by the rules of sdice_sample_matrix_finish"""
    import mpmath
    m = len(shared)
    corr, rmsd = np.full((m, m), np.nan), np.full((m, m), np.nan)
    with mpmath.workdps(DPS):
        for a in range(m):
            for b in range(m):
                N = int(shared[a][b])
                if N < min_shared or N == 0:
                    continue
                sa, sb = int(sum1[a][b]), int(sum1[b][a])
                va, vb = N * int(sum2[a][b]) - sa * sa, N * int(sum2[b][a]) - sb * sb
                if va > 0 and vb > 0:
                    num = N * int(prod[a][b]) - sa * sb
                    corr[a, b] = float(mpmath.mpf(num) / mpmath.sqrt(mpmath.mpf(va) * mpmath.mpf(vb)))
                sq = int(sum2[a][b]) + int(sum2[b][a]) - 2 * int(prod[a][b])
                rmsd[a, b] = float(mpmath.sqrt(mpmath.mpf(sq) / N) / 1000)
    return corr, rmsd


def random_table(rng, n, s, nan_frac=0.3):
    """float32 [n, s] of random 3-decimal PS values with about nan_frac NaN"""
    ps = GRID[rng.integers(0, 1001, size=(n, s))].copy()
    ps[rng.random((n, s)) < nan_frac] = np.nan
    return ps
