"""Referee for the Wilcoxon signed-rank test of compare_sample_sets --paired (helper module, no tests in here; it does
not use the library).

Per row, by the rules of DESIGN.md section 7: a pair (a[q], b[q]) is kept when both values are non-NaN, the row is tested
with at least 3 kept pairs; medians and means are numpy's on the float32 values of the kept pairs in pair order.  The
differences are integers in thousandths when every kept value v of the row is a 3-decimal PS value (key = rint(1000 v) in
0..1000 and float32(key / 1000) == v), float32 subtractions otherwise.  Zero differences are dropped, 2 * average rank of
|d| comes from scipy.stats.rankdata, and

    z = (2 W2 - n'(n'+1)) / (4 sqrt(V)),   V = (n'(n'+1)(2n'+1) - sum(t^3 - t)/2) / 24 as a Fraction,

W2 = sum of the doubled ranks of the positive differences: all integers, one square root and one division in mpmath at 50
digits.  p = erfc(|z| / sqrt 2) from mpmath at 50 digits.  A tested row without a non-zero difference: z = 0, p = 1.
"""
from fractions import Fraction

import numpy as np

DPS = 50


def grid_keys(values):
    """-> integer keys when every float32 value is float32(key / 1000), key = 0..1000, else None"""
    v = np.asarray(values, dtype=np.float32)
    key = np.rint(v.astype(np.float64) * 1000.0)
    with np.errstate(invalid="ignore"):
        ok = (key >= 0) & (key <= 1000) & ((key / 1000.0).astype(np.float32) == v)
    return key.astype(np.int64) if bool(np.all(ok)) else None


def differences(x, y):
    """the kept pairs' float32 values -> (d, is_grid): int64 thousandths on a grid row, float32 x - y otherwise"""
    kx, ky = grid_keys(x), grid_keys(y)
    if kx is not None and ky is not None:
        return kx - ky, True
    with np.errstate(over="ignore"):
        return (np.asarray(x, np.float32) - np.asarray(y, np.float32)).astype(np.float32), False


def integer_pieces(d):
    """differences -> (n', W2, sum(t^3 - t)) as Python ints"""
    from scipy.stats import rankdata
    d = d[d != 0]
    npairs = int(d.size)
    if npairs == 0:
        return 0, 0, 0
    mag = np.abs(d.astype(np.float64) if d.dtype.kind == "f" else d)     # (float32 -> float64 is exact and keeps the order)
    r2 = np.rint(2.0 * rankdata(mag)).astype(np.int64)
    w2 = int(r2[d > 0].sum())
    _, cnt = np.unique(mag, return_counts=True)
    tie = sum(int(t) ** 3 - int(t) for t in cnt)
    return npairs, w2, tie


def z_and_p(npairs, w2, tie):
    """-> (z, p) as floats (p may underflow to 0), and p as an mpmath.mpf"""
    import mpmath
    if npairs == 0:
        return 0.0, 1.0, mpmath.mpf(1)
    nn = npairs * (npairs + 1)
    num = 2 * w2 - nn
    var = (Fraction(nn * (2 * npairs + 1)) - Fraction(tie, 2)) / 24
    with mpmath.workdps(DPS):
        z = mpmath.mpf(num) / (4 * mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator)))
        p = mpmath.erfc(abs(z) / mpmath.sqrt(2))
        return float(z), float(p), p


def row_reference(row, a, b):
    """One table row (float32) and the pair lists -> dict(tested, z, p, med1, med2, mean1, mean2, delta, grid, npairs)"""
    x, y = row[np.asarray(a)], row[np.asarray(b)]
    keep = ~(np.isnan(x) | np.isnan(y))
    x, y = x[keep], y[keep]
    zero = np.float32(0)
    if x.size < 3:
        return dict(tested=0, z=0.0, p=0.0, med1=zero, med2=zero, mean1=zero, mean2=zero, delta=zero, grid=False, npairs=0)
    d, grid = differences(x, y)
    npairs, w2, tie = integer_pieces(d)
    z, p, _ = z_and_p(npairs, w2, tie)
    with np.errstate(over="ignore", invalid="ignore"):
        med1, med2 = np.median(x), np.median(y)
        return dict(tested=1, z=z, p=p, med1=med1, med2=med2, mean1=np.mean(x), mean2=np.mean(y),
                    delta=np.float32(med1 - med2), grid=grid, npairs=npairs)


FIELDS = (("tested", np.uint8), ("p", np.float64), ("z", np.float64), ("med1", np.float32), ("med2", np.float32),
          ("mean1", np.float32), ("mean2", np.float32), ("delta", np.float32))


def table_reference(ps, a, b):
    """row_reference for every row -> dict of arrays [n] with the keys of engine.Context.signedrank (+ grid, npairs)"""
    ps = np.asarray(ps, dtype=np.float32)
    n = ps.shape[0]
    out = {name: np.zeros(n, dt) for name, dt in FIELDS}
    out["grid"] = np.zeros(n, bool)
    out["npairs"] = np.zeros(n, np.int64)
    for r in range(n):
        ref = row_reference(ps[r], a, b)
        for name in out:
            out[name][r] = ref[name]
    return out
