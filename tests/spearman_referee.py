"""Referee for the Spearman rank correlation of `correlate` (helper module, no tests in here; it does not use the library).

Per row, by the rules of DESIGN.md section 7: a listed sample is kept when its PS value is not NaN, the row is tested with
at least 3 kept samples; n is the kept count, mean and median are numpy's on the float32 values of the kept samples in the
order of the column list.  Both sides are ranked among the kept samples of the row with scipy.stats.rankdata (average
ranks; PS ties by float32 equality, covariate ties by float64 equality) and the ranks are doubled to integers a, b.  Then

    N = n' sum(a b) - sum(a) sum(b),   Dx = n' sum(a^2) - sum(a)^2,   Dy = n' sum(b^2) - sum(b)^2      as Python ints,
    rho = N / sqrt(Dx Dy),   1 - rho^2 = (Dx Dy - N^2) / (Dx Dy)                    (a Fraction, then mpmath at 50 digits),
    p = I_{1 - rho^2}(nu / 2, 1 / 2),   nu = n' - 2                                 (mpmath.betainc, regularized)

which is scipy's 2 t.sf(|t|, nu).  Edge rules: Dx = 0 or Dy = 0 (a constant side; scipy: NaN) -> rho = 0, p = 1, the row
stays tested; N = 0 -> rho = 0, p = 1; N^2 = Dx Dy -> rho = +-1, p = 0.
"""
from fractions import Fraction

import numpy as np

DPS = 50


def integer_pieces(x, y):
    """kept covariate values (float64) and kept PS values (float32) -> (N, Dx, Dy) as Python ints"""
    from scipy.stats import rankdata
    a = [int(v) for v in np.rint(2.0 * rankdata(np.asarray(x, np.float64)))]
    b = [int(v) for v in np.rint(2.0 * rankdata(np.asarray(y, np.float32).astype(np.float64)))]   # (exact, keeps order and ties)
    k = len(a)
    sa, sb = sum(a), sum(b)
    return (k * sum(u * v for u, v in zip(a, b)) - sa * sb, k * sum(u * u for u in a) - sa * sa,
            k * sum(v * v for v in b) - sb * sb)


def rho_and_p(k, num, dx, dy):
    """-> (rho, p) as floats (p may underflow to 0), and p as an mpmath.mpf"""
    import mpmath
    if dx == 0 or dy == 0 or num == 0:
        return 0.0, 1.0, mpmath.mpf(1)
    if num * num == dx * dy:
        return (1.0 if num > 0 else -1.0), 0.0, mpmath.mpf(0)
    one_minus = Fraction(dx * dy - num * num, dx * dy)
    with mpmath.workdps(DPS):
        rho = mpmath.mpf(num) / mpmath.sqrt(mpmath.mpf(dx * dy))
        x = mpmath.mpf(one_minus.numerator) / mpmath.mpf(one_minus.denominator)
        p = mpmath.betainc(mpmath.mpf(k - 2) / 2, mpmath.mpf(1) / 2, 0, x, regularized=True)
        return float(rho), float(p), p


def row_reference(row, cols, x):
    """One table row (float32), the column list and the covariate value of each listed column ->
    dict(tested, rho, p, n_kept, med, mean)"""
    y = np.asarray(row, np.float32)[np.asarray(cols)]
    x = np.asarray(x, np.float64)
    keep = ~np.isnan(y)
    x, y = x[keep], y[keep]
    if y.size < 3:
        return dict(tested=0, rho=0.0, p=0.0, n_kept=0, med=np.float32(0), mean=np.float32(0))
    rho, p, _ = rho_and_p(int(y.size), *integer_pieces(x, y))
    with np.errstate(over="ignore", invalid="ignore"):
        return dict(tested=1, rho=rho, p=p, n_kept=int(y.size), med=np.median(y), mean=np.float32(0) + np.mean(y))


FIELDS = (("tested", np.uint8), ("p", np.float64), ("rho", np.float64), ("n_kept", np.int32), ("med", np.float32),
          ("mean", np.float32))


def table_reference(ps, cols, x):
    """row_reference for every row -> dict of arrays [n] with the keys of engine.Context.spearman.  cols and x in the
    order the library gets them (engine.spearman_order: by covariate, ties in table order)."""
    ps = np.asarray(ps, dtype=np.float32)
    n = ps.shape[0]
    out = {name: np.zeros(n, dt) for name, dt in FIELDS}
    for r in range(n):
        ref = row_reference(ps[r], cols, x)
        for name in out:
            out[name][r] = ref[name]
    return out

