"""Referee of the two-sample Kolmogorov-Smirnov test (sdice_ks, include/sdice.h), pure Python on float32 arrays: M by its
definition, D as a Fraction, the exact conditional p by the path recurrence in Python ints, the asymptotic p by the two
series of Kolmogorov's limiting distribution in mpmath at 50 digits.  Helper module: no tests in here and no import of
the package."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

EXACT_MAX = 32                      # kept values of a row the exact form takes
FIELDS = (("tested", np.uint8), ("p", np.float64), ("d", np.float64), ("med1", np.float32), ("med2", np.float32),
          ("mean1", np.float32), ("mean2", np.float32), ("delta", np.float32), ("exact", np.uint8))
DIGITS = 50


def kept(values):
    v = np.asarray(values, np.float32)
    return v[~np.isnan(v)]


def statistic(x, y):
    """kept float32 values of the two groups -> (M, T): M = max over the distinct values v of |c1(v) n2 - c2(v) n1|, c(v)
    = #{values <= v} by float32 comparison (-0.0 == +0.0); T = the tie-run ends of the merged order as cumulative counts"""
    x, y = np.sort(np.asarray(x, np.float32)), np.sort(np.asarray(y, np.float32))
    n1, n2 = x.size, y.size
    vals = np.unique(np.concatenate([x, y]))            # (sorted; -0.0 and +0.0 compare equal and are one value)
    c1 = np.searchsorted(x, vals, side="right").astype(np.int64)
    c2 = np.searchsorted(y, vals, side="right").astype(np.int64)
    return int(np.abs(c1 * n2 - c2 * n1).max()), [int(t) for t in c1 + c2]


def statistic_plain(x, y):
    """the definition again, one value at a time in Python (the check of statistic() on small rows)"""
    x, y = [np.float32(v) for v in x], [np.float32(v) for v in y]
    best, ends = 0, set()
    for v in x + y:
        c1, c2 = sum(1 for a in x if a <= v), sum(1 for b in y if b <= v)
        best = max(best, abs(c1 * len(y) - c2 * len(x)))
        ends.add(c1 + c2)
    return best, sorted(ends)


def exact_p(M, n1, n2, T):
    """the conditional permutation probability given the ties -> Fraction: cnt_t[i] = cnt_{t-1}[i] + cnt_{t-1}[i-1] over
    the lattice 0 <= i <= n1, 0 <= t - i <= n2, zeroed at a checkpoint t in T where |i n2 - (t - i) n1| >= M"""
    N, ends = n1 + n2, set(T)
    assert N in ends
    cnt = [1] + [0] * n1
    for t in range(1, N + 1):
        new = [0] * (n1 + 1)
        for i in range(max(0, t - n2), min(t, n1) + 1):
            new[i] = cnt[i] + (cnt[i - 1] if i else 0)
            if t in ends and abs(i * n2 - (t - i) * n1) >= M:
                new[i] = 0
        cnt = new
    total = math.comb(N, n1)
    return Fraction(total - cnt[n1], total)


def _alternating(lam2):
    total, k = mpmath.mpf(0), 1
    while True:
        term = mpmath.exp(-2 * k * k * lam2)
        total += term if k % 2 else -term
        if k > 1 and term < mpmath.mpf(10) ** (-DIGITS - 10) * mpmath.exp(-2 * lam2):
            return 2 * total
        k += 1


def _dual(lam2):
    total, k = mpmath.mpf(0), 1
    while True:
        term = mpmath.exp(-((2 * k - 1) ** 2) * mpmath.pi ** 2 / (8 * lam2))
        total += term
        if k > 1 and (term == 0 or term < mpmath.mpf(10) ** (-DIGITS - 10)):
            return 1 - mpmath.sqrt(2 * mpmath.pi / lam2) * total
        k += 1


def kolmogorov_mp(lam2, form=None):
    """Kolmogorov's limiting survival function at lambda^2 = lam2 (an mpf or a Fraction) -> mpf at DIGITS + 30 working
    digits: 2 sum (-1)^(k-1) exp(-2 k^2 lam2) (form "alternating"), or Jacobi's dual 1 - sqrt(2 pi / lam2) sum exp(-(2k -
    1)^2 pi^2 / (8 lam2)) (form "dual"); by default the one that converges fast at lam2"""
    with mpmath.workdps(DIGITS + 30):
        lam2 = mpmath.mpf(lam2.numerator) / lam2.denominator if isinstance(lam2, Fraction) else mpmath.mpf(lam2)
        if lam2 == 0:
            return mpmath.mpf(1)
        if form is None:
            form = "alternating" if lam2 >= 1 else "dual"
        return +(_alternating(lam2) if form == "alternating" else _dual(lam2))


@functools.lru_cache(maxsize=None)
def asymptotic_p(M, n1, n2):
    """-> float64 nearest to min(1, Kolmogorov(lam2)), lam2 = M^2 / (n1 n2 (n1 + n2)) as an exact quotient"""
    if M == 0:
        return 1.0
    p = kolmogorov_mp(Fraction(M * M, n1 * n2 * (n1 + n2)))
    return float(min(p, mpmath.mpf(1)))


def row_reference(row, g1, g2, want_exact=True):
    """one table row (float32) and the two column lists -> dict of FIELDS + M, n1, n2 (kept counts), p_asym and p_exact (a
    Fraction, None where the row is not eligible whatever want_exact says)"""
    row = np.asarray(row, np.float32)
    x, y = kept(row[np.asarray(g1)]), kept(row[np.asarray(g2)])
    n1, n2 = x.size, y.size
    zero = np.float32(0)
    if n1 < 3 or n2 < 3:
        return dict(tested=0, p=0.0, d=0.0, med1=zero, med2=zero, mean1=zero, mean2=zero, delta=zero, exact=0, M=0, n1=n1,
                    n2=n2, p_asym=0.0, p_exact=None)
    M, T = statistic(x, y)
    p_asym = asymptotic_p(M, n1, n2)
    p_exact = exact_p(M, n1, n2, T) if n1 + n2 <= EXACT_MAX else None
    use = want_exact and p_exact is not None
    with np.errstate(over="ignore", invalid="ignore"):
        med1, med2 = np.median(x), np.median(y)
        return dict(tested=1, p=float(p_exact) if use else p_asym, d=float(Fraction(M, n1 * n2)), med1=med1, med2=med2,
                    mean1=np.mean(x), mean2=np.mean(y), delta=np.float32(med1 - med2), exact=int(use), M=M, n1=n1, n2=n2,
                    p_asym=p_asym, p_exact=p_exact)


def table_reference(ps, g1, g2, want_exact=True):
    """-> name -> array over the rows: FIELDS in their dtypes, M, n1, n2 int64, p_asym float64, eligible uint8"""
    rows = [row_reference(ps[r], g1, g2, want_exact) for r in range(ps.shape[0])]
    out = {name: np.array([r[name] for r in rows], dtype=dt) for name, dt in FIELDS}
    for name in ("M", "n1", "n2"):
        out[name] = np.array([r[name] for r in rows], dtype=np.int64)
    out["p_asym"] = np.array([r["p_asym"] for r in rows], dtype=np.float64)
    out["eligible"] = np.array([r["p_exact"] is not None for r in rows], dtype=np.uint8)
    return out
