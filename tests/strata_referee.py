"""Referee for the stratified rank-sum test of compare_sample_sets --strata (van Elteren; helper module, no tests in
here; it does not use the library).

Per row, by the rules of include/sdice.h: per stratum h the values at the group-1 and at the group-2 columns of h with NaNs
dropped; a stratum with a kept value on both sides is informative.  Inside one, from integer keys that order and tie as
the values do (grid_keys: thousandths on a row of 3-decimal PS values, dense ranks otherwise, as tests/kruskal_referee.py),

    r2 = 2 #{x < v} + #{x == v} + 1,  D_h = sum r2 over group 1 - n1h (N_h + 1),  T_h = sum t^3 - t,
    d_h = D_h / (2 (N_h + 1)),  V_h = n1h n2h (N_h^3 - N_h - T_h) / (12 N_h (N_h - 1) (N_h + 1)^2)

as fractions.Fraction: sum d_h and sum V_h carry no rounding at all.  z = sign * sqrt of the exact z^2 = (sum d_h)^2 /
sum V_h by mpmath at 50 digits, p = mpmath erfc(|z| / sqrt 2) at 50 digits, converted to float.  cond = sum |d_h| /
sqrt(sum V_h) is what a float64 summation of the d_h can lose to cancellation, in units of its rounding error.  The row is
tested when the informative strata keep >= 3 values on both sides; sum V_h = 0 gives z = 0, p = 1.  Float32 fields are
numpy's over ALL kept values of a group in list order.
"""
from fractions import Fraction

import numpy as np

from kruskal_referee import dense_keys, grid_keys

DPS = 50
FIELDS = (("tested", np.uint8), ("p", np.float64), ("z", np.float64), ("med1", np.float32), ("med2", np.float32),
          ("mean1", np.float32), ("mean2", np.float32), ("delta", np.float32))


def is_grid(values):
    """every float32 value is float32(key / 1000), key = 0..1000"""
    v = np.asarray(values, dtype=np.float32)
    key = np.rint(v.astype(np.float64) * 1000.0)
    with np.errstate(invalid="ignore"):
        return bool(np.all((key >= 0) & (key <= 1000) & ((key / 1000.0).astype(np.float32) == v)))


def stratum_pieces(k1, k2):
    """the integer keys of a stratum's two sides -> (n1h, n2h, D_h, T_h) as Python ints"""
    allk = np.concatenate([k1, k2])
    _, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
    before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    r2 = (2 * before + cnt + 1)[inv]
    n1h, n2h = int(k1.size), int(k2.size)
    D = int(r2[:n1h].sum()) - n1h * (n1h + n2h + 1)
    T = sum(int(t) ** 3 - int(t) for t in cnt)
    return n1h, n2h, D, T


def exact_sums(strata_keys):
    """[(keys of side 1, keys of side 2)] per stratum -> (sum d_h, sum V_h, sum |d_h|) as Fractions, n1', n2' over the
    informative strata"""
    sd, sv, sa, n1, n2 = Fraction(0), Fraction(0), Fraction(0), 0, 0
    for k1, k2 in strata_keys:
        if k1.size < 1 or k2.size < 1:
            continue
        n1h, n2h, D, T = stratum_pieces(k1, k2)
        N = n1h + n2h
        d = Fraction(D, 2 * (N + 1))
        sd += d
        sa += abs(d)
        sv += Fraction(n1h * n2h * (N ** 3 - N - T), 12 * N * (N - 1) * (N + 1) ** 2)
        n1 += n1h
        n2 += n2h
    return sd, sv, sa, n1, n2


def z_p_cond(sd, sv, sa):
    """the exact sums -> (z, p, cond) as floats (p may underflow to 0), z2 = the exact z^2 as a Fraction"""
    import mpmath
    if sv == 0:
        return 0.0, 1.0, 0.0, Fraction(0)
    z2 = sd * sd / sv
    with mpmath.workdps(DPS):
        root = mpmath.sqrt(mpmath.mpf(z2.numerator) / mpmath.mpf(z2.denominator))
        z = root if sd >= 0 else -root
        p = mpmath.erfc(root / mpmath.sqrt(2))
        c2 = sa * sa / sv
        cond = mpmath.sqrt(mpmath.mpf(c2.numerator) / mpmath.mpf(c2.denominator))
        return float(z), float(p), float(cond), z2


def row_keys(row, g1, g2, strat1, strat2):
    """-> (kept values of side 1, of side 2 in list order, [(keys1, keys2)] per stratum id 0..max, grid)"""
    g1, g2, strat1, strat2 = (np.asarray(v) for v in (g1, g2, strat1, strat2))
    x, y = row[g1], row[g2]
    k1, k2 = ~np.isnan(x), ~np.isnan(y)
    x, y, s1, s2 = x[k1], y[k2], strat1[k1], strat2[k2]
    both = np.concatenate([x, y])
    grid = is_grid(both)
    keys = grid_keys(both) if grid else dense_keys(both)
    kx, ky = keys[:x.size], keys[x.size:]
    H = int(max(strat1.max(initial=-1), strat2.max(initial=-1))) + 1
    return x, y, [(kx[s1 == h], ky[s2 == h]) for h in range(H)], grid


def row_reference(row, g1, g2, strat1, strat2):
    """One table row (float32), the column lists and their stratum ids -> dict(tested, z, p, med1, med2, mean1, mean2,
    delta, cond, grid, z2)"""
    x, y, strata_keys, grid = row_keys(np.asarray(row, np.float32), g1, g2, strat1, strat2)
    sd, sv, sa, n1, n2 = exact_sums(strata_keys)
    zero = np.float32(0)
    if n1 < 3 or n2 < 3:
        return dict(tested=0, z=0.0, p=0.0, med1=zero, med2=zero, mean1=zero, mean2=zero, delta=zero, cond=0.0, grid=grid,
                    z2=Fraction(0))
    z, p, cond, z2 = z_p_cond(sd, sv, sa)
    with np.errstate(over="ignore", invalid="ignore"):
        med1, med2 = np.median(x), np.median(y)
        return dict(tested=1, z=z, p=p, med1=med1, med2=med2, mean1=np.mean(x), mean2=np.mean(y),
                    delta=np.float32(med1 - med2), cond=cond, grid=grid, z2=z2)


def table_reference(ps, g1, g2, strat1, strat2):
    """row_reference for every row -> dict of arrays [n] with the keys of engine.Context.ranksum_strata (+ cond, grid)"""
    ps = np.asarray(ps, dtype=np.float32)
    n = ps.shape[0]
    out = {name: np.zeros(n, dt) for name, dt in FIELDS}
    out["cond"] = np.zeros(n)
    out["grid"] = np.zeros(n, bool)
    for r in range(n):
        ref = row_reference(ps[r], g1, g2, strat1, strat2)
        for name in out:
            out[name][r] = ref[name]
    return out
