"""Referee of the paired shift and its confidence interval (sdice_walsh, include/sdice.h) by brute force over all
M = m'(m'+1)/2 Walsh sums d_i + d_j, i <= j, of the kept pairs' differences, zeros included: on a row of 3-decimal values the
differences and the sums are integers and a reported value is one division of a Python int; on any other row the
differences are numpy float32 subtractions, the sums numpy float64 additions, sorted, and a reported value is half a sum.
The rank of the interval's ends comes from mpmath at 40 digits with the zq it is given.  The grid test, the quantile, the
field list and the writer of the command's table are tests/shift_referee.py's.  Helper module: no tests in here and no
import of the package."""
import functools

import mpmath
import numpy as np

from shift_referee import FIELDS, OUTS, format_table, grid_keys, plus_zero, zq_of  # noqa: F401

DIGITS = 40
SORT_LIMIT = 1 << 20                # sums a row may have and still be sorted outright; above, np.partition


@functools.lru_cache(maxsize=None)
def rank_and_margin(m, zq):
    """-> (c = max(1, floor(M/2 - zq sqrt(m (m + 1) (2m + 1) / 24))), the distance of the floored quantity from the nearest
    integer), M = m (m + 1) / 2, at DIGITS digits with zq taken as the float64 it is"""
    with mpmath.workdps(DIGITS):
        v = mpmath.mpf(m * (m + 1)) / 4 - mpmath.mpf(zq) * mpmath.sqrt(mpmath.mpf(m * (m + 1) * (2 * m + 1)) / 24)
        return max(1, int(mpmath.floor(v))), float(abs(v - mpmath.nint(v)))


def kept_pairs(row, a, b):
    """-> (x, y) float32: the two sides of the pairs without a NaN, in pair order"""
    row = np.asarray(row, np.float32)
    x, y = row[np.asarray(a)], row[np.asarray(b)]
    keep = ~(np.isnan(x) | np.isnan(y))
    return x[keep], y[keep]


def walsh_sums(d):
    """every d_i + d_j, i <= j, of the vector d, in its dtype (int64: exact; float64: one addition each)"""
    d = np.sort(d)
    return np.concatenate([d[i] + d[i:] for i in range(d.size)])


def _order_statistics(s, ranks):
    """the 1-based order statistics `ranks` of the array s, as Python scalars"""
    if s.size <= SORT_LIMIT:
        srt = sorted(s.tolist())
        return {r: srt[r - 1] for r in ranks}
    part = np.partition(s, sorted({r - 1 for r in ranks}))
    return {r: part[r - 1].item() for r in ranks}


def row_reference(row, a, b, zq):
    """one table row (float32) and the two pair lists -> dict of FIELDS + m (the kept pairs), grid (the row is on the
    3-decimal grid)"""
    x, y = kept_pairs(row, a, b)
    m = x.size
    if m < 3:
        return dict(tested=0, shift=0.0, lo=0.0, hi=0.0, rank=0, m=m, grid=False)
    M = m * (m + 1) // 2
    c, _ = rank_and_margin(m, zq)
    ia, ib = (M + 1) // 2, M // 2 + 1
    out = dict(tested=1, rank=c, m=m)
    keys = grid_keys(np.concatenate([x, y]))
    out["grid"] = keys is not None
    if keys is not None:
        S = {r: int(v) for r, v in _order_statistics(walsh_sums(keys[:m] - keys[m:]), (ia, ib, c, M + 1 - c)).items()}
        shift = S[ia] / 2000.0 if M % 2 else (S[ia] + S[ib]) / 4000.0
        lo, hi = S[c] / 2000.0, S[M + 1 - c] / 2000.0
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            d = x - y                                                         # float32
        assert d.dtype == np.float32
        if not np.all(np.isfinite(d)):                                        # a kept infinity, or FLT_MAX - (-FLT_MAX)
            return dict(out, shift=np.nan, lo=np.nan, hi=np.nan)
        S = _order_statistics(walsh_sums(d.astype(np.float64)), (ia, ib, c, M + 1 - c))
        W = {r: 0.5 * v for r, v in S.items()}
        shift = W[ia] if M % 2 else 0.5 * (W[ia] + W[ib])
        lo, hi = W[c], W[M + 1 - c]
    return dict(out, shift=plus_zero(shift), lo=plus_zero(lo), hi=plus_zero(hi))


def table_reference(ps, a, b, zq):
    """-> name -> array over the rows: FIELDS in their dtypes, m int64, grid uint8"""
    rows = [row_reference(ps[r], a, b, zq) for r in range(ps.shape[0])]
    out = {name: np.array([r[name] for r in rows], dtype=dt) for name, dt in FIELDS}
    out["m"] = np.array([r["m"] for r in rows], dtype=np.int64)
    out["grid"] = np.array([r["grid"] for r in rows], dtype=np.uint8)
    return out
