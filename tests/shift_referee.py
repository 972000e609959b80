"""Referee of the Hodges-Lehmann shift and its confidence interval (sdice_shift, include/sdice.h) by brute force over all
n1' n2' differences: on a row of 3-decimal values the differences are integers (thousandths) and a reported value is one
float64 division; on any other row they are numpy float64 subtractions, sorted.  The rank of the interval's ends comes
from mpmath at 40 digits with the zq it is given.  Also the writer of the command's table.  Helper module: no tests in
here and no import of the package."""
import functools
import statistics

import mpmath
import numpy as np

FIELDS = (("tested", np.uint8), ("shift", np.float64), ("lo", np.float64), ("hi", np.float64), ("rank", np.int32))
OUTS = tuple(name for name, _ in FIELDS)
DIGITS = 40
SORT_LIMIT = 1 << 20                # differences a row may have and still be sorted outright; above, np.partition


def zq_of(conf):
    """the standard normal quantile at 1 - (1 - conf) / 2, as the product computes it"""
    return statistics.NormalDist().inv_cdf(1.0 - (1.0 - conf) / 2.0)


@functools.lru_cache(maxsize=None)
def rank_and_margin(n1, n2, zq):
    """-> (c = max(1, floor(M/2 - zq sqrt(M (N + 1) / 12))), the distance of the floored quantity from the nearest integer),
    M = n1 n2, N = n1 + n2, at DIGITS digits with zq taken as the float64 it is"""
    with mpmath.workdps(DIGITS):
        M, N = n1 * n2, n1 + n2
        v = mpmath.mpf(M) / 2 - mpmath.mpf(zq) * mpmath.sqrt(mpmath.mpf(M * (N + 1)) / 12)
        return max(1, int(mpmath.floor(v))), float(abs(v - mpmath.nint(v)))


def kept(values):
    v = np.asarray(values, np.float32)
    return v[~np.isnan(v)]


def grid_keys(v):
    """kept float32 values -> their integer keys when every one is float32(key / 1000.0) for a key in 0..1000, else None"""
    v = np.asarray(v, np.float32)
    if not np.all(np.isfinite(v)):
        return None
    k = np.rint(v.astype(np.float64) * 1000.0)
    if np.any(k < 0) or np.any(k > 1000) or np.any((k / 1000.0).astype(np.float32) != v):
        return None
    return k.astype(np.int64)


def _order_statistics(d, ranks):
    """the 1-based order statistics `ranks` of the array d"""
    idx = sorted({r - 1 for r in ranks})
    if d.size <= SORT_LIMIT:
        s = sorted(d.tolist())
        return {r: s[r - 1] for r in ranks}
    part = np.partition(d, idx)
    return {r: part[r - 1].item() for r in ranks}


def plus_zero(v):
    return v + 0.0


def row_reference(row, g1, g2, zq):
    """one table row (float32) and the two column lists -> dict of FIELDS + n1, n2 (the kept counts), grid (the row is on
    the 3-decimal grid)"""
    row = np.asarray(row, np.float32)
    x, y = kept(row[np.asarray(g1)]), kept(row[np.asarray(g2)])
    n1, n2 = x.size, y.size
    if n1 < 3 or n2 < 3:
        return dict(tested=0, shift=0.0, lo=0.0, hi=0.0, rank=0, n1=n1, n2=n2, grid=False)
    M = n1 * n2
    c, _ = rank_and_margin(n1, n2, zq)
    a, b = (M + 1) // 2, M // 2 + 1
    out = dict(tested=1, rank=c, n1=n1, n2=n2)
    keys = grid_keys(np.concatenate([x, y]))
    out["grid"] = keys is not None
    if np.any(np.isinf(x)) or np.any(np.isinf(y)):
        return dict(out, shift=np.nan, lo=np.nan, hi=np.nan)
    if keys is not None:
        d = (keys[:n1, None] - keys[None, n1:]).reshape(-1)                  # exact integers
        D = {r: int(v) for r, v in _order_statistics(d, (a, b, c, M + 1 - c)).items()}
        shift = D[a] / 1000.0 if M % 2 else (D[a] + D[b]) / 2000.0
        lo, hi = D[c] / 1000.0, D[M + 1 - c] / 1000.0
    else:
        d = (x.astype(np.float64)[:, None] - y.astype(np.float64)[None, :]).reshape(-1)
        D = _order_statistics(d, (a, b, c, M + 1 - c))
        shift = D[a] if M % 2 else 0.5 * (D[a] + D[b])
        lo, hi = D[c], D[M + 1 - c]
    return dict(out, shift=plus_zero(shift), lo=plus_zero(lo), hi=plus_zero(hi))


def table_reference(ps, g1, g2, zq):
    """-> name -> array over the rows: FIELDS in their dtypes, n1, n2 int64, grid uint8"""
    rows = [row_reference(ps[r], g1, g2, zq) for r in range(ps.shape[0])]
    out = {name: np.array([r[name] for r in rows], dtype=dt) for name, dt in FIELDS}
    for name in ("n1", "n2"):
        out[name] = np.array([r[name] for r in rows], dtype=np.int64)
    out["grid"] = np.array([r["grid"] for r in rows], dtype=np.uint8)
    return out


def format_table(names, keep, plain, shift, q, suffixes=None, annotated=False):
    """the command's table: plain = the rank-sum call's per-row fields (mean1, mean2, med1, med2 and delta float32, p
    float64), shift = table_reference()'s, q = the corrected p of the kept rows; cells as numpy prints its scalars"""
    lines = ["event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tshift\tshift_lo\tshift_hi\tp-value\tcorrected" +
             ("\tgene\toverlapping\ttranscript_id" if annotated else "")]
    for i, r in enumerate(keep):
        cells = [plain["mean1"][r], plain["mean2"][r], plain["med1"][r], plain["med2"][r], plain["delta"][r],
                 np.float64(shift["shift"][r]), np.float64(shift["lo"][r]), np.float64(shift["hi"][r]),
                 np.float64(plain["p"][r]), np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + (suffixes[i] if suffixes else ""))
    return "\n".join(lines) + "\n"
