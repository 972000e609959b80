"""Exact referee for Friedman's test and Page's L test over k matched sets (helper module, no tests in here).

Everything up to the last division is a Python / numpy integer (include/sdice.h, sdice_friedman):
  r2(q, j) = 2 #{l: x_ql < x_qj} + #{l: x_ql == x_qj} + 1,  D_j = sum_q r2 - m'(k + 1),  C = sum (t^3 - t),
  den = m'(k^3 - k) - C;  Q = 3 (k - 1) sum D^2 / den,  W = 3 sum D^2 / (m' den);  A = 6 sum (j + 1) D_j,  B = k (k + 1) den,
  z = A / sqrt(B),  L = sum (j + 1) R_j.
Q and W are Fractions and their float64 is the correctly rounded one; z is A / sqrt(B) from mpmath at 50 digits, rounded
once; p at 50 digits: the regularised upper incomplete gamma function for Friedman, erfc for Page.  The float32 fields
are numpy's own (np.mean, np.median) over the kept blocks in subject order.  table_reference() works on whole tables:
the integers by numpy (int64: every bound of the header holds with room), one mpmath evaluation per distinct integer
tuple."""
from fractions import Fraction

import numpy as np

MAX_SETS, MAX_BLOCKS, MAX_N = 64, 4096, 16384


def integers(X):
    """X float32 [..., k, m'] without NaN -> (r2sum [..., k], C [...]) int64: the per-set sums of twice the mid-ranks inside
    the blocks and the tie term"""
    X = np.asarray(X, np.float32)
    lt = np.zeros(X.shape, np.int64)
    eq = np.zeros(X.shape, np.int64)
    for l in range(X.shape[-2]):                # (a loop over the sets: [.., k, k, m'] at once is too much memory)
        y = X[..., l:l + 1, :]
        lt += y < X
        eq += y == X
    return (2 * lt + eq + 1).sum(axis=-1), (eq * eq - 1).sum(axis=(-1, -2))


def pieces(r2sum, C, k, mk):
    """-> dict of Python ints of one row: D (list), S = sum D^2, den, A, B, L2 = 2 L"""
    D = [int(v) - mk * (k + 1) for v in r2sum]
    den = mk * (k ** 3 - k) - int(C)
    return dict(D=D, S=sum(d * d for d in D), den=den, A=6 * sum((j + 1) * d for j, d in enumerate(D)), B=k * (k + 1) * den,
                L2=sum((j + 1) * int(v) for j, v in enumerate(r2sum)))


def friedman_exact(S, den, k, mk):
    """-> (Q, W) as Fractions; (0, 0) when every kept block is fully tied"""
    if den == 0:
        return Fraction(0), Fraction(0)
    return Fraction(3 * (k - 1) * S, den), Fraction(3 * S, mk * den)


_cache = {}


def p_friedman(S, den, k):
    """chi2.sf(Q, k - 1) of the exact Q at 50 digits -> mpmath.mpf"""
    import mpmath
    key = ("f", S, den, k)
    if key not in _cache:
        with mpmath.workdps(50):
            if den == 0:
                _cache[key] = mpmath.mpf(1)
            else:
                x = mpmath.mpf(3 * (k - 1) * S) / mpmath.mpf(den) / 2
                _cache[key] = mpmath.gammainc(mpmath.mpf(k - 1) / 2, x, mpmath.inf, regularized=True)
    return _cache[key]


def z_page(A, B):
    """-> (z float64: the correctly rounded A / sqrt(B), p = erfc(|A| / sqrt(2 B)) as mpmath.mpf at 50 digits); (0.0, 1) for
    A == 0 or B == 0"""
    import mpmath
    key = ("p", A, B)
    if key not in _cache:
        with mpmath.workdps(50):
            if A == 0 or B == 0:
                _cache[key] = (0.0, mpmath.mpf(1))
            else:
                z = mpmath.mpf(A) / mpmath.sqrt(mpmath.mpf(B))
                _cache[key] = (float(z), mpmath.erfc(abs(z) / mpmath.sqrt(2)))
    return _cache[key]


def kept_blocks(row, sets):
    """one table row and the k matched column lists -> (X float32 [k, m'] of the kept blocks in subject order, m')"""
    X = np.asarray(row, np.float32)[np.asarray(sets)]
    X = X[:, ~np.isnan(X).any(axis=0)]
    return X, X.shape[1]


FIELDS = ("tested", "blocks", "q", "w", "p_friedman", "z", "l", "p_page", "med", "mean", "delta")


def table_reference(ps, sets, summaries=True):
    """every row of a table -> dict of arrays: tested uint8, blocks int32, q, w, z, l float64 [n], p_friedman, p_page float64
    [n] (the 50-digit values rounded once; 0.0 past the float64 range), med, mean float32 [k, n], delta float32 [n]; 0 where
    not tested.  summaries=False skips the per-row numpy means and medians (left 0)."""
    ps = np.asarray(ps, np.float32)
    sets = np.asarray(sets)
    n, (k, m) = ps.shape[0], sets.shape
    out = dict(tested=np.zeros(n, np.uint8), blocks=np.zeros(n, np.int32), q=np.zeros(n), w=np.zeros(n), z=np.zeros(n),
               l=np.zeros(n), p_friedman=np.zeros(n), p_page=np.zeros(n),
               med=np.zeros((k, n), np.float32), mean=np.zeros((k, n), np.float32), delta=np.zeros(n, np.float32))
    X = ps[:, sets.reshape(-1)].reshape(n, k, m)
    keep = ~np.isnan(X).any(axis=1)                              # [n, m]
    mk = keep.sum(axis=1)
    full = np.flatnonzero(mk == m) if m >= 3 else np.zeros(0, np.int64)
    r2 = np.zeros((n, k), np.int64)
    C = np.zeros(n, np.int64)
    for at in range(0, full.size, 4096):                         # rows without a NaN: the integers of many rows at once
        rows = full[at: at + 4096]
        r2[rows], C[rows] = integers(X[rows])
    for r in np.flatnonzero((mk >= 3) & (mk < m)):
        r2[r], C[r] = integers(X[r][:, keep[r]])
    for r in np.flatnonzero(mk >= 3):
        mr = int(mk[r])
        pc = pieces(r2[r], C[r], k, mr)
        Q, W = friedman_exact(pc["S"], pc["den"], k, mr)
        out["tested"][r], out["blocks"][r] = 1, mr
        out["q"][r], out["w"][r] = float(Q), float(W)
        out["p_friedman"][r] = float(p_friedman(pc["S"], pc["den"], k))
        out["z"][r], p_page = z_page(pc["A"], pc["B"])
        out["p_page"][r] = float(p_page)
        out["l"][r] = pc["L2"] / 2
        if summaries:
            Xr = X[r][:, keep[r]]
            med = np.array([np.median(np.ascontiguousarray(v)) for v in Xr], np.float32)
            out["med"][:, r] = med
            out["mean"][:, r] = [np.mean(np.ascontiguousarray(v)) for v in Xr]
            out["delta"][r] = np.float32(med.max() - med.min())
    return out


def command_header(k, trend, gtf=False):
    """the header cells of compare_sample_sets --repeated [--trend] for k sets"""
    return (["event"] + [f"mean{i}" for i in range(1, k + 1)] + [f"median{i}" for i in range(1, k + 1)] + ["delta"] +
            (["z"] if trend else ["Q", "W"]) + ["p-value", "corrected"] + (["gene", "overlapping", "transcript_id"] if gtf else []))


def command_table(ref, names, trend, corrected):
    """a table_reference, the event names of all rows and the corrected p of the tested rows -> (the tested rows, one list
    of cells per tested row: str() of the numpy scalars, as the command prints them)"""
    keep = np.flatnonzero(ref["tested"])
    stats = ("z",) if trend else ("q", "w")
    p = ref["p_page" if trend else "p_friedman"]
    return keep, [[names[r]] + [str(x) for x in ref["mean"][:, r]] + [str(x) for x in ref["med"][:, r]] + [str(ref["delta"][r])] +
                  [str(ref[f][r]) for f in stats] + [str(p[r]), str(np.float64(corrected[i]))] for i, r in enumerate(keep)]


def row_reference(row, sets):
    """table_reference of one row -> dict of scalars (med, mean: [k])"""
    ref = table_reference(np.asarray(row, np.float32)[None, :], sets)
    return {name: v[..., 0] for name, v in ref.items()}
