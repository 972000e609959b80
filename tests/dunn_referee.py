"""Exact referee for Dunn's test after Kruskal-Wallis (helper module, no tests in here).

Everything K12 defines -- the row rules, the keys, H, the float32 fields -- is kruskal_referee's.  On the same integer keys
(1000 * value for 3-decimal PS values, a dense rank for arbitrary float32 values) this module adds, per pair of sets i < j
in the order (0,1), (0,2), .., (k-2,k-1):

   r2  = 2 * mid-rank over all N kept values (int)        D_i = sum_{set i} r2 - n_i (N + 1)   (int)
   den = N^3 - N - sum(t^3 - t)                           num = D_i n_j - D_j n_i              (int)
   z^2 = 3 (N - 1) num^2 / (n_i n_j (n_i + n_j) den)      (fractions.Fraction: no rounding)
   z   = sign(num) sqrt(z^2), CORRECTLY ROUNDED to float64: the candidate float(mpmath sqrt at 60 digits) is kept only when
         z^2 lies strictly between the squares of the midpoints to its two float64 neighbours, compared as Fractions
   p   = erfc(|z| / sqrt 2) from mpmath at 50 digits on the exact z
   padj: Holm's step-down in mpmath: the p's in ascending order, padj_(r) = min(1, max_{t <= r} (m - t + 1) p_(t))

A row whose kept values are all equal (den == 0): z = 0, p = 1, padj = 1 in every pair.  A row that is not tested: 0.
"""
import math
from fractions import Fraction

import numpy as np

import kruskal_referee as KR

DPS = 50


def pairs(k):
    """the pairs (i, j), i < j, in output order"""
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def exact_pieces(key_sets):
    """key_sets: one integer array per set -> dict(N, n (list), D (list), den) of Python ints"""
    key_sets = [np.asarray(g, dtype=np.int64) for g in key_sets]
    allk = np.concatenate(key_sets)
    N = int(allk.size)
    _, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
    before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    r2 = 2 * before + cnt + 1
    D, n, at = [], [], 0
    for g in key_sets:
        m = int(g.size)
        D.append(int(r2[inv[at: at + m]].sum()) - m * (N + 1))
        n.append(m)
        at += m
    return dict(N=N, n=n, D=D, den=N ** 3 - N - sum(int(t) ** 3 - int(t) for t in cnt))


def pair_num(pc, i, j):
    return pc["D"][i] * pc["n"][j] - pc["D"][j] * pc["n"][i]


def z_squared(pc, i, j):
    """z_ij^2 as a Fraction (den > 0)"""
    ni, nj = pc["n"][i], pc["n"][j]
    return Fraction(3 * (pc["N"] - 1) * pair_num(pc, i, j) ** 2, ni * nj * (ni + nj) * pc["den"])


def rounded_sqrt(q):
    """the float64 nearest to sqrt(q) for a Fraction q >= 0, proved: q lies strictly between the squares of the midpoints
    to the candidate's neighbours (exact comparisons)"""
    import mpmath
    if q == 0:
        return 0.0
    with mpmath.workdps(60):
        f = float(mpmath.sqrt(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator)))
    lo = (Fraction(f) + Fraction(math.nextafter(f, 0.0))) / 2
    hi = (Fraction(f) + Fraction(math.nextafter(f, math.inf))) / 2
    assert lo * lo < q < hi * hi, ("not the nearest float64, or a tie", f, q)
    return f


def holm(ps):
    """Holm's step-down over a list of numbers (mpmath or float) -> the adjusted values in the order given.  Ties in the
    sort are broken by index; equal p's get equal results whatever the order (the earlier rank has the larger factor)."""
    m = len(ps)
    order = sorted(range(m), key=lambda q: (ps[q], q))
    out = [None] * m
    best = 0
    for r, q in enumerate(order):
        v = (m - r) * ps[q]
        best = v if r == 0 or v > best else best
        out[q] = best if best < 1 else type(best)(1)
    return out


def row_pairs(pc):
    """-> (z floats, p mpmath, padj mpmath, z2 Fractions, num ints) per pair, from exact_pieces' result"""
    import mpmath
    k = len(pc["n"])
    pr = pairs(k)
    nums = [pair_num(pc, i, j) for i, j in pr]
    if pc["den"] == 0:
        one = mpmath.mpf(1)
        return [0.0] * len(pr), [one] * len(pr), [one] * len(pr), [Fraction(0)] * len(pr), nums
    z2 = [z_squared(pc, i, j) for i, j in pr]
    z = [math.copysign(rounded_sqrt(q), num) if num else 0.0 for q, num in zip(z2, nums)]
    with mpmath.workdps(DPS):
        p = [mpmath.erfc(mpmath.sqrt(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator) / 2)) for q in z2]
        padj = holm(p)
    return z, p, padj, z2, nums


def row_reference(row, sets, grid):
    """One table row (float32) and the sets' column lists -> kruskal_referee.row_reference's dict plus pair_z (float64 [m]),
    pair_p, pair_padj (lists of mpmath numbers, or of 0.0 on an untested row), z2 (Fractions), num (ints), pieces"""
    base = KR.row_reference(row, sets, grid)
    m = len(sets) * (len(sets) - 1) // 2
    if not base["tested"]:
        return dict(base, pair_z=np.zeros(m), pair_p=[0.0] * m, pair_padj=[0.0] * m, z2=[Fraction(0)] * m, num=[0] * m, pieces=None)
    kept = [row[np.asarray(g)] for g in sets]
    kept = [v[~np.isnan(v)] for v in kept]
    if grid:
        key_sets = [KR.grid_keys(v) for v in kept]
    else:
        key_sets = np.split(KR.dense_keys(np.concatenate(kept)), np.cumsum([v.size for v in kept])[:-1])
    pc = exact_pieces(key_sets)
    z, p, padj, z2, nums = row_pairs(pc)
    return dict(base, pair_z=np.array(z), pair_p=p, pair_padj=padj, z2=z2, num=nums, pieces=pc)


def table_reference(rows, sets, grid=False):
    """row_reference for every row -> kruskal_referee.table_reference's dict of arrays plus pair_z, pair_p, pair_padj
    float64 [m, n] (an mpmath value below the float64 range becomes 0.0), zero_num bool [m, n] (tested and num == 0) and
    `exact`: per row the (pair_p, z2) lists of the tested rows, None elsewhere, for the tests that need more than float64"""
    n, k = rows.shape[0], len(sets)
    m = k * (k - 1) // 2
    out = KR.table_reference(rows, sets, grid)
    out.update(pair_z=np.zeros((m, n)), pair_p=np.zeros((m, n)), pair_padj=np.zeros((m, n)), zero_num=np.zeros((m, n), bool),
               exact=[None] * n)
    for r in range(n):
        if not out["tested"][r]:
            continue
        ref = row_reference(rows[r], sets, grid)
        out["pair_z"][:, r] = ref["pair_z"]
        out["pair_p"][:, r] = [float(x) for x in ref["pair_p"]]
        out["pair_padj"][:, r] = [float(x) for x in ref["pair_padj"]]
        out["zero_num"][:, r] = [x == 0 for x in ref["num"]]
        out["exact"][r] = (ref["pair_p"], ref["z2"])
    return out


def close_pairs(ref, rel=1e-6):
    """the condition on a GPU fixture: -> [(row, q, t)] of pair p-values of one row closer than `rel` relative without
    being equal as Fractions (equal z^2), so that no Holm order hangs on a rounding; empty for a usable fixture"""
    bad = []
    for r, ex in enumerate(ref["exact"]):
        if ex is None:
            continue
        p, z2 = ex
        for q in range(len(p)):
            for t in range(q + 1, len(p)):
                if z2[q] != z2[t] and abs(p[q] - p[t]) <= rel * max(p[q], p[t]):
                    bad.append((r, q, t))
    return bad


def command_header(k, gtf=False):
    """the header cells of `compare_sample_sets -mx --posthoc` over k sets"""
    cells = ["event"] + [f"mean{i + 1}" for i in range(k)] + [f"median{i + 1}" for i in range(k)] + ["delta", "H"]
    for i, j in pairs(k):
        cells += [f"z{i + 1}v{j + 1}", f"padj{i + 1}v{j + 1}"]
    return cells + ["p-value", "corrected"] + (["gene", "overlapping", "transcript_id"] if gtf else [])


def pair_cells(k):
    """-> (the positions of the z cells, the positions of the padj cells) in a line of the command's table"""
    first = 2 + 2 * k + 1
    m = k * (k - 1) // 2
    return [first + 2 * q for q in range(m)], [first + 2 * q + 1 for q in range(m)]


def command_table(ref, names, k, bh):
    """the expected table of the command from table_reference's result: the header and one list of cells per tested row,
    in row order.  The float32 cells and the z cells are str() of the referee's values (the engine's z is the correctly
    rounded one, so these are compared as text); H, padj, p-value and corrected are float64 values the engine's last bits
    may miss, so their cells are the referee's numbers, for the caller to hold the parsed cell to the parity bar.  bh: the
    Benjamini-Hochberg values of ref["p"] over the tested rows."""
    keep = np.flatnonzero(ref["tested"])
    lines = []
    for at, r in enumerate(keep):
        cells = [names[r]] + [str(x) for x in ref["mean"][:, r]] + [str(x) for x in ref["med"][:, r]] + [str(ref["delta"][r])]
        cells.append(float(ref["hf"][r]))
        for q in range(k * (k - 1) // 2):
            cells += [str(np.float64(ref["pair_z"][q, r])), float(ref["pair_padj"][q, r])]
        lines.append(cells + [float(ref["p"][r]), float(bh[at])])
    return command_header(k), keep, lines
