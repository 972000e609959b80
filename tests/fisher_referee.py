"""Referee of the pair kernels on counts of any size (helper module, no tests in here): the two-sided Fisher p of one 2x2
table and the Yates-corrected chi-square p in mpmath at 60 digits.

scipy.stats.fisher_exact takes minutes on margins of 1e7 and its Boost pmf is a difference of log-gammas like the one the
kernel used to have; tools/exact_fisher.py is exact but O(margin^2) bits.  Here pmf(a) comes from mpmath.loggamma (60
digits: the nine terms of ~1e17 cancel to ~1e2 and leave ~40 digits) and the ratios r_k = pmf(k) / pmf(a) from the exact
one-step recurrence outward from k = a, so a walk costs O(sigma) multiplications whatever the counts are.

    two_sided(a, b, c, d)  -> (p, nearest)      p: the sum of pmf(k) over the support with pmf(k) <= pmf(a) (scipy's rule),
                                                any zero margin -> 1, clipped at 1;  nearest: the smallest |r_k - 1| over
                                                the terms with r_k != 1 (inf when there is none)
    chi2_yates(a, b, c, d) -> (p, bad)          the formula in the header of csrc/chi2.hip; bad: an expected frequency
                                                is zero (p = NaN then)

`nearest` is what makes a table a fair fixture: scipy accepts pmf(k) <= pmf(a) (1 + 1e-14), the kernel (1 + 1e-12), the
referee ties only; with nearest >= 1e-9 all three select the same terms.  A mathematical tie (r_k == 1) is accepted; it
shows as |r_k - 1| < 1e-40 after at most a few million roundings of 1e-60, and no ratio of integers below 2^64 that walks
can reach is that close to 1 without being 1.
"""
import math

import mpmath as mp

DPS = 60
TIE = mp.mpf(10) ** -40
DONE = mp.mpf(10) ** -30      # a side stops once its ratio is falling and the term is below this fraction of the sum

_CACHE = {}


def _side(u1, u2, v1, v2, steps):
    """sum of the accepted r_k walking away from a: the step ratio is (u1 u2) / (v1 v2), u falling and v rising by one per
    step (csrc/fisher.hip, Walk) -> (sum, nearest, terms walked)"""
    r, acc, nearest, k = mp.mpf(1), mp.mpf(0), mp.inf, 0
    while k < steps:
        num, den = (u1 - k) * (u2 - k), (v1 + k) * (v2 + k)
        r = r * num / den
        k += 1
        off = abs(r - 1)
        if off < TIE:
            acc += 1
        else:
            nearest = min(nearest, off)
            if r < 1:
                acc += r
        if num < den and r < DONE * (1 + acc):
            break
    return acc, nearest, k


def two_sided(a, b, c, d):
    """(p, nearest) as floats; see the module text"""
    key = (int(a), int(b), int(c), int(d))
    if key not in _CACHE:
        a, b, c, d = key
        assert min(key) >= 0
        n1, n2, n, m = a + b, c + d, a + c, b + d
        if n1 == 0 or n2 == 0 or n == 0 or m == 0:
            _CACHE[key] = (1.0, math.inf)
        else:
            with mp.workdps(DPS):
                lf = lambda k: mp.loggamma(k + 1)                                              # noqa: E731
                logp = lf(n1) + lf(n2) + lf(n) + lf(m) - lf(n1 + n2) - lf(a) - lf(b) - lf(c) - lf(d)
                down, near_d, _ = _side(a, d, b + 1, c + 1, min(a, d))
                up, near_u, _ = _side(b, c, a + 1, d + 1, min(b, c))
                p = mp.exp(logp) * (1 + down + up)
                _CACHE[key] = (float(min(p, mp.mpf(1))), float(min(near_d, near_u)))
    return _CACHE[key]


def ratio_sum(a, b, c, d):
    """1 + the sum of the accepted ratios (what the kernel's walk computes), as an mpf; a zero margin has no step"""
    with mp.workdps(DPS):
        return 1 + _side(a, d, b + 1, c + 1, min(a, d))[0] + _side(b, c, a + 1, d + 1, min(b, c))[0]


def log_pmf(a, b, c, d):
    """log pmf(a) as an mpf (margins non-zero)"""
    with mp.workdps(DPS):
        lf = lambda k: mp.loggamma(k + 1)                                                      # noqa: E731
        return lf(a + b) + lf(c + d) + lf(a + c) + lf(b + d) - lf(a + b + c + d) - lf(a) - lf(b) - lf(c) - lf(d)


def chi2_yates(a, b, c, d):
    """(p, bad): expected = row * col / total, observed moved towards expected by min(0.5, |expected - observed|),
    chi2 = sum (observed - expected)^2 / expected, p = erfc(sqrt(chi2 / 2)) -- all in mpf"""
    a, b, c, d = int(a), int(b), int(c), int(d)
    r0, r1, c0, c1 = a + b, c + d, a + c, b + d
    tot = r0 + r1
    if tot == 0 or r0 * c0 == 0 or r0 * c1 == 0 or r1 * c0 == 0 or r1 * c1 == 0:
        return math.nan, True
    with mp.workdps(DPS):
        stat = mp.mpf(0)
        for o, rc in ((a, r0 * c0), (b, r0 * c1), (c, r1 * c0), (d, r1 * c1)):
            e = mp.mpf(rc) / tot
            diff = e - o
            t = o + mp.sign(diff) * min(mp.mpf(0.5), abs(diff)) - e
            stat += t * t / e
        return float(mp.erfc(mp.sqrt(stat / 2))), False
