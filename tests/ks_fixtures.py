"""The tables of the Kolmogorov-Smirnov suites (tests/test_ks_cpu.py, test_gpu_ks.py, test_gpu_ks_sweeps.py) and their
references from tests/ks_referee.py, built once and cached (helper module, no tests in here).

A mixed table holds every row kind of KINDS twice -- on 3-decimal values and on off-grid float32 values -- interleaved,
so that the rows side by side in a wave are of different kinds.  Outside the ladders the shift between the groups is
scaled with sqrt((n1 + n2) / (n1 n2)), which keeps the referee's p far above the floor of 1e-280 at any size (D stays
under 0.39 at 4096 v 4096: 2 exp(-4096 D^2) >= 1e-280 needs D <= 0.397); test_ks_cpu.py asserts it."""
import functools

import numpy as np

import ks_referee as KR

# every total in 6..66: both kernels, every lane-group width (8, 16, 32, 64 lanes), the switch at 64 | 65; and the
# workgroup kernel's first LDS sizes
TOTALS = tuple(range(6, 67)) + (127, 128, 129)
KINDS = ("no NaN", "6 % NaN", "NaNs leaving 3 v 3", "NaNs leaving 2 v 3", "all values equal", "identical samples",
         "fully separated", "tie run of both groups at the extreme", "heavy ties", "signed zeros", "subnormals and FLT_MAX",
         "+-inf")
LARGE_KINDS = (0, 1, 2, 8, 9)       # of the 4096-column tables: no kind that takes p under the floor there
F32 = ("med1", "med2", "mean1", "mean2", "delta")
OUTS = ("tested", "p", "d") + F32 + ("exact",)
BLOCK = 4096


def split(total):
    """-> (n1, n2), n1 + n2 = total, both >= 3: halves (equal or consecutive, so coprime), a third where total = 1 mod 3"""
    n1 = total // 3 if (total % 3 == 1 and total >= 10) else total // 2
    return n1, total - n1


def draw_lists(rng, n1, n2, spare=3):
    """two disjoint column lists of a shuffled table of n1 + n2 + spare columns"""
    s = n1 + n2 + spare
    perm = rng.permutation(s).astype(np.int32)
    return perm[:n1].copy(), perm[n1: n1 + n2].copy(), s


def _grid(v):
    return (np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32)          # float32(k / 1000.0)


def _base(rng, n1, n2, grid):
    """the two sides of a row before its kind is applied: uniform values of width 0.6, side 1 shifted by a draw that
    moves D by about 2.4 sqrt((n1 + n2) / (n1 n2)) at most (by 0.2 at most, so that small groups stay inside [0, 1])"""
    shift = rng.uniform(-5.0, 5.0) * min(0.29 * np.sqrt((n1 + n2) / (n1 * n2)), 0.04)
    x, y = 0.2 + 0.6 * rng.random(n1) + shift, 0.2 + 0.6 * rng.random(n2)
    if grid:
        return [_grid(x), _grid(y)]
    x, y = ((v * 1.7 - 0.3).astype(np.float32) + rng.random(v.size, dtype=np.float32) * np.float32(1e-3) for v in (x, y))
    dup = rng.integers(0, min(n1, n2), size=(max(1, min(n1, n2) // 4), 2))       # exact duplicates across the sides ...
    x[dup[:, 0]] = y[dup[:, 1]]
    dup = rng.integers(0, n2, size=(max(1, n2 // 6), 2))                         # ... and inside one
    y[dup[:, 0]] = y[dup[:, 1]]
    return [x, y]


def make_row(rng, kind, v, g1, g2, s):
    """one row of KINDS[kind], variant v (even: 3-decimal values, odd: off-grid float32)"""
    name = KINDS[kind]
    n1, n2 = g1.size, g2.size
    grid = v % 2 == 0
    x, y = _base(rng, n1, n2, grid)
    nan = np.float32(np.nan)
    if name == "6 % NaN":
        x[rng.random(n1) < 0.06] = nan
        y[rng.random(n2) < 0.06] = nan
    elif name in ("NaNs leaving 3 v 3", "NaNs leaving 2 v 3"):
        x[rng.permutation(n1)[(3 if name[13] == "3" else 2):]] = nan
        y[rng.permutation(n2)[3:]] = nan
    elif name == "all values equal":
        x[:], y[:] = (np.float32(0.5), np.float32(0.5)) if grid else (np.float32(0.1234567), np.float32(0.1234567))
    elif name == "identical samples":
        k = min(n1, n2)                              # the longer side keeps as many values as the shorter has
        keep1, keep2 = rng.permutation(n1)[:k], rng.permutation(n2)[:k]
        vals = x[keep1].copy()
        x[:], y[:] = nan, nan
        x[keep1], y[keep2] = vals, rng.permutation(vals)
    elif name == "fully separated":
        lo, hi = (x, y) if v % 4 < 2 else (y, x)
        if grid:
            lo[:], hi[:] = _grid(0.4 * rng.random(lo.size)), _grid(0.6 + 0.4 * rng.random(hi.size))
        else:
            lo[:], hi[:] = -np.abs(lo) - np.float32(0.5), np.abs(hi) + np.float32(0.5)
    elif name == "tie run of both groups at the extreme":
        # side 1 sits on one value t (but for one value below it from 4 columns up), a quarter of side 2 shares t and
        # the rest lies above: the largest deviation, n1 (n2 - ties of side 2), is at the END of the run of t, and an
        # evaluation inside the run (side 1's part first) would report n1 n2
        t = np.float32(0.3) if grid else np.float32(-0.777)
        x[:] = t
        y[:] = _grid(0.5 + 0.4 * rng.random(n2)) if grid else (0.5 + rng.random(n2)).astype(np.float32)
        if n1 >= 4:
            x[rng.integers(0, n1)] = np.float32(0.1) if grid else np.float32(-1.5)
        y[rng.permutation(n2)[: max(1, n2 // 4)]] = t
    elif name == "heavy ties":
        levels = (rng.permutation(1001)[:8] / 1000.0).astype(np.float32) if grid else rng.random(8, dtype=np.float32) * np.float32(3) - np.float32(1)
        x, y = levels[rng.integers(0, 8, size=n1)], levels[rng.integers(0, 8, size=n2)]
    elif name == "signed zeros":
        zeros = np.array([-0.0, 0.0], np.float32)
        sx, sy = rng.random(n1) < 0.4, rng.random(n2) < 0.4
        sx[0], sy[0] = True, True
        x[sx], y[sy] = rng.choice(zeros, size=int(sx.sum())), rng.choice(zeros, size=int(sy.sum()))
        x[0], y[0] = zeros[v % 2], zeros[1 - v % 2]          # a zero of either sign on the two sides: one value
    elif name == "subnormals and FLT_MAX":
        # multiples of 2^-149 of either sign, and the largest float of one sign (two of them overflow a float32 sum)
        x, y = (rng.integers(1, 41, size=k).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], np.float32), size=k)
                for k in (n1, n2))
        top = np.float32(np.finfo(np.float32).max)
        x[rng.permutation(n1)[: 1 + v % 2]] = top
        y[rng.permutation(n2)[:1]] = top
    elif name == "+-inf":
        # one sign of infinity per side (both signs on a side would make its mean a NaN of no defined sign); variant
        # 1 and 3: +inf on both sides, a tie run of both groups at the top of the order
        inf = np.float32(np.inf)
        x[rng.permutation(n1)[:1]] = inf if v % 2 else -inf
        y[rng.permutation(n2)[:1]] = inf
    row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)       # would show if a spare column were read
    row[g1], row[g2] = x, y
    return row


@functools.lru_cache(maxsize=None)
def table(n1, n2, per_kind=2, kinds=None):
    """-> (ps float32[rows, n1 + n2 + 3], g1, g2, kind[rows]); the kinds interleaved"""
    rng = np.random.default_rng(19000 + 131 * n1 + 17 * n2)
    g1, g2, s = draw_lists(rng, n1, n2)
    rows, names = [], []
    for v in range(per_kind):
        for k in (range(len(KINDS)) if kinds is None else kinds):
            rows.append(make_row(rng, k, v, g1, g2, s))
            names.append(k)
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, g1, g2, np.array(names)


@functools.lru_cache(maxsize=None)
def reference(n1, n2, per_kind=2, kinds=None, want_exact=True):
    ps, g1, g2, _ = table(n1, n2, per_kind, kinds)
    return KR.table_reference(ps, g1, g2, want_exact)


# ---------------------------------------------------------------- the exact sweep: every kept pair
def kept_pairs():
    """every (n1', n2') with 3 <= n1', n2' and N <= 32, and the pairs of N = 33 (not eligible)"""
    return [(a, N - a) for N in range(6, 34) for a in range(3, N - 2)]


@functools.lru_cache(maxsize=None)
def pair_table(n1, n2):
    """columns n1 v n2 with NaNs leaving every pair of kept_pairs() that fits, each tied (3-decimal values of 12 levels) and
    untied (distinct off-grid values) -> (ps, g1, g2, pairs[rows]).  30 v 30 holds every pair and goes through the
    lane-group kernel (60 columns), 40 v 40 through the workgroup kernel"""
    rng = np.random.default_rng(500 + n1)
    g1, g2, s = draw_lists(rng, n1, n2)
    rows, pairs = [], []
    for a, b in kept_pairs():
        if a > n1 or b > n2:
            continue
        for tied in (True, False):
            if tied:
                x, y = (rng.integers(0, 12, size=k) / 10.0 for k in (n1, n2))
                x = np.clip(x + rng.integers(0, 3) / 10.0, 0, 1)
            else:
                perm = rng.permutation(4 * (n1 + n2)) / 7.0 - 3.0
                x, y = perm[:n1] + rng.uniform(-2, 2), perm[n1: n1 + n2]
            x, y = x.astype(np.float32), y.astype(np.float32)
            x[rng.permutation(n1)[a:]] = np.nan
            y[rng.permutation(n2)[b:]] = np.nan
            row = np.full(s, np.nan, np.float32)
            row[g1], row[g2] = x, y
            rows.append(row)
            pairs.append((a, b))
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, g1, g2, np.array(pairs)


@functools.lru_cache(maxsize=None)
def pair_reference(n1, n2):
    ps, g1, g2, _ = pair_table(n1, n2)
    return KR.table_reference(ps, g1, g2, True)


# ---------------------------------------------------------------- the grid-stride blocks
@functools.lru_cache(maxsize=None)
def block(n1, n2):
    """BLOCK distinct rows, the kinds cycling -> (ps, g1, g2)"""
    rng = np.random.default_rng(990 + n1)
    g1, g2, s = draw_lists(rng, n1, n2)
    ps = np.stack([make_row(rng, r % len(KINDS), r // len(KINDS), g1, g2, s) for r in range(BLOCK)])
    ps.setflags(write=False)
    return ps, g1, g2


@functools.lru_cache(maxsize=None)
def block_reference(n1, n2):
    ps, g1, g2 = block(n1, n2)
    return KR.table_reference(ps, g1, g2, True)


# ---------------------------------------------------------------- the p ladders
LADDERS = [(1024, 1024, 40), (4096, 4096, 48)]


@functools.lru_cache(maxsize=None)
def ladder(n1, n2, steps):
    """rows whose D runs from 0 to 1: in row t the first round(t / (steps - 1) n2) columns of group 2 lie above every
    value of group 1 and the rest are group 1's own values again (n1 == n2), so D = that share.  Even rows hold
    3-decimal values (heavy ties), odd rows distinct off-grid values."""
    assert n1 == n2
    rng = np.random.default_rng(n1 + 5)
    s = n1 + n2
    g1, g2 = np.arange(0, s, 2, dtype=np.int32)[:n1], np.arange(1, s, 2, dtype=np.int32)[:n2]
    ps = np.zeros((steps, s), np.float32)
    for t in range(steps):
        up = int(round(t / (steps - 1.0) * n2))
        if t % 2 == 0:
            x = rng.integers(0, 501, size=n1) / 1000.0
            top = rng.integers(600, 1001, size=up) / 1000.0
        else:
            x = rng.permutation(9973)[:n1] / 9973.0 - 2.0
            top = 2.0 + rng.permutation(n2)[:up] / 7919.0
        order = rng.permutation(n1)
        y = np.concatenate([top, np.sort(x)[: n2 - up]])       # the n2 - up smallest of x again: the ECDFs part at the top only
        ps[t, g1], ps[t, g2] = x.astype(np.float32)[order], y.astype(np.float32)[rng.permutation(n2)]
    ps.setflags(write=False)
    return ps, g1, g2


@functools.lru_cache(maxsize=None)
def ladder_reference(n1, n2, steps):
    ps, g1, g2 = ladder(n1, n2, steps)
    return KR.table_reference(ps, g1, g2, True)
