"""The tables of the shift suites (tests/test_shift_cpu.py, test_gpu_shift.py, test_gpu_shift_sweeps.py) and their
references from tests/shift_referee.py, built once and cached (helper module, no tests in here).

A table is of one FLAVOUR: "grid" (every row holds 3-decimal values only: the kernels' integer path, and in the lane-group
kernel the pass where no row is off the grid), "off" (every row holds a value off the grid) or "mixed" (the rows of the
two interleaved, so that the rows side by side in a wave differ).  CASES lists every table any GPU test runs with its
confidence level; tests/test_shift_cpu.py checks the fixture condition on all of them."""
import functools

import numpy as np

import shift_referee as SR

# every total in 6..66: both kernels, every lane-group width (8, 16, 32, 64 lanes), the switch at 64 | 65; and the
# workgroup kernel's first LDS sizes (128 | 256 keys)
TOTALS = tuple(range(6, 67)) + (127, 128, 129)
FLAVOURS = ("grid", "off", "mixed")
# kind -> the flavours of row it has
KINDS = {
    "no NaN": ("grid", "off"),
    "6 % NaN": ("grid", "off"),
    "NaNs leaving 3 v 3": ("grid", "off"),
    "NaNs leaving 2 v 3": ("grid", "off"),
    "all values equal": ("grid", "off"),
    "fully separated": ("grid", "off"),
    "heavy ties": ("grid", "off"),
    "signed zeros": ("grid", "off"),
    "keys 0 and 1000": ("grid",),
    "subnormals": ("off",),
    "+-FLT_MAX": ("off",),
    "outside [0, 1]": ("off",),
    "a kept infinity": ("off",),
    "one value off the grid": ("off",),
}
LARGE_KINDS = ("no NaN", "6 % NaN", "NaNs leaving 3 v 3", "heavy ties", "keys 0 and 1000", "+-FLT_MAX")
LEVELS = (0.5, 0.9, 0.95, 0.99)
LEVEL_TOTALS = (7, 16, 40, 65, 129)
LARGE = ((4096, 4096), (4096, 3), (3, 4096))
SLICE_TOTALS = (9, 40, 66)
# lists of unlike lengths: the longest group a lane-group row can have, beside the shortest, on both sides; the same one
# column further, in the workgroup kernel
LOPSIDED = ((3, 61), (61, 3), (3, 13), (13, 3), (3, 62), (62, 3))


def split(total):
    """-> (n1, n2), n1 + n2 = total, both >= 3: halves, a third where total = 1 mod 3"""
    n1 = total // 3 if (total % 3 == 1 and total >= 10) else total // 2
    return n1, total - n1


def draw_lists(rng, n1, n2, spare=3):
    """two disjoint column lists of a shuffled table of n1 + n2 + spare columns"""
    s = n1 + n2 + spare
    perm = rng.permutation(s).astype(np.int32)
    return perm[:n1].copy(), perm[n1: n1 + n2].copy(), s


def _grid(v):
    return (np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32)          # float32(k / 1000.0)


def make_row(rng, name, grid, g1, g2, s):
    """one row of kind `name` on the grid or off it"""
    n1, n2 = g1.size, g2.size
    nan = np.float32(np.nan)
    shift = rng.uniform(-0.2, 0.2)
    x, y = 0.25 + 0.5 * rng.random(n1) + shift, 0.25 + 0.5 * rng.random(n2)
    if grid:
        x, y = _grid(x), _grid(y)
    else:
        x, y = ((v * 1.7 - 0.3).astype(np.float32) for v in (x, y))
        dup = rng.integers(0, min(n1, n2), size=(max(1, min(n1, n2) // 4), 2))           # equal values across the sides
        x[dup[:, 0]] = y[dup[:, 1]]
    if name == "6 % NaN":
        x[rng.random(n1) < 0.06] = nan
        y[rng.random(n2) < 0.06] = nan
    elif name in ("NaNs leaving 3 v 3", "NaNs leaving 2 v 3"):
        x[rng.permutation(n1)[(3 if name[13] == "3" else 2):]] = nan
        y[rng.permutation(n2)[3:]] = nan
    elif name == "all values equal":
        x[:], y[:] = (np.float32(0.5), np.float32(0.5)) if grid else (np.float32(0.1234567), np.float32(0.1234567))
    elif name == "fully separated":
        lo, hi = (x, y) if rng.random() < 0.5 else (y, x)
        if grid:
            lo[:], hi[:] = _grid(0.4 * rng.random(lo.size)), _grid(0.6 + 0.4 * rng.random(hi.size))
        else:
            lo[:], hi[:] = -np.abs(lo) - np.float32(0.5), np.abs(hi) + np.float32(0.5)
    elif name == "heavy ties":
        levels = ((rng.permutation(1001)[:6] / 1000.0).astype(np.float32) if grid
                  else rng.random(6, dtype=np.float32) * np.float32(3) - np.float32(1))
        x, y = levels[rng.integers(0, 6, size=n1)], levels[rng.integers(0, 6, size=n2)]
    elif name == "signed zeros":
        # zeros of either sign on both sides: every difference of two of them is one value, and the result is +0.0
        zeros = np.array([-0.0, 0.0], np.float32)
        sx, sy = rng.random(n1) < 0.7, rng.random(n2) < 0.7
        sx[:2], sy[:2] = True, True
        sx[-1], sy[-1] = False, False                       # (a value of the row's own flavour stays on each side)
        x[sx], y[sy] = rng.choice(zeros, size=int(sx.sum())), rng.choice(zeros, size=int(sy.sum()))
        x[0], y[0], x[1], y[1] = zeros[0], zeros[1], zeros[1], zeros[0]
    elif name == "keys 0 and 1000":
        # the two ends of the grid on both sides: differences of +-1000 thousandths
        x, y = (np.array([0.0, 1.0], np.float32)[rng.integers(0, 2, size=k)] for k in (n1, n2))
        x[0], x[1], y[0], y[1] = 0.0, 1.0, 1.0, 0.0
    elif name == "subnormals":
        x, y = (rng.integers(1, 41, size=k).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], np.float32), size=k)
                for k in (n1, n2))
    elif name == "+-FLT_MAX":
        # the largest float of both signs on both sides: a difference of 2 FLT_MAX is finite in float64
        top = np.float32(np.finfo(np.float32).max)
        x[0], x[1], y[0], y[1] = top, -top, -top, top
    elif name == "outside [0, 1]":
        x, y = (x * np.float32(40) - np.float32(7.5)), (y * np.float32(40) - np.float32(7.5))
        x[0], y[0] = np.float32(1.001), np.float32(-0.001)        # 3-decimal values that have no key
    elif name == "a kept infinity":
        inf = np.float32(np.inf)
        (x if rng.random() < 0.5 else y)[rng.integers(0, 3)] = inf if rng.random() < 0.5 else -inf
    elif name == "one value off the grid":
        x, y = _grid(x), _grid(y)
        y[rng.integers(0, n2)] = np.float32(0.12345)
    row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)       # would show if a spare column were read
    row[g1], row[g2] = x, y
    return row


@functools.lru_cache(maxsize=None)
def table(n1, n2, flavour="mixed", per_kind=1, kinds=None):
    """-> (ps float32[rows, n1 + n2 + 3], g1, g2, (kind, grid)[rows]); read-only"""
    rng = np.random.default_rng(20000 + 131 * n1 + 17 * n2 + FLAVOURS.index(flavour))
    g1, g2, s = draw_lists(rng, n1, n2)
    rows, what = [], []
    for _ in range(per_kind):
        for name in (KINDS if kinds is None else kinds):
            for fl in KINDS[name]:
                if flavour in (fl, "mixed"):
                    rows.append(make_row(rng, name, fl == "grid", g1, g2, s))
                    what.append((name, fl == "grid"))
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, g1, g2, what


@functools.lru_cache(maxsize=None)
def reference(n1, n2, flavour="mixed", per_kind=1, kinds=None, conf=0.95):
    ps, g1, g2, _ = table(n1, n2, flavour, per_kind, kinds)
    return SR.table_reference(ps, g1, g2, SR.zq_of(conf))


def cases():
    """every (table arguments, conf) a GPU test runs: what the fixture condition is checked on"""
    out = [((*split(t), fl), 0.95) for t in TOTALS for fl in FLAVOURS]
    out += [((*split(t), "mixed"), conf) for t in LEVEL_TOTALS for conf in LEVELS]
    out += [((n1, n2, "mixed", 1, LARGE_KINDS), 0.95) for n1, n2 in LARGE]
    out += [((*split(t), "mixed", 4), 0.95) for t in SLICE_TOTALS]
    out += [((n1, n2, "mixed"), 0.95) for n1, n2 in LOPSIDED]
    out += [((3, 3, "mixed", 4), 0.95), ((32, 33, "mixed", 4), 0.95)]                # the palettes of the grid-stride tables
    return out
