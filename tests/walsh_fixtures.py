"""The tables of the paired-shift suites (tests/test_walsh_cpu.py, test_gpu_walsh.py, test_gpu_walsh_sweeps.py,
test_gpu_walsh_call_order.py) and their references from tests/walsh_referee.py, built once and cached (helper module, no
tests in here).

A table is of one FLAVOUR: "grid" (every row holds 3-decimal values only: the kernels' integer paths, and in the lane-group
kernel the pass where no row is off the grid), "off" (every row holds a value off the grid) or "mixed" (the rows of the two
interleaved, so that the rows side by side in a wave differ).  cases() lists every table any GPU test runs with its
confidence level; tests/test_walsh_cpu.py checks the fixture condition on all of them, and that LEVELS are levels at which
no rank of any pair count hangs on a rounding."""
import functools

import numpy as np

import rank_support as RS
import walsh_referee as WR

# every pair count 3..66: both kernels, every lane-group width (8, 16, 32, 64 lanes), the switch at 64 | 65; the workgroup
# kernel's first sort lengths (128 | 256 | 512 keys)
PAIRS = tuple(range(3, 67)) + (127, 128, 129, 255, 256, 257)
FLAVOURS = ("grid", "off", "mixed")
BOTH = ("grid", "off")
# kind -> the flavours of row it has
KINDS = {
    "no NaN": BOTH,
    "6 % NaN": BOTH,
    "NaNs leaving 3 pairs": BOTH,
    "NaNs leaving 2 pairs": BOTH,
    "NaNs leaving no pair": BOTH,
    "all differences zero": BOTH,
    "all differences equal": BOTH,
    "heavy ties": BOTH,
    "all positive": BOTH,
    "all negative": BOTH,
    "signed zeros": BOTH,
    "keys 0 and 1000": ("grid",),
    "subnormals": ("off",),
    "+-FLT_MAX": ("off",),
    "FLT_MAX overflow": ("off",),
    "outside [0, 1]": ("off",),
    "a kept infinity": ("off",),
    "one value off the grid": ("off",),
}
NAN_TRIPLES = ("FLT_MAX overflow", "a kept infinity")
LEVELS = (0.5, 0.8, 0.9, 0.95, 0.99)          # the only levels a GPU fixture uses (test_walsh_cpu.py: the survey)
LEVEL_PAIRS = (3, 7, 16, 40, 65, 129)
LARGE = 4096                                    # two rows only: the referee orders 8.4 M sums a row
LARGE_KINDS = ("6 % NaN",)
SLICE_PAIRS = (9, 40, 66)
GROUP_PALETTE, BLOCK_PALETTE = 3, 65            # the palettes of the grid-stride tables: the fewest pairs of each kernel


def _grid(v):
    return (np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32)          # float32(k / 1000.0)


def make_row(rng, name, grid, a, b, s):
    """one row of kind `name` on the grid or off it: x at the columns a, y at the columns b"""
    m = a.size
    nan, top = np.float32(np.nan), np.float32(np.finfo(np.float32).max)
    move = rng.uniform(-0.2, 0.2)
    y = 0.25 + 0.5 * rng.random(m)
    x = y + move + 0.1 * rng.standard_normal(m)
    if grid:
        x, y = _grid(x), _grid(y)
    else:
        x, y = ((v * 1.7 - 0.3).astype(np.float32) for v in (x, y))
    same = rng.random(m) < 0.2                              # pairs of equal values: zero differences, which the estimate keeps
    x[same] = y[same]
    if name == "6 % NaN":
        x[rng.random(m) < 0.06] = nan
        y[rng.random(m) < 0.06] = nan
    elif name.startswith("NaNs leaving"):
        left = {"3": 3, "2": 2, "n": 0}[name[13]]
        for q in rng.permutation(m)[left:]:                  # a NaN on one side of the pair, on the other, or on both
            side = rng.integers(0, 3)
            if side != 1:
                x[q] = nan
            if side != 0:
                y[q] = nan
    elif name == "all differences zero":
        x = y.copy()
    elif name == "all differences equal":
        if grid:
            y = _grid(0.1 + 0.5 * rng.random(m))
            x = _grid(y.astype(np.float64) + 0.137)         # 137 thousandths in every pair
        else:
            y = ((513 + rng.integers(0, 500, size=m)) / 1024.0).astype(np.float32)        # exact in float32, and so is the
            y[0] = np.float32(513 / 1024.0)                                                # difference; 513/1024 has no key
            x = y - np.float32(0.25)
    elif name == "heavy ties":
        levels = ((rng.permutation(1001)[:6] / 1000.0).astype(np.float32) if grid
                  else rng.random(6, dtype=np.float32) * np.float32(3) - np.float32(1))
        x, y = levels[rng.integers(0, 6, size=m)], levels[rng.integers(0, 6, size=m)]
    elif name in ("all positive", "all negative"):
        if grid:
            lo, hi = _grid(0.4 * rng.random(m)), _grid(0.6 + 0.4 * rng.random(m))
        else:
            lo, hi = -np.abs(y) - np.float32(0.5), np.abs(x) + np.float32(0.5)
        x, y = (hi, lo) if name == "all positive" else (lo, hi)
    elif name == "signed zeros":
        # zeros of either sign on both sides: a float32 difference of two of them is -0.0 or +0.0, one value, and the
        # result is +0.0
        zeros = np.array([-0.0, 0.0], np.float32)
        z = rng.random(m) < 0.7
        z[:2], z[-1] = True, False                          # (a pair of the row's own flavour stays)
        x[z], y[z] = rng.choice(zeros, size=int(z.sum())), rng.choice(zeros, size=int(z.sum()))
        x[0], y[0], x[1], y[1] = zeros[0], zeros[1], zeros[1], zeros[0]
        if not grid:
            x[-1] = np.float32(0.12345)
    elif name == "keys 0 and 1000":
        # the two ends of the grid on both sides: differences of +-1000 thousandths, sums of +-2000
        x, y = (np.array([0.0, 1.0], np.float32)[rng.integers(0, 2, size=m)] for _ in range(2))
        x[0], y[0], x[1], y[1] = 0.0, 1.0, 1.0, 0.0
    elif name == "subnormals":
        x, y = (rng.integers(1, 41, size=m).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], np.float32), size=m)
                for _ in range(2))
    elif name == "+-FLT_MAX":
        # differences of +-FLT_MAX: a sum of 2 FLT_MAX is finite in float64
        x[0], y[0], x[1], y[1] = top, np.float32(0.0), -top, np.float32(0.0)
    elif name == "FLT_MAX overflow":
        x[0], y[0] = top, -top                               # the float32 difference is +inf
    elif name == "outside [0, 1]":
        x, y = (x * np.float32(40) - np.float32(7.5)), (y * np.float32(40) - np.float32(7.5))
        x[0], y[0] = np.float32(1.001), np.float32(-0.001)        # 3-decimal values that have no key
    elif name == "a kept infinity":
        inf = np.float32(np.inf)
        (x if rng.random() < 0.5 else y)[rng.integers(0, 3)] = inf if rng.random() < 0.5 else -inf
    elif name == "one value off the grid":
        x, y = _grid(x), _grid(y)
        y[rng.integers(0, m)] = np.float32(0.12345)
    elif not grid and name == "no NaN":
        x[0] = np.float32(0.12345)                           # (m = 3 with three equal pairs would leave nothing off the grid)
    row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)       # would show if a spare column were read
    row[a], row[b] = x, y
    return row


@functools.lru_cache(maxsize=None)
def table(m, flavour="mixed", per_kind=1, kinds=None):
    """-> (ps float32[rows, 2 m + 3], a, b, (kind, grid)[rows]); read-only"""
    rng = np.random.default_rng(22000 + 131 * m + FLAVOURS.index(flavour))
    a, b, s = RS.draw_pairs(rng, m)
    rows, what = [], []
    for _ in range(per_kind):
        for name in (KINDS if kinds is None else kinds):
            for fl in KINDS[name]:
                if flavour in (fl, "mixed"):
                    rows.append(make_row(rng, name, fl == "grid", a, b, s))
                    what.append((name, fl == "grid"))
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, a, b, what


@functools.lru_cache(maxsize=None)
def reference(m, flavour="mixed", per_kind=1, kinds=None, conf=0.95):
    ps, a, b, _ = table(m, flavour, per_kind, kinds)
    return WR.table_reference(ps, a, b, WR.zq_of(conf))


def cases():
    """every (table arguments, conf) a GPU test runs, the two rows of LARGE pairs aside (their kept counts are checked where
    they are made): what the fixture condition is checked on"""
    out = [((m, fl), 0.95) for m in PAIRS for fl in FLAVOURS]
    out += [((m, "mixed"), conf) for m in LEVEL_PAIRS for conf in LEVELS]
    out += [((m, "mixed", 4), 0.95) for m in SLICE_PAIRS + (GROUP_PALETTE, BLOCK_PALETTE)]
    return out
