"""Tables over k sample sets for the Kruskal-Wallis and Jonckheere-Terpstra suites (helper module, no tests in here): the
random parity tables, the palette of row kinds behind the rows-per-wave tables, and the named edge rows."""
import numpy as np

from rank_support import _values as flavour_values
from rank_support import on_grid


# ------------------------------------------------------------------------------ random parity tables
def draw_sets(rng, k, lo, hi, spare=3):
    """k disjoint column lists of lo..hi columns in a shuffled table of sum + spare columns"""
    sizes = rng.integers(lo, hi + 1, size=k)
    s = int(sizes.sum()) + spare
    perm = rng.permutation(s)
    sets, at = [], 0
    for m in sizes:
        sets.append(perm[at: at + m].astype(np.int32))
        at += int(m)
    return sets, s


def values(rng, shape, sets, s, hi):
    """one row of values in [0, 1] before rounding / NaNs"""
    if shape == "uniform":
        return rng.random(s)
    if shape == "ties":
        return rng.choice([0.0, 0.5, 1.0], size=s, p=[0.4, 0.2, 0.4])
    if shape == "cluster":
        return 0.5 + 0.004 * rng.standard_normal(s)
    row = rng.random(s)
    if shape == "trend":            # set i centred at 0.5 + a (i / (k - 1) - 1/2), a = U(-6, 6) / sqrt(N), noise 0.1
        k, N = len(sets), sum(g.size for g in sets)
        a = rng.uniform(-6.0, 6.0) / np.sqrt(N)
        for i, g in enumerate(sets):
            row[g] = 0.5 + a * (i / (k - 1) - 0.5) + 0.1 * rng.standard_normal(g.size)
        return row
    for g in sets:                  # shifted normals: set means apart by about two standard errors of a set mean
        row[g] = 0.5 + 0.3 * rng.standard_normal() / np.sqrt(hi) + 0.15 * rng.standard_normal(g.size)
    return row


def table(rng, sets, s, hi, rows_per_shape, grid, shapes, starve):
    """rows_per_shape rows of every value shape of `shapes`; in the rows where starve(shape, r) holds one set falls below
    3 values"""
    rows = []
    for shape in shapes:
        for r in range(rows_per_shape):
            v = np.clip(values(rng, shape, sets, s, hi), 0.0, 1.0)
            if grid:
                row = (np.rint(v * 1000.0) / 1000.0).astype(np.float32)       # float32(k / 1000.0)
            else:
                row = (v * 1.7 - 0.3).astype(np.float32)                       # off the grid, some outside [0, 1]
                row += rng.random(s, dtype=np.float32) * np.float32(1e-3)      # random mantissas
                dup = rng.integers(0, s, size=(max(2, s // 6), 2))             # some exact duplicates
                row[dup[:, 0]] = row[dup[:, 1]]
            if r % 3 != 0:
                row[rng.random(s) < 0.06] = np.nan
            if starve(shape, r):
                g = sets[int(rng.integers(len(sets)))]
                row[g[2:]] = np.nan
            rows.append(row)
    return np.ascontiguousarray(np.stack(rows))


# ------------------------------------------------------------------------------ the palette of the rows-per-wave tables
KINDS = ("grid tested", "grid starved", "off-grid tested", "off-grid starved", "all equal on the grid",
         "all equal off the grid", "grid with NaNs")
PER_KIND = 40
PALETTE_S = 20
CHS = (64, 32, 8, 2)


def palette():
    """-> (rows float32[7 * 40, 20], sets, kind[280]): k = 3 sets of 4, 5 and 6 of the 20 columns (interleaved); the
    five other columns hold values that would show if they were read"""
    rng = np.random.default_rng(64328)
    perm = rng.permutation(PALETTE_S)
    sets = [np.sort(perm[:4]).astype(np.int32), np.sort(perm[4:9]).astype(np.int32), np.sort(perm[9:15]).astype(np.int32)]
    other = perm[15:]
    rows = np.empty((len(KINDS) * PER_KIND, PALETTE_S), np.float32)
    for r in range(rows.shape[0]):
        kind = KINDS[r // PER_KIND]
        v = r % PER_KIND
        if kind.startswith("all equal"):
            row = np.full(PALETTE_S, flavour_values(rng, 1, "q3" if kind.endswith("on the grid") else "cont")[0], np.float32)
        else:
            row = flavour_values(rng, PALETTE_S, "q3" if kind.startswith("grid") else "cont")
            if v % 4 == 1:                                   # ties across sets
                row[rng.integers(0, PALETTE_S, 6)] = row[rng.integers(0, PALETTE_S, 6)]
        g = sets[v % 3]
        if kind.endswith("starved"):
            row[g[2:]] = np.nan                              # the set keeps two values
            if v % 2:
                row[sets[(v + 1) % 3][0]] = np.nan
        elif kind == "grid with NaNs" or (kind == "off-grid tested" and v % 2):
            row[g[rng.integers(0, g.size)]] = np.nan          # every set still keeps >= 3
            if v % 2:
                row[sets[2][rng.integers(0, 3, 2)]] = np.nan
        row[other] = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=other.size)
        rows[r] = row
    return rows, sets, np.repeat(np.arange(len(KINDS)), PER_KIND)


def palette_index(n):
    """row r takes kind (r + r // 64) % 7: a 64-row chunk cycles through all kinds, and the kind at a chunk's positions
    0 and 63 moves on by two from chunk to chunk; the variant inside the kind is seeded"""
    r = np.arange(n, dtype=np.int64)
    kind = (r + r // 64) % len(KINDS)
    return kind * PER_KIND + np.random.default_rng(n).integers(0, PER_KIND, size=n)


# ------------------------------------------------------------------------------ edge values
def _edge_rows():
    """-> (ps float32[rows, 16], sets, names).  Sets: columns 0..5, 6..10, 11..15.  A row named `... / sorted` is the row
    before it with one value moved up by an ulp, which takes it off the grid and to the sorting kernel."""
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))                # noqa: E731
    down = lambda x: np.nextafter(f(x), f(-np.inf))             # noqa: E731
    nan = np.nan
    tiny = f(1e-45)                                             # the smallest float32 subnormal
    rows = {
        "-0.0 among +0.0 (one tie group)":
            [-0.0, 0.0, -0.0, 0.0, 0.5, 0.25,   -0.0, -0.0, -0.0, 0.0, 0.0,   0.1, 0.0, -0.0, 0.2, 0.3],
        "only -0.0 in every set but one":
            [-0.0, -0.0, -0.0, -0.0, -0.0, -0.0,   -0.0, -0.0, -0.0, -0.0, nan,   -0.0, -0.0, -0.0, -0.0, 0.001],
        "subnormals next to 0.0 (distinct values)":
            [0.0, tiny, 2 * tiny, -tiny, 0.0, f(1.1754942e-38),   tiny, 0.0, -0.0, 3 * tiny, -2 * tiny,
             0.0, f(1e-40), tiny, -tiny, f(1.17549435e-38)],
        "one ulp above and one ulp below a grid value, the grid value beside them":
            [0.3, up(0.3), 0.5, 0.7, 0.1, 0.9,   0.7, down(0.7), 0.3, 0.2, 0.5,   0.3, 0.7, 0.4, 0.6, 0.8],
        "just outside [0, 1]: clamp to keys 0 and 1000":
            [f(1.0004), 1.0, 0.0, 0.5, 0.25, f(-0.0004),   1.0, 0.0, f(-0.0004), 0.75, 0.5,   f(1.0004), 1.0, 0.999, 0.001, 0.0],
        "a set keeps exactly 3":
            [0.2, nan, nan, 0.8, nan, 0.5,   0.1, 0.2, nan, 0.4, 0.5,   nan, 0.9, 0.2, nan, 0.7],
        "every set keeps exactly 3, ties":
            [0.5, nan, nan, 0.5, nan, 0.25,   0.25, 0.5, nan, nan, 0.75,   nan, 0.75, 0.5, nan, 0.25],
    }
    names, table = [], []
    for name, row in rows.items():
        row = np.array(row, np.float32)
        names.append(name)
        table.append(row)
        if np.all(on_grid(row)):
            moved = row.copy()
            at = int(np.nanargmax(row))                         # the row's largest value: no order changes
            moved[at] = up(row[at])
            names.append(name + " / sorted")
            table.append(moved)
    sets = [np.arange(0, 6, dtype=np.int32), np.arange(6, 11, dtype=np.int32), np.arange(11, 16, dtype=np.int32)]
    return np.stack(table), sets, names


def _zero_sum_rows():
    """-> (ps float32[2, 20], sets): a set of ten -0.0 (a pairwise leaf with its eight accumulators; np.sum starts from the
    identity 0, so numpy's mean is +0.0) beside two sets of five, on the grid and with one value off it"""
    ps = np.empty((2, 20), np.float32)
    ps[:, :10] = -0.0
    ps[:, 10:15] = [0.1, 0.2, 0.0, 0.4, 0.5]
    ps[:, 15:] = [0.3, -0.0, 0.25, 0.125, 0.75]
    ps[1, 19] = np.float32(0.7500001)
    return ps, [np.arange(0, 10, dtype=np.int32), np.arange(10, 15, dtype=np.int32), np.arange(15, 20, dtype=np.int32)]
