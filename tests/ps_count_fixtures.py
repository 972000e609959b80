"""Count tables for the PS kernels (ps.hip) over the whole int32 range that the ABI accepts (counts[n,s] int32, sdice.h),
with the integer oracle they are checked against.  Used by test_gpu_ps_counts.py and test_gpu_ps_plans.py; every claim
made here about a fixture is asserted without a GPU by test_ps_count_fixtures_cpu.py.

The kernels keep 32-bit sums and one float32 division (the "fast item") while (degree + 1) x (largest count a tile has
loaded) stays below 2^24, and 64-bit sums with a float64 division (the "slow item") from there on:

  ps_tile_v3_kernel   per item: fast iff (degree + 1) <= 0xFFFFFF / tile_cmax, degree < 254, every neighbour staged
  ps_tile_kernel      per tile: fast iff tile_cmax <= 0xFFFFFF / (tile_dmax + 1), list total within the LDS stage

tile_cmax is taken over the staged window: the tile's own rows and `halo` rows on either side (all of them when the
lists are not the context's own: then there are no reach words).  A neighbour beyond the window is read from global
memory by the slow item and does not enter the bound.  The first totals at which the float32 path would be wrong are
the odd ones above 2^24 (2^24 itself is a float32); a tile whose bound is exactly 2^24 cannot hold one (a total is at
most (degree + 1) x tile_cmax), so the cells on which a bound one step too loose shows sit in tiles at 2^24 + 1 and
just above.
"""
import fractions
import functools
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_loci_fixtures as DL  # noqa: E402   (the "star" and "hb" loci and their layout helper)
from oracle import oracle_np as O  # noqa: E402

F24 = 1 << 24
I31 = (1 << 31) - 1
PALETTE = (2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, F24 - 1, F24, F24 + 1, 2 ** 30, 2 ** 31 - 2, I31)
SMALL = (0, 1, 2, 3, 7, 30, 0, 5)
MIX = tuple(x for pair in zip(PALETTE, SMALL + (11,)) for x in pair)          # large and small counts alternate


# ------------------------------------------------------------------------------------------------ the oracle
def oracle(counts, row_ptr, col):
    """-> (ps float32 [n, s], excl int64 [n, s]): excl = int64 sums over the lists, ps = float32(float64(incl) /
    float64(incl + excl)), 0 / 0 -> NaN.  Integers all the way to the one float64 division: int32 counts widen to
    int64, the sums are an int64 sparse product, incl + excl is an int64 sum below 2^53 (asserted), so both operands of
    the division are exact."""
    counts = np.asarray(counts)
    assert counts.dtype == np.int32 and counts.min(initial=0) >= 0
    n = counts.shape[0]
    c64 = counts.astype(np.int64)
    adj = scipy.sparse.csr_matrix((np.ones(len(col), np.int64), np.asarray(col, np.int64), np.asarray(row_ptr, np.int64)),
                                  shape=(n, n))
    excl = np.asarray(adj @ c64, dtype=np.int64)
    total = c64 + excl
    assert excl.dtype == np.int64 and total.max(initial=0) < 2 ** 53
    with np.errstate(invalid="ignore", divide="ignore"):
        ps = (c64.astype(np.float64) / total.astype(np.float64)).astype(np.float32)
    return ps, excl


def same_ps(a, b):
    """float32 bit patterns are equal, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def fraction_cell(counts, row_ptr, col, r, c):
    """(ps, excl) of one cell in rational arithmetic: Python integers, the quotient as a Fraction, rounded once to
    float64 (Fraction.__float__ rounds correctly) and from there to float32, as the contract words it"""
    incl = int(counts[r, c])
    excl = sum(int(counts[j, c]) for j in col[row_ptr[r]:row_ptr[r + 1]])
    if incl + excl == 0:
        return np.float32(np.nan), excl
    return np.float32(float(fractions.Fraction(incl, incl + excl))), excl


def float32_path(counts, row_ptr, col, r, c):
    """what 32-bit arithmetic would store in one cell, two ways: the exact total converted to float32 and divided in
    float32 (the fast item), and the total accumulated in float32 in list order"""
    incl = int(counts[r, c])
    nb = [int(counts[j, c]) for j in col[row_ptr[r]:row_ptr[r + 1]]]
    acc = np.float32(incl)
    for x in nb:
        acc = np.float32(acc + np.float32(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(incl) / np.float32(incl + sum(nb)), np.float32(incl) / acc


class Fixture:
    def __init__(self, counts, row_ptr, col, show=(), marks=None):
        self.counts = np.ascontiguousarray(counts, np.int32)
        self.row_ptr, self.col = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32)
        self.show = tuple(show)             # (row, column): cells on which 32-bit arithmetic gives other bits
        self.marks = marks or {}            # name -> first row of the tile that the name describes
        for a in (self.counts, self.row_ptr, self.col):
            a.setflags(write=False)

    @property
    def n(self):
        return self.counts.shape[0]

    @property
    def s(self):
        return self.counts.shape[1]

    @functools.cached_property
    def want(self):
        """(ps, excl, '.3f' ps), computed once and read-only"""
        ps, excl = oracle(self.counts, self.row_ptr, self.col)
        q = O.quantize3_fast(ps)
        for a in (ps, excl, q):
            a.setflags(write=False)
        return ps, excl, q

    def designed_cells(self):
        """the cells that the CPU test walks in rational arithmetic: every cell of a row with neighbours, or, on the
        larger fixtures, of the rows around every mark and every show cell"""
        rows = set(r for r, _ in self.show)
        for r0 in self.marks.values():
            rows.update(range(r0, min(r0 + 4, self.n)))
        if self.n <= 64:
            rows.update(range(self.n))
        return [(r, c) for r in sorted(rows) for c in range(min(self.s, 12))]


# ------------------------------------------------------------------------------------------------ builder
class _Builder:
    """rows appended one group at a time; any CSR over the rows is valid input (sdice.h), lists need not be symmetric"""

    def __init__(self, s, seed):
        self.s, self.rng = s, np.random.default_rng(seed)
        self.lists, self.rows, self.show, self.marks = [], [], [], {}

    @property
    def n(self):
        return len(self.lists)

    def singles(self, m, below=4):
        """m rows without neighbours, counts below `below`"""
        for _ in range(m):
            self.lists.append([])
            self.rows.append(self.rng.integers(0, below, self.s))
        return self

    def pad_to(self, R):
        return self.singles(-self.n % R)

    def group(self, counts, lists):
        """rows with the given counts [k, s]; lists[i] = neighbours of row i as indices into the group"""
        at = self.n
        for i, row in enumerate(np.asarray(counts, np.int64)):
            assert row.min() >= 0 and row.max() <= I31
            self.lists.append([at + j for j in lists[i]])
            self.rows.append(row)
        return at

    def fan(self, counts):
        """every row lists all the others (rotated, so list order differs from row order)"""
        k = len(counts)
        return self.group(counts, [[(i + 1 + j) % k for j in range(k - 1)] for i in range(k)])

    def star(self, counts):
        """row 0 lists all the others, each of which lists row 0"""
        k = len(counts)
        return self.group(counts, [list(range(1, k))] + [[0]] * (k - 1))

    def done(self):
        row_ptr = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])])
        col = np.asarray([j for x in self.lists for j in x], np.int32)
        return Fixture(np.stack(self.rows), row_ptr, col, self.show, self.marks)


def fan_counts(k, cap, s):
    """counts [k, s] of a fan whose largest count is `cap`.  Column 0: every row at cap, total k cap.  Column c >= 1:
    total k cap - d_c, d_c = fix + 2 ((c - 1) mod 4), fix = 1 when k cap is even: odd totals within 7 of k cap, taken
    off row c mod k."""
    out = np.full((k, s), cap, np.int64)
    fix = 1 - (k * cap) % 2
    for c in range(1, s):
        out[c % k, c] -= fix + 2 * ((c - 1) % 4)
    return out


def _show_cells(fan, at, k, s):
    """cells of the first three rows of the fan at row `at` whose total is odd and above 2^24 and whose float32 quotient
    of the float32 total is not the contract's value (most are; the CPU test asserts it for every cell returned)"""
    tot = fan.sum(0)
    out = []
    for c in range(min(s, 8)):
        for i in range(min(k, 3)):
            if tot[c] > F24 and tot[c] % 2 and np.float32(fan[i, c]) / np.float32(tot[c]) != np.float32(fan[i, c] / tot[c]):
                out.append((at + i, c))
    return out


# ------------------------------------------------------------------------------------------------ palette
STAR_D = 40


def _palette_counts(n, s, hub, d):
    c = np.zeros((n, s), np.int64)
    for r in range(n):
        for k in range(s):
            c[r, k] = MIX[(5 * r + 7 * k) % len(MIX)]
    c[:, s - 1] = 0                                        # 0 / 0 in every row
    c[hub, 1] = 0                                          # PS 0 on the hub, 1 on its leaves
    c[hub + 1:hub + 1 + d:2, 2] = 0                        # PS 0 on every other leaf
    c[hub + 1:hub + 1 + d, 3] = 0                          # PS 1 on the hub
    c[hub, 3] = I31
    return c


@functools.lru_cache(maxsize=None)
def palette(s):
    """3 rows without neighbours, a hub over STAR_D leaves, 5 more rows: every magnitude of PALETTE, alone and in sums
    with every other, on the hub (degree 40) and on the leaves (degree 1)"""
    c = _palette_counts(3 + 1 + STAR_D + 5, s, 3, STAR_D)
    b = _Builder(s, 1)
    b.group(c[:3], [[]] * 3)                               # (the rows without neighbours carry the palette too)
    b.marks["hub"] = b.star(c[3:4 + STAR_D])
    b.group(c[4 + STAR_D:], [[]] * 5)
    return b.done()


@functools.lru_cache(maxsize=None)
def palette_junctions():
    """the same rows as junctions (clustered on the device: the lists are the context's own, reach words exist)"""
    return DL._Layout().singletons(3).star(STAR_D).singletons(5).arrays()


@functools.lru_cache(maxsize=None)
def palette_on_device_lists(s):
    row_of, row_ptr, col = O.cluster_csr(*palette_junctions())
    assert np.array_equal(row_of, np.arange(row_of.size))
    return Fixture(palette(s).counts, row_ptr, col, marks={"hub": 3})


# ------------------------------------------------------------------------------------------------ the 2^24 bound
BOUND_R, BOUND_HALO = 128, 16              # ps.tile_rows of the bound fixture; the halo the planner gives a foreign list
CAP16 = (F24 - 1) // 16                    # 1 048 575: 16 x CAP16 = 2^24 - 16, the largest fast count at degree 15
CAP3 = (F24 - 1) // 3                      # 5 592 405: 3 x CAP3 = 2^24 - 1
CAP97 = (F24 + 1) // 97                    # 172 961: 97 x CAP97 = 2^24 + 1
CAP17 = 986897                             # 17 x CAP17 = 2^24 + 33
# the halo tiles: a fan of 16 at HALO_OWN, three rows of which also list one halo row (degree 16): 17 x HALO_OWN < 2^24, so
# the own rows alone leave every item fast; the halo row holds HALO_FAST (17 x HALO_FAST = 2^24 - 1: still fast) or
# HALO_SLOW + 2 (column mod 4) (17 x that is above 2^24: slow because of the halo count alone, and the listing rows' totals
# 16 x HALO_OWN + halo count are odd and above 2^24)
HALO_OWN, HALO_FAST, HALO_SLOW = 986890, (F24 - 1) // 17, 987001
HALO_LISTERS = (4, 5, 6)                   # rows of the tile that list the halo row
# name -> (what (tile_dmax + 1) x tile_cmax must be, which side of the bound)
BOUND_TILES = {
    "own_fast16": (16 * CAP16, "fast"), "own_slow16": (F24, "slow"), "own_fast3": (F24 - 1, "fast"),
    "own_slow3": (F24 + 2, "slow"), "own_slow97": (F24 + 1, "slow"), "own_slow17": (F24 + 33, "slow"),
    "below_fast": (17 * HALO_FAST, "fast"), "below_slow": (17 * (HALO_SLOW + 6), "slow"),
    "above_fast": (17 * HALO_FAST, "fast"), "above_slow": (17 * (HALO_SLOW + 6), "slow"),
    "outside": (16 * CAP16, "fast"), "per_item": (17 * CAP16, "slow"),
}
SHOW_TILES = ("own_slow3", "own_slow97", "own_slow17", "per_item", "below_slow", "above_slow")


@functools.lru_cache(maxsize=None)
def bound(s):
    """tiles of BOUND_R rows, every second one a tile of rows without neighbours and counts below 4.  The named tiles:
      own_*        a fan at the head of the tile whose own counts set the bound: 16 x 1 048 575 and 3 x 5 592 405 =
                   2^24 - 1 (fast), 16 x 2^20 = 2^24, 97 x 172 961 = 2^24 + 1, 3 x 5 592 406 = 2^24 + 2 and 17 x 986 897 =
                   2^24 + 33 (slow)
      below_*      a fan of 16 at 986 890, three rows of which also list the row in front of the tile (above_*: the row
                   behind it), which lists nobody: 17 x 986 890 < 2^24, and the count in that halo row sets the bound --
                   986 895 (17 x = 2^24 - 1, fast) or 987 001 .. 987 007 (slow; the listing rows' totals are odd and above
                   2^24, so a bound taken over the own rows alone stores other bits)
      outside      a fan at 1 048 575 and a fan of three small rows, one of which also lists a row of 2^31 - 1 far in
                   front of the tile: that item leaves the window, the tile's bound stays (degree 3, and the far
                   count is never staged)
      per_item     a fan of 16 and a fan of 17 at 1 048 575 in one tile: 16 x cap < 2^24 < 17 x cap, so the register-
                   staged kernel takes the short rows fast and the long rows slow (the first-generation kernel decides
                   for the whole tile: slow)"""
    R = BOUND_R
    b = _Builder(s, 2)

    def tile(name, fans):
        b.pad_to(R)
        b.marks[name] = b.n
        for k, cap in fans:
            cnt = fan_counts(k, cap, s)
            at = b.fan(cnt)
            if name in SHOW_TILES:
                b.show.extend(_show_cells(cnt, at, k, s))
        b.pad_to(R)
        b.singles(R)

    b.singles(R)
    far = R // 2                                     # a row no window of a named tile holds
    tile("own_fast16", [(16, CAP16)])
    tile("own_slow16", [(16, CAP16 + 1)])
    tile("own_fast3", [(3, CAP3)])
    tile("own_slow3", [(3, CAP3 + 1)])
    tile("own_slow97", [(97, CAP97)])
    tile("own_slow17", [(17, CAP17)])
    cols = np.arange(s)
    for where in ("below", "above"):
        for side, value in (("fast", np.full(s, HALO_FAST)), ("slow", HALO_SLOW + 2 * (cols % 4))):
            name = f"{where}_{side}"
            b.pad_to(R)
            r0 = b.marks[name] = b.n
            own = np.full((16, s), HALO_OWN, np.int64)
            own[1] -= 2 * (cols % 3)
            b.fan(own)
            b.pad_to(R)
            b.singles(R)
            halo_row = r0 - 1 if where == "below" else r0 + R
            b.rows[halo_row][:] = value
            for i in HALO_LISTERS:
                b.lists[r0 + i].append(halo_row)
                if side == "slow":
                    for c in range(min(s, 8)):
                        tot = int(own[:, c].sum() + value[c])
                        if np.float32(own[i, c]) / np.float32(tot) != np.float32(own[i, c] / tot):
                            b.show.append((r0 + i, c))
    tile("outside", [(16, CAP16), (3, 1000)])
    b.lists[b.marks["outside"] + 17].append(far)
    b.rows[far][:] = I31
    tile("per_item", [(16, CAP16), (17, CAP16)])
    return b.done()


def tile_bounds(fx, R, halo):
    """per tile of R rows: (tile_dmax + 1) x tile_cmax with tile_cmax over the window of `halo` rows on either side, and
    the same per row with the row's own degree (what the register-staged kernel compares per item)"""
    deg = np.diff(fx.row_ptr)
    per_tile, per_row = {}, np.zeros(fx.n, np.int64)
    for r0 in range(0, fx.n, R):
        r1 = min(r0 + R, fx.n)
        cmax = int(fx.counts[max(r0 - halo, 0):r1 + halo].max())
        per_tile[r0] = (int(deg[r0:r1].max()) + 1) * cmax
        per_row[r0:r1] = (deg[r0:r1] + 1) * cmax
    return per_tile, per_row


# ------------------------------------------------------------------------------------------------ large sums
TIE_KEYS = (1, 3, 5, 25, 125, 999, 1001, 1999)         # k / 2000 = x.xxx5: a '.3f' tie in exact arithmetic
TIE_UNIT = 1 << 20


@functools.lru_cache(maxsize=None)
def large_sums(s=8):
    """stars of 600 and of 3000 leaves with every count at 2^31 - 1 (exclusion sums of 600 and 3000 x (2^31 - 1): past
    2^40), a fan of four all-zero rows (NaN), pairs (x, 0) (PS 1 and 0) and pairs (k 2^20, (2000 - k) 2^20): PS k / 2000,
    the decimal ties of the '.3f' store, from totals of 2000 x 2^20"""
    b = _Builder(s, 3)
    b.singles(5)
    for d in (600, 3000):
        b.marks[f"star{d}"] = b.star(np.full((d + 1, s), I31, np.int64))
        b.singles(7)
    b.marks["zeros"] = b.fan(np.zeros((4, s), np.int64))
    one = np.zeros((2, s), np.int64)
    one[0] = [PALETTE[c % len(PALETTE)] for c in range(s)]
    b.marks["one_zero"] = b.fan(one)
    for i in range(len(TIE_KEYS)):
        k = np.asarray([TIE_KEYS[(i + c) % len(TIE_KEYS)] for c in range(s)], np.int64)
        at = b.fan(np.stack([k * TIE_UNIT, (2000 - k) * TIE_UNIT]))
        b.marks.setdefault("ties", at)
        b.marks[f"tie{i}"] = at
    b.singles(3)
    return b.done()


# ------------------------------------------------------------------------------------------------ dense loci
BIGS = (F24, F24 + 1, 2 ** 30, 2 ** 31 - 2, I31, F24 + 3)


@functools.lru_cache(maxsize=None)
def dense(name):
    """the "star" (degrees 252 .. 256 and 300) and "hb" (reach 255 .. 257) loci of dense_loci_fixtures with their counts,
    and in every row one value at or above 2^24 (column r mod S of row r): no tile keeps 32-bit sums, so the degree
    cutoff of the fast item, a list total beyond the offset stage and neighbours beyond the halo all meet 64-bit sums"""
    assert name in ("star", "hb")
    _, row_ptr, col = DL.oracle_csr(name)
    c = np.array(DL.counts(name))
    r = np.arange(c.shape[0])
    c[r, r % DL.S] = np.asarray(BIGS, np.int64)[r % len(BIGS)].astype(np.int32)
    deg = np.diff(row_ptr)
    rows = np.flatnonzero(deg > 1) if name == "star" else np.asarray([0, 300, c.shape[0] // 2, c.shape[0] - 1])
    return Fixture(c, row_ptr, col, marks={f"row{i}": int(i) for i in rows})


# ------------------------------------------------------------------------------------------------ gene-shaped tables
@functools.lru_cache(maxsize=None)
def gene_csr(n, seed=5):
    """(row_ptr, col) of n gene-shaped junctions (synth.make_junctions) in row order, plus one far-reaching pair: row 1
    and row n - 2 list each other, further apart than any halo, so the global-memory path runs whatever the plan"""
    from splicedice_amd import synth
    _, row_ptr, col = O.cluster_csr(*synth.make_junctions(n, seed))
    lists = [col[row_ptr[r]:row_ptr[r + 1]].tolist() for r in range(n)]
    lists[1].append(n - 2)
    lists[n - 2].insert(0, 1)
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    cl = np.asarray([j for x in lists for j in x], np.int32)
    for a in (rp, cl):
        a.setflags(write=False)
    return rp, cl


@functools.lru_cache(maxsize=None)
def gene_table(n, s, seed=5):
    """gene_csr(n) with counts below 40, zeros included, a few rows of the palette and one row at 2^31 - 1"""
    rng = np.random.default_rng([seed, n, s])
    c = rng.integers(0, 40, (n, s)).astype(np.int64)
    c[rng.random(n) < 0.05] = 0
    c[:, s // 2] = np.where(rng.random(n) < 0.5, 0, c[:, s // 2])
    for i, r in enumerate(range(7, n, max(n // 9, 1))):
        c[r] = MIX[(i * 2) % len(MIX)]
    c[n - 2] = I31
    rp, cl = gene_csr(n, seed)
    return Fixture(c, rp, cl)


def wide(s, chunk=128):
    """6 rows that all list each other, s columns: counts in the first, a middle and the last column chunk, zeros (NaN)
    everywhere else; -> (counts, row_ptr, col, ps, excl) with the oracle taken on the three chunks alone"""
    n = 6
    row_ptr = np.arange(n + 1, dtype=np.int64) * (n - 1)
    col = np.asarray([(i + 1 + j) % n for i in range(n) for j in range(n - 1)], np.int32)
    counts = np.zeros((n, s), np.int32)
    mid = (s // chunk // 2) * chunk
    last = (s - 1) // chunk * chunk
    spans = [(0, chunk), (mid, mid + chunk), (last, s)]
    rng = np.random.default_rng(s)
    for a, b in spans:
        block = rng.integers(0, 50, (n, b - a)).astype(np.int64)
        block[:, ::5] = np.asarray(PALETTE, np.int64)[rng.integers(0, len(PALETTE), (n, len(range(a, b, 5))))]
        block[:, 1] = 0
        counts[:, a:b] = block
    ps = np.full((n, s), np.nan, np.float32)
    excl = np.zeros((n, s), np.int64)
    for a, b in spans:
        ps[:, a:b], excl[:, a:b] = oracle(np.ascontiguousarray(counts[:, a:b]), row_ptr, col)
    return counts, row_ptr, col, ps, excl, spans


# ------------------------------------------------------------------------------------------------ running a fixture
OUTPUTS = (("both", True, True), ("excl", True, False), ("ps", False, True))
FILL = 0xA5
PS_KERNELS = {0: "ps_tile_v3_kernel", 2: "ps_tile_kernel"}


class Resident:
    """a table and its lists on the device, the outputs beside them; check() runs sdice_ps_dev with both outputs, excl
    alone and ps alone, each with ps.quantize3 0 and 1, on outputs filled with 0xA5, and compares bit for bit (NaN =
    NaN) with `want` = (ps, excl, '.3f' ps).  -> the plan of the launches (sdice_ps_last_plan), which is the same for
    all six but for q3; `seen` collects every plan."""

    def __init__(self, ctx, counts, row_ptr, col, want, d_rp=None, d_col=None):
        self.ctx, self.want = ctx, want
        self.n, self.s = counts.shape
        self.d_counts = ctx.to_device(counts, np.int32)
        self.d_rp = ctx.to_device(row_ptr, np.int64) if d_rp is None else d_rp
        self.d_col = ctx.to_device(col if len(col) else np.zeros(1, np.int32), np.int32) if d_col is None else d_col
        self.d_excl, self.d_ps = ctx.empty((self.n, self.s), np.int64), ctx.empty((self.n, self.s), np.float32)

    def launch(self, knobs, want_excl=True, want_ps=True, args=None):
        """-> (ps or None, excl or None, plan, {kernel: launches})"""
        ctx = self.ctx
        d_counts, d_excl, d_ps = args or (self.d_counts, self.d_excl, self.d_ps)
        with ctx.params(knobs):
            self.d_excl.memset(FILL)
            self.d_ps.memset(FILL)
            ctx.prof_enable(1)
            ctx.prof_reset()
            try:
                ctx.ps_dev(d_counts, self.d_rp, self.d_col, d_excl if want_excl else None, d_ps if want_ps else None)
                ran = {name: ctx.prof_query(name)[0] for name in PS_KERNELS.values()}
            finally:
                ctx.prof_enable(0)
            plan = ctx.ps_last_plan()
        return d_ps.to_host(), d_excl.to_host(), plan, ran

    def check(self, knobs, expect=None, seen=None, what=""):
        ps_want, excl_want, q_want = self.want
        fill_ps = np.full(1, FILL * 0x01010101, np.uint32).view(np.float32)[0]
        fill_excl = np.full(1, FILL * 0x0101010101010101, np.uint64).view(np.int64)[0]
        plan0 = None
        for name, want_excl, want_ps in OUTPUTS:
            for q3 in (0, 1):
                ps, excl, plan, ran = self.launch({**knobs, "ps.quantize3": q3}, want_excl, want_ps)
                tag = f"{what} {knobs} outputs={name} q3={q3} plan={plan} launches={ran}"
                if seen is not None:
                    seen.append(plan)
                assert plan["q3"] == q3, tag
                assert ran[PS_KERNELS[plan["kern"]]] == 1 and sum(ran.values()) == 1, tag
                for key, value in (expect or {}).items():
                    assert plan[key] == value, f"{key}: {tag}"
                shape = {k: v for k, v in plan.items() if k != "q3"}
                assert plan0 is None or shape == plan0, tag
                plan0 = shape
                if want_ps:
                    assert same_ps(ps, q_want if q3 else ps_want), _first_diff(ps, q_want if q3 else ps_want, tag)
                else:
                    assert (ps.view(np.uint32) == fill_ps.view(np.uint32)).all(), tag
                if want_excl:
                    assert excl.dtype == np.int64 and np.array_equal(excl, excl_want), _first_diff(excl, excl_want, tag)
                else:
                    assert (excl == fill_excl).all(), tag
        return plan0


def _first_diff(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    bad = ~((got == want) | ((got != got) & (want != want)))
    at = np.argwhere(bad)[:4]
    return f"{int(bad.sum())} cells differ, first {[(tuple(map(int, i)), got[tuple(i)], want[tuple(i)]) for i in at]}: {tag}"
