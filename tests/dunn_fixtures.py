"""Tables for the Dunn's-test suites (helper module, no tests in here): every GPU fixture of tests/test_gpu_dunn.py and
tests/test_gpu_dunn_sweeps.py with its reference from tests/dunn_referee.py, built once and shared; tests/test_dunn_cpu.py
checks on the CPU that no fixture row has two pair p-values that only a rounding tells apart.

A fixture is (ps float32 [n, s], sets, label); FIXTURES maps a name to its maker, reference(name) to the referee's table
(dense-rank keys, which serve rows on and off the 3-decimal grid alike).  FLAVOURS: `grid` rows take the histogram kernel,
`off` rows (the same rows through rank_support.twin's map: same order, same ties) the sorting kernel, `mixed` interleaves the
two, so the sorting kernel takes KW_REDO rows among grid rows.

check_pairs holds the pair outputs of a call to the bars of tests/test_gpu_dunn.py (its docstring) against such a reference."""
import functools

import numpy as np

import dunn_referee as DR
import kset_fixtures as KF
import rank_support as RS
from rank_support import twin

FLAVOURS = ("grid", "off", "mixed")
KS = (2, 3, 4, 5, 10, 11)                      # m = 1, 3, 6, 10, 45, 55 pairs: the last lane in use is 0 .. 54
SHAPES = ("uniform", "shifted", "ties", "cluster")
TOTALS = tuple(range(9, 67)) + (127, 128, 129)
FIXTURES = {}
Z_ROUNDINGS = 1
PAIR = ("pair_z", "pair_p", "pair_padj")


def ulps(a, b):
    """the distance of two float64 arrays of one sign pattern in units of the last place"""
    return np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))


def check_pairs(got, ref, label):
    """the bars of the pair outputs on every row -> (tested rows, worst z distance in ulps, cells below the p floor)"""
    assert np.array_equal(got["tested"], ref["tested"]), (label, "tested")
    t = ref["tested"].astype(bool)
    m = ref["pair_z"].shape[0]
    for name in PAIR:
        if name in got:
            assert got[name].dtype == np.float64 and got[name].shape == (m, t.size), (label, name)
            assert not RS.bits(got[name][:, ~t]).any(), (label, name, "a pair slot of a row that is not tested")
    z, zr = got["pair_z"][:, t], ref["pair_z"][:, t]
    zero = ref["zero_num"][:, t]
    assert np.all(zr[zero] == 0) and np.all(zr[~zero] != 0)
    assert np.all(z[zero] == 0), (label, "z where the referee's is 0")
    assert np.array_equal(np.signbit(z[~zero]), np.signbit(zr[~zero])), (label, "sign of z")
    dist = ulps(z[~zero], zr[~zero])
    worst = int(dist.max()) if dist.size else 0
    print(f"{label}: rows {t.size} tested {int(t.sum())} pairs {m} worst z distance {worst} ulp largest |z| "
          f"{np.abs(zr).max() if zr.size else 0:.3g}", end=" ")
    assert worst <= Z_ROUNDINGS <= 8, (label, "z", worst)
    below = 0
    for name in ("pair_p", "pair_padj"):
        if name in got:
            below += RS.check_p(got[name][:, t].ravel(), ref[name][:, t].ravel(), (label, name))[0]
    if "pair_p" in got and "pair_padj" in got:
        p, padj = got["pair_p"][:, t], got["pair_padj"][:, t]
        assert np.all(padj >= p) and np.all(padj <= 1.0), (label, "padj against p and 1")
        first = np.argmin(p, axis=0)
        at = np.arange(p.shape[1])
        assert np.array_equal(padj[first, at], np.minimum(1.0, m * p[first, at])), (label, "padj of the smallest p")
        assert np.all(p[zero] == 1.0), (label, "p where z is 0")
    return int(t.sum()), worst, below


def _flavoured(grid_rows, sets, flavour):
    """a 3-decimal table as it is, as its off-grid twin, or row by row alternately"""
    if flavour == "grid":
        return grid_rows
    tw = twin(grid_rows, np.concatenate(sets))
    if flavour == "off":
        return tw
    out = grid_rows.copy()
    out[1::2] = tw[1::2]
    return out


def _fixture(name):
    def register(make):
        assert name not in FIXTURES
        FIXTURES[name] = make
        return make
    return register


def _set_count(k, flavour):
    """k sets of 3..8 columns, two rows of every value shape (NaNs, a starved set in some rows)"""
    rng = np.random.default_rng(7100 + k)
    sets, s = KF.draw_sets(rng, k, 3, 8)
    ps = KF.table(rng, sets, s, 8, 2, True, SHAPES, lambda shape, r: r == 1 and shape == "uniform")
    return _flavoured(ps, sets, flavour), sets, f"k={k} {flavour}"


def _column_counts(flavour):
    """three sets over every total column count 9..66 and 127..129 (set sizes from 3 up, the third takes the rest): one
    table per total would be 61 calls, so the totals share one table of 129 + 3 columns and every total has its own sets;
    -> list of (ps, sets, label)"""
    rng = np.random.default_rng(7200)
    s = 132
    grid = KF.table(rng, [np.arange(s)], s, 40, 2, True, ("uniform", "shifted", "ties"), lambda shape, r: False)
    out = []
    for T in TOTALS:
        perm = rng.permutation(s)[:T]
        a = T // 3
        sets = [perm[:a].astype(np.int32), perm[a: 2 * a].astype(np.int32), perm[2 * a:].astype(np.int32)]
        rows = grid.copy()
        for i, g in enumerate(sets):                      # something to find: the sets apart by a few hundredths
            rows[:, g] = np.clip(np.rint((rows[:, g] + np.float32(0.04 * i)) * 1000.0), 0, 1000) / 1000.0
        rows = rows.astype(np.float32)
        out.append((_flavoured(rows, sets, flavour), sets, f"total {T} {flavour}"))
    return out


def _unequal(big_first, flavour):
    """3 v 3 v 64 and 4096 v 3 v 3"""
    sizes = (4096, 3, 3) if big_first else (3, 3, 64)
    rng = np.random.default_rng(7300 + big_first)
    s = sum(sizes) + 2
    perm = rng.permutation(s)
    cuts = np.cumsum((0,) + sizes)
    sets = [np.sort(perm[cuts[i]: cuts[i + 1]]).astype(np.int32) for i in range(3)]
    ps = KF.table(rng, sets, s, max(sizes), 2, True, ("uniform", "shifted", "ties"), lambda shape, r: False)
    for g in sets:                                        # the sets of 3 keep their 3 values (the NaNs fall in the big one)
        if g.size == 3:
            ps[:, g] = np.where(np.isnan(ps[:, g]), np.float32(0.5), ps[:, g])
    return _flavoured(ps, sets, flavour), sets, f"sizes {sizes} {flavour}"


KIND_SETS = [np.arange(0, 6, dtype=np.int32), np.arange(6, 11, dtype=np.int32), np.arange(11, 17, dtype=np.int32),
             np.arange(17, 22, dtype=np.int32)]             # k = 4: 6, 5, 6, 5 of 24 columns; 22, 23 belong to no set
KINDS = ("NaNs scattered", "a set left with 2 kept values", "all values equal", "one set fully separated", "heavy ties",
         "two sets identical")


def _kind_rows():
    """-> (ps float32 [3 * len(KINDS), 24] of 3-decimal values, kind index per row)"""
    rng = np.random.default_rng(7400)
    nan = np.nan
    rows, kinds = [], []
    for kind, name in enumerate(KINDS):
        for v in range(3):
            row = (rng.integers(100, 901, size=24) / 1000.0).astype(np.float32)
            if name == "NaNs scattered":
                row[rng.choice(22, 4 + v, replace=False)] = nan
                row[[0, 1, 2, 6, 7, 8, 11, 12, 13, 17, 18, 19]] = (rng.integers(100, 901, size=12) / 1000.0).astype(np.float32)
            elif name == "a set left with 2 kept values":
                row[KIND_SETS[v][2:]] = nan
            elif name == "all values equal":
                row[:] = np.float32((250 + 250 * v) / 1000.0)
                row[5 * v] = nan
            elif name == "one set fully separated":
                row[KIND_SETS[v + 1]] = (rng.integers(950, 1001, size=KIND_SETS[v + 1].size) / 1000.0).astype(np.float32)
            elif name == "heavy ties":
                row[:] = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=24, p=[0.4, 0.2, 0.4])
                row[KIND_SETS[v][:3]] = np.float32(1.0)
            else:                                          # sets 1 and 3 (5 columns each) hold the same values: z = 0
                row[KIND_SETS[3]] = row[KIND_SETS[1]][::-1] if v else row[KIND_SETS[1]]
                if v == 2:
                    row[KIND_SETS[1][0]] = row[KIND_SETS[3][4]] = nan
            row[22:] = [nan, 1e30][v % 2]
            rows.append(row)
            kinds.append(kind)
    return np.stack(rows), np.array(kinds)


def _kinds(flavour):
    rows, _ = _kind_rows()
    clean = rows.copy()
    clean[:, 22:] = np.nan                                 # (twin() wants grid values in the columns it is told of only)
    out = _flavoured(clean, KIND_SETS, flavour)
    out[:, 22:] = rows[:, 22:]
    return out, KIND_SETS, f"row kinds {flavour}"


def _block_edges():
    """the sorting kernel's own values, k = 3 sets of 5: signed zeros (one tie group), subnormals (distinct values),
    +-FLT_MAX"""
    f = np.float32
    tiny, big = f(1e-45), np.finfo(np.float32).max
    rows = np.array([
        [-0.0, 0.0, -0.0, 0.25, 0.5,   0.0, -0.0, 0.0, 0.125, 0.75,   -0.0, -0.0, 0.0, 0.0, f(0.37500003)],
        [0.0, tiny, 2 * tiny, -tiny, f(1e-40),   tiny, 0.0, -0.0, 3 * tiny, -2 * tiny,   f(1.1754942e-38), -tiny, tiny, 0.0, 4 * tiny],
        [big, -big, 0.5, 0.25, -0.5,   -big, -big, 0.0, 1.0, big,   big, big, 0.75, -big, 2.0],
        [big, big, big, 0.5, np.nan,   -big, -big, -big, np.nan, 0.5,   0.5, 0.25, 0.75, big, -big],
    ], dtype=np.float32)
    sets = [np.arange(0, 5, dtype=np.int32), np.arange(5, 10, dtype=np.int32), np.arange(10, 15, dtype=np.int32)]
    return rows, sets, "signed zeros, subnormals, +-FLT_MAX"


LADDER_A, LADDER_STEPS = 1400, 24


def _ladder(flavour):
    """k = 3: two sets of 1400 columns and one of 3; in row t a share g_t of the first set's columns holds values above all
    of the second set's, g from 0 (both sets hold the same multiset of values: z = 0 exactly) to 1 (fully separated:
    z = sqrt(3 * 1400 / 2) = 45.8, p far below the float64 range)"""
    rng = np.random.default_rng(7500)
    a = LADDER_A
    perm = rng.permutation(2 * a + 3)
    sets = [np.sort(perm[:a]).astype(np.int32), np.sort(perm[a: 2 * a]).astype(np.int32), np.sort(perm[2 * a:]).astype(np.int32)]
    g = np.concatenate([[0.0], np.geomspace(0.002, 1.0, LADDER_STEPS - 1)])
    ps = np.empty((LADDER_STEPS, 2 * a + 3), np.float32)
    for t in range(LADDER_STEPS):
        low = rng.integers(100, 500, size=a)
        high = low.copy()
        up = rng.choice(a, int(round(g[t] * a)), replace=False)
        high[up] = rng.integers(500, 900, size=up.size)
        ps[t, sets[0]] = (rng.permutation(high) / 1000.0).astype(np.float32)
        ps[t, sets[1]] = (low / 1000.0).astype(np.float32)
        ps[t, sets[2]] = np.float32([0.3, 0.5, 0.7])
    return _flavoured(ps, sets, flavour), sets, f"ladder {flavour}"


for _fl in FLAVOURS:
    for _k in KS:
        _fixture(f"set count k={_k} {_fl}")(functools.partial(_set_count, _k, _fl))
    for _big in (False, True):
        _fixture(f"unequal {'4096v3v3' if _big else '3v3v64'} {_fl}")(functools.partial(_unequal, _big, _fl))
    _fixture(f"row kinds {_fl}")(functools.partial(_kinds, _fl))
for _fl in ("grid", "off"):
    _fixture(f"ladder {_fl}")(functools.partial(_ladder, _fl))
_fixture("block edges")(_block_edges)


@functools.lru_cache(maxsize=None)
def fixture(name):
    ps, sets, label = FIXTURES[name]()
    ps.setflags(write=False)
    return ps, sets, label


@functools.lru_cache(maxsize=None)
def reference(name):
    ps, sets, _ = fixture(name)
    with np.errstate(over="ignore"):                       # (np.mean of +-FLT_MAX values: inf, as the kernels' means)
        return DR.table_reference(ps, sets, False)


@functools.lru_cache(maxsize=None)
def column_count_fixtures(flavour):
    return tuple(_column_counts(flavour))


@functools.lru_cache(maxsize=None)
def column_count_references(flavour):
    return tuple(DR.table_reference(ps, sets, False) for ps, sets, _ in column_count_fixtures(flavour))


@functools.lru_cache(maxsize=None)
def palette_reference():
    """the referee's table of kset_fixtures.palette() (k = 3, 280 rows of seven kinds), for the rows-per-wave tables"""
    rows, sets, _ = KF.palette()
    return DR.table_reference(rows, sets, False)
