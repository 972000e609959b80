"""What the pair suites share (helper module, no tests in here): the palettes of (incl, excl) entries with their
references per distinct 2x2 table (scipy.stats.fisher_exact and an exact rational sum, scipy chi2_contingency) and the
element-wise comparison, of tests/test_gpu_pair_sweeps.py and tests/test_gpu_pair_list.py; the host stand-in engine and
argument helpers of the `pairwise --pairs` tests; the recording engine, array and communicator doubles of the sharded
pipelines' step() tests; the large-count rows of tests/test_gpu_pair_large_counts.py and tests/test_fisher_referee_cpu.py."""
import argparse
import contextlib
import io
import math
import os
import warnings
from fractions import Fraction

import numpy as np

from oracle import oracle_np as O

P_RTOL_TIGHT = 1e-9    # p-values (tests/test_gpu_parity.py)
P_RTOL_BIG = 1e-7      # Fisher tables with a total above 5e4: pmf(a) = exp of nine log-factorials (test_fisher_fuzz_tables)
BIG_TOTAL = 50_000
EXACT_MAX_TOTAL = 400  # the rational sum is used where the total (so every margin) is at most this

# (incl, excl) per sample.  A pair (i, j) is the table [[incl_i, incl_j], [excl_i, excl_j]].
PALETTES = {
    # zero margins (p = 1; chi2 raises), a = 0 or a at the top of the support (one-sided walks), expected == observed
    "zeros": [(0, 0), (0, 9), (6, 0), (1, 0), (0, 1), (5, 5), (3, 12), (11, 2)],
    # (x, y) beside (y, x): symmetric tables, pmf(k) == pmf(a) for a k on the other side of the mode
    "ties": [(4, 9), (9, 4), (20, 7), (7, 20), (13, 13), (1, 6), (6, 1), (30, 30)],
    # margins up to ~200 (the rational sum), a at either end of the support, p down to ~1e-77
    "small": [(17, 60), (45, 12), (2, 90), (80, 3), (33, 33), (0, 140), (120, 0), (9, 25)],
    # counts in the thousands: walks of hundreds of steps, rescaled products, the negligible-tail cut
    "thousands": [(2500, 9000), (3300, 12000), (2900, 8800), (3100, 11500), (2700, 9900), (3000, 10400)],
    # totals above 5e4
    "big": [(9000, 30000), (8000, 29000), (10500, 31000), (8800, 33000)],
    # hundreds of sigma out: p down to ~1e-267 (scipy is reliable above ~1e-280)
    "tiny": [(450, 3), (2, 440), (430, 0), (0, 460), (440, 6), (5, 450), (300, 300)],
    # fisher.table_max = 256: totals 128 + 128 = T (lgamma), 127 + 128 = T - 1 (the last table entry), 127 + 127
    "edge": [(40, 88), (100, 27), (3, 125), (64, 64), (1, 126), (0, 128), (120, 8), (0, 0)],
    # every total below T = 256: a row of these is never flagged
    "under": [(100, 27), (1, 126), (60, 67), (0, 0), (20, 20), (5, 0)],
    # a bit of everything, for rows where long walks must stay rare (s = 8192, 20 000 junctions): see MIX_WEIGHTS
    "mix": [(0, 0), (0, 9), (6, 0), (13, 13), (7, 20), (20, 7), (45, 12), (2, 90), (450, 3), (2, 440), (2900, 8800),
            (2800, 9000)],
}
MIX_WEIGHTS = np.array([8, 8, 8, 10, 10, 10, 10, 10, 1, 1, 0.5, 0.5])
SWEEP = ("zeros", "ties", "small", "thousands", "big", "tiny", "mix")
TABLE_MAX_T = 256


# ------------------------------------------------------------------------------ references per distinct table
def exact_two_sided(a, b, c, d):
    """scipy's two-sided Fisher p in rational arithmetic: the sum of pmf(k) over the support with
    pmf(k) <= pmf(a) (1 + 1e-12) (the acceptance rule of tools/exact_fisher.py), any zero margin -> 1, clipped at 1.
    pmf(k) = comb(n1, k) comb(n2, n - k) / comb(M, n): the weights share the denominator, so the test is on integers."""
    n1, n2, n = a + b, c + d, a + c
    if n1 == 0 or n2 == 0 or n == 0 or b + d == 0:
        return 1.0
    w = [math.comb(n1, k) * math.comb(n2, n - k) for k in range(max(0, n - n2), min(n1, n) + 1)]
    wa = math.comb(n1, a) * math.comb(n2, n - a)
    acc = sum(x for x in w if x * 10 ** 12 <= wa * (10 ** 12 + 1))
    return float(min(Fraction(acc, math.comb(n1 + n2, n)), Fraction(1)))


_FISHER, _CHI2 = {}, {}


def fisher_scipy(t):
    if t not in _FISHER:
        from scipy.stats import fisher_exact
        a, b, c, d = t
        _FISHER[t] = float(fisher_exact([[a, b], [c, d]])[1])
    return _FISHER[t]


def chi2_scipy(t):
    """p of scipy chi2_contingency, NaN where scipy raises (a zero expected frequency: the kernel's n_bad)"""
    if t not in _CHI2:
        from scipy.stats import chi2_contingency
        a, b, c, d = t
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            try:
                _CHI2[t] = float(chi2_contingency([[a, b], [c, d]])[1])
            except ValueError:
                _CHI2[t] = math.nan
    return _CHI2[t]


def _pack(t):
    assert (t >= 0).all() and (t < 1 << 16).all()
    return (t[..., 0] << 48) | (t[..., 1] << 32) | (t[..., 2] << 16) | t[..., 3]


class PaletteRef:
    """The distinct tables of a set of palettes (np.unique on packed keys), their references, and the table id of every
    ordered palette pair: ids[k, x, y] for samples of palette k holding entries x and y."""

    def __init__(self, names):
        self.names = list(names)
        pmax = max(len(PALETTES[nm]) for nm in self.names)
        tabs = np.zeros((len(self.names), pmax, pmax, 4), np.int64)
        for k, nm in enumerate(self.names):
            pal = np.array(PALETTES[nm], np.int64)
            p = len(pal)
            tabs[k, :p, :p, 0] = pal[:, None, 0]
            tabs[k, :p, :p, 1] = pal[None, :, 0]
            tabs[k, :p, :p, 2] = pal[:, None, 1]
            tabs[k, :p, :p, 3] = pal[None, :, 1]
        uniq, inv = np.unique(_pack(tabs).ravel(), return_inverse=True)
        self.tables = np.stack([(uniq >> sh) & 0xFFFF for sh in (48, 32, 16, 0)], axis=1)
        self.ids = inv.reshape(tabs.shape[:3]).astype(np.int32)
        self.total = self.tables.sum(axis=1)
        self._fisher = self._chi2 = None

    def fisher(self):
        """(p, rtol) per distinct table; where the total is small the rational sum must agree with scipy first"""
        if self._fisher is None:
            p = np.array([fisher_scipy(tuple(int(v) for v in t)) for t in self.tables])
            for t, ps, tot in zip(self.tables, p, self.total):
                if tot <= EXACT_MAX_TOTAL:
                    assert abs(exact_two_sided(*(int(v) for v in t)) - ps) <= 1e-12 * ps, (t, ps)
            self._fisher = p, np.where(self.total > BIG_TOTAL, P_RTOL_BIG, P_RTOL_TIGHT)
        return self._fisher

    def chi2(self):
        """(p, rtol) per distinct table, p = NaN for the tables scipy refuses"""
        if self._chi2 is None:
            self._chi2 = np.array([chi2_scipy(tuple(int(v) for v in t)) for t in self.tables]), \
                np.full(len(self.tables), P_RTOL_TIGHT)
        return self._chi2

    def rows(self, s, reps=1, seed=0, weights=None):
        """-> (incl int32[n, s], excl int64[n, s], pid[n], pi[n, s]): `reps` rows per palette; pi[r, k] is the palette
        entry of sample k.  s = 2: one row per ordered entry pair instead.  s >= 2P: the entries in order and then in
        reverse order at a random place in the row, so that every ordered pair of entries (x, x included) appears."""
        rng = np.random.default_rng(seed * 7919 + s)
        pid, pi = [], []
        for k, nm in enumerate(self.names):
            p = len(PALETTES[nm])
            if s == 2:
                xy = np.stack(np.meshgrid(np.arange(p), np.arange(p), indexing="ij"), axis=-1).reshape(-1, 2)
                pid += [k] * len(xy)
                pi += list(xy)
                continue
            w = None
            if weights is not None and nm in weights:
                w = weights[nm] / weights[nm].sum()
            for _ in range(reps):
                if s >= 2 * p:
                    rest, at = rng.choice(p, s - 2 * p, p=w), rng.integers(0, s - 2 * p + 1)
                    pi.append(np.r_[rest[:at], np.arange(p), np.arange(p)[::-1], rest[at:]])
                else:
                    pi.append(rng.choice(p, s, p=w))
                pid.append(k)
        pid, pi = np.array(pid), np.array(pi)
        pal = np.zeros((len(self.names), self.ids.shape[1], 2), np.int64)
        for k, nm in enumerate(self.names):
            pal[k, :len(PALETTES[nm])] = PALETTES[nm]
        vals = pal[pid[:, None], pi]
        return vals[..., 0].astype(np.int32), vals[..., 1].astype(np.int64), pid, pi

    def pair_ids(self, pid, pi):
        """table id of every pair of every row, int32[n, s(s-1)/2], built one i at a time (vectorised over rows and j:
        no s^2 index arrays at s = 8192)"""
        n, s = pi.shape
        out = np.empty((n, s * (s - 1) // 2), np.int32)
        q = 0
        for i in range(s - 1):
            out[:, q:q + s - 1 - i] = self.ids[pid[:, None], pi[:, i:i + 1], pi[:, i + 1:]]
            q += s - 1 - i
        return out


def assert_p_match(got, ids, want, rtol, what):
    """every element: |got - want| <= rtol * want per table (NaN where want is NaN), in slices so that s = 8192 needs
    no s^2-sized temporaries; returns the number of p-values compared"""
    assert got.shape == ids.shape, (got.shape, ids.shape)
    g, t = got.reshape(-1), ids.reshape(-1)
    step = 1 << 22
    for lo in range(0, g.size, step):
        gs, ts = g[lo:lo + step], t[lo:lo + step]
        w, r = want[ts], rtol[ts]
        nan_w = np.isnan(w)
        ok = np.where(nan_w, np.isnan(gs), np.abs(gs - w) <= r * w)
        if not ok.all():
            bad = lo + np.flatnonzero(~ok)[:5]
            idx = [np.unravel_index(b, got.shape) for b in bad]
            raise AssertionError(f"{what}: {int((~ok).sum())} p-values differ in [{lo}, {lo + gs.size}); first (row, q, "
                                 f"got, want): {[(int(i[0]), int(i[1]), g[b], want[t[b]]) for i, b in zip(idx, bad)]}")
    return g.size


def _check_fisher(ref, got, ids, what):
    p, rtol = ref.fisher()
    return assert_p_match(got, ids, p, rtol, what)


def _check_chi2(ref, got, n_bad, ids, what):
    p, rtol = ref.chi2()
    assert n_bad == int(np.isnan(p)[ids].sum()), (what, n_bad)
    return assert_p_match(got, ids, p, rtol, what)


# ------------------------------------------------------------------------------ CPU doubles of the pair-list tests
class ListEngine:
    """Host stand-in for engine.Context with the pair-list keyword: scipy on every listed table, column q =
    [[incl_i, incl_j], [excl_i, excl_j]] of pair q = (i, j) -- for (j, i) the swapped table, which is what the reference
    would compute on a count table with those two sample columns exchanged."""

    def __init__(self):
        self.calls = []

    def ps(self, counts, row_ptr, col, want_excl=False, want_ps=True):
        ps, excl = O.calculate_psi_vectorised(counts, row_ptr, col)
        return (ps, excl) if want_excl and want_ps else excl if want_excl else ps

    def _pairs(self, s, pairs):
        self.calls.append(None if pairs is None else np.asarray(pairs).tolist())
        return O.pair_list(s) if pairs is None else [(int(i), int(j)) for i, j in np.asarray(pairs)]

    def fisher_pairs(self, incl, excl, pairs=None):
        from scipy.stats import fisher_exact
        incl, excl = np.asarray(incl), np.asarray(excl)
        plist = self._pairs(incl.shape[1], pairs)
        out = np.empty((incl.shape[0], len(plist)))
        for r in range(incl.shape[0]):
            for q, (i, j) in enumerate(plist):
                out[r, q] = fisher_exact([[incl[r, i], incl[r, j]], [excl[r, i], excl[r, j]]])[1]
        return out

    def chi2_pairs(self, incl, excl, pairs=None):
        incl, excl = np.asarray(incl), np.asarray(excl)
        plist = self._pairs(incl.shape[1], pairs)
        out, bad = np.ones((incl.shape[0], len(plist))), 0
        for r in range(incl.shape[0]):
            for q, (i, j) in enumerate(plist):
                try:
                    out[r, q] = O.chi2_yates_restated(incl[r, i], incl[r, j], excl[r, i], excl[r, j])
                except ValueError:
                    bad += 1
        return out, bad

    def bh(self, p):
        return O.bh_fdr(p)

    def bh_columns(self, p):
        return O.bh_columns(p)



def _args(golden_dir, out, mode="none", pairs=None, chi2=False, table="in_inclusionCounts.tsv", filt=None):
    d = os.path.join(golden_dir, "pairwise")
    return argparse.Namespace(inclusionSPLICEDICE=os.path.join(d, table), clusters=os.path.join(d, "in_allClusters.tsv"),
                              chi2=chi2, multiple_test_correction=mode, filter_list=filt, output=str(out), pairs=pairs)


def _pair_file(tmp_path, text, name="pairs.txt"):
    f = tmp_path / name
    f.write_text(text)
    return str(f)


def _quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*a, **k)
    return buf.getvalue()


# ------------------------------------------------------------------------------ recording doubles of the shard classes
class _RecArray:
    """engine.DeviceArray's surface; every call that would reach the device is logged on the engine double"""

    def __init__(self, eng, shape, dtype, ptr, owned):
        self.ctx, self.ptr, self.owned, self.free_calls = eng, ptr, owned, 0
        self.shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def to_host(self, out=None):
        self.ctx.calls.append("to_host")
        return np.zeros(self.shape, self.dtype)

    def memset(self, byte):
        self.ctx.calls.append("memset")
        return self

    def zero(self):
        return self.memset(0)

    def offset(self, lead, shape):
        return _RecArray(self.ctx, shape, self.dtype, self.ptr + lead * self.dtype.itemsize, owned=False)

    def free(self):
        self.free_calls += 1
        if self.owned and self.ptr:                              # (as DeviceArray: a view is never released)
            self.ctx.released.append(self.ptr)
            self.ptr = None


class _RecEngine:
    """the engine.Context methods the shard classes use: allocations hand out tracked arrays, the rest only log"""

    def __init__(self):
        self.calls, self.allocated, self.released, self.next_ptr = [], [], [], 1 << 40
        self.list_ptr = self._address()                          # the context's own list buffer

    def _address(self):
        self.next_ptr += 1 << 40
        return self.next_ptr

    def empty(self, shape, dtype):
        self.calls.append("empty")
        self.allocated.append(_RecArray(self, shape, dtype, self._address(), owned=True))
        return self.allocated[-1]

    def to_device(self, host, dtype=None):
        self.calls.append("to_device")
        host = np.ascontiguousarray(host, dtype=dtype)
        self.allocated.append(_RecArray(self, host.shape, host.dtype, self._address(), owned=True))
        return self.allocated[-1]

    def cluster_dev(self, *arrays, sync=True):
        self.calls.append("cluster_dev")
        self.views.append(_RecArray(self, (0,), np.int32, self.list_ptr, owned=False))
        return self.views[-1], (3 if sync else None)

    views = ()


for _name in ("set_param", "sync", "ps_dev", "ranksum_dev", "fisher_pairs_dev", "chi2_pairs_dev", "bh_columns_dev",
              "bh_columns_pitched_dev", "bh_masked_dev", "copy2d_dev", "comm_fork", "comm_join"):
    setattr(_RecEngine, _name, lambda self, *a, _name=_name, **kw: self.calls.append(_name))


class _IntoComm:
    """RcclComm's surface at world 2: collectives into a buffer the caller owns; the allocating forms allocate"""
    device = True

    def __init__(self, eng, rank, world):
        self.eng, self.rank, self.world = eng, rank, world

    def allgather(self, x):
        return self.eng.empty((self.world * x.shape[0],) + tuple(x.shape[1:]), x.dtype)

    def alltoall(self, x):
        return self.eng.empty(x.shape, x.dtype)

    def allgather_into(self, x, recv):
        self.eng.calls.append("allgather_into")
        return recv

    def alltoall_into(self, x, recv):
        self.eng.calls.append("alltoall_into")
        return recv

    def allsum(self, value):
        return int(value)


# ------------------------------------------------------------------------------ large counts (test_gpu_pair_large_counts)
# Rows of (incl, excl) samples; every ordered pair (i, j), i != j, of a row is a fixture table [[incl_i, incl_j],
# [excl_i, excl_j]].  Expected values: tests/fisher_referee.py.  Every table meets (tests/test_fisher_referee_cpu.py):
#   - nearest >= 1e-9: no ratio r_k != 1 within 1e-9 of 1, so the kernel's tie slack (1e-12), scipy's (1e-14) and the
#     referee's (ties only) select the same terms.  Two samples with EQUAL totals give mathematical ties
#     (pmf(k) = pmf(a + b - k)); two huge totals that differ by little give near-ties, hence the spread of a few per cent;
#   - the step budget: at most LARGE_MAX_STEPS walk steps per table and LARGE_MAX_LANE_STEPS per set of rows, counted
#     by tests/fisher_walk_model.py at the longest trip (24) -- a GPU test runs one set through each entry point once;
#   - the count range of include/sdice.h: total, a d and b c at most 2^53.
LARGE_MAX_STEPS = 2_000_000
LARGE_MAX_LANE_STEPS = 20_000_000
LF_TABLE_DEFAULT = 1 << 20      # fisher.table_max: a total below it reads the log-factorial table
I32_MAX = (1 << 31) - 1
_H = 1 << 19


def _near(x, incl=(1500, 1700, 0, 2000, 37, 1, 640, 1100)):
    """small inclusion counts against exclusion sums within a few per cent of x; samples 0 and 1 share their total (exact
    ties), sample 2 has a = 0 (and, listed second, b = 0: a at either end of its support)"""
    spread = (0, 0, 31, -17, 43, -29, 11, -7)             # in thousandths of x
    out = []
    for k, (a, sp) in enumerate(zip(incl, spread)):
        out.append((a, x + x * sp // 1000 + 13 * k))
    out[1] = (incl[1], out[0][0] + out[0][1] - incl[1])
    return out


LARGE_SETS = {
    # totals of 2^20 - 1, 2^20 and 2^20 + 1 at the default table: sample totals 2^19 (0, 1), 2^19 - 1 (2), 2^19 + 1 (3);
    # the second row stays inside the table
    "boundary": [
        [(104858, _H - 104858), (105500, _H - 105500), (104000, _H - 1 - 104000), (105900, _H + 1 - 105900),
         (40, 190), (0, 77), (2100, 8000), (13, 13)],
        [(104858, _H - 2 - 104858), (105500, _H - 105500), (104000, _H - 1 - 104000), (20000, 80500),
         (40, 190), (0, 77), (2100, 8000), (13, 13)],
    ],
    # balanced tables at counts of 1e5 (inside the table), 3e5 and 1e6 (beyond it): long walks, many rescales, a tail
    # cut that fires late; small columns beside them
    "balanced": [
        [(1_000_000, 4_000_000), (1_003_000, 4_001_000), (300_000, 1_200_000), (301_500, 1_200_700),
         (100_000, 400_000), (100_600, 400_300), (12, 50), (0, 7)],
    ],
    "1e7": [_near(10 ** 7) + [(12, 50), (700, 1300), (1300, 700)]],
    "1e9": [_near(10 ** 9) + [(12, 50), (700, 1300), (1300, 700)]],
    "2^31": [_near((1 << 31) - 1)[:4] + _near((1 << 31) + 1)[4:] + [(12, 50), (700, 1300), (1300, 700)]],
    "1e10": [_near(10 ** 10) + [(12, 50), (700, 1300), (1300, 700)]],
    "2^40": [_near(1 << 40) + [(12, 50), (700, 1300), (1300, 700)]],
    # a d <= 2^53 leaves inclusion counts of 0, 1 and 2 at exclusion sums of 2^52; sample totals of exactly 2^52 twice:
    # a table total of 2^53, the largest accepted
    "2^52": [[(2, (1 << 52) - 2), (1, (1 << 52) - 1), (0, (1 << 51) + (1 << 49)), (2, (1 << 51) + 5), (1, 3), (2, 7), (0, 5),
              (1, 1 << 40), (2, 1 << 45)]],
    # the largest inclusion count against 2^40, beside columns it is balanced with (incl ~ excl / 512) and a d <= 2^53
    "int32": [[(I32_MAX, 1 << 40), (1000, 512_000), (1100, 520_000), (640, 300_000), (2, 1000), (0, 4000),
               (4090, 1 << 21), (5, 2560)]],
}
# the unroll sweep runs on the small-a / huge-d sets only
LARGE_SMALL_A = ("1e7", "1e9", "2^31", "1e10", "2^40", "2^52", "int32")


def large_tables(name):
    """the distinct tables of a set: every ordered pair of every row -> list of (a, b, c, d)"""
    seen = {}
    for row in LARGE_SETS[name]:
        for i, (a, c) in enumerate(row):
            for j, (b, d) in enumerate(row):
                if i != j:
                    seen[(a, b, c, d)] = None
    return list(seen)


def large_arrays(name):
    """(incl int32[n, s], excl int64[n, s]) of a set"""
    rows = np.array(LARGE_SETS[name], dtype=np.int64)
    return rows[..., 0].astype(np.int32), rows[..., 1].copy()


def in_count_range(a, b, c, d, walk=True):
    """the range the host entry points accept (include/sdice.h)"""
    lim = 1 << 53
    return a + b + c + d <= lim and (not walk or (a * d <= lim and b * c <= lim))


def large_pair_list(s):
    """the list of the large-count tests: every pair reversed (i > j), then the last three pairs again, forwards"""
    iu, ju = np.triu_indices(s, 1)
    nat = np.stack([iu, ju], axis=1).astype(np.int32)
    return np.concatenate([nat[:, ::-1], nat[-3:]])


def large_test_tables(name):
    """every table a GPU test walks for a set, call by call: the distinct tables through sdice_fisher_tables, all pairs
    and the list through the host and the _dev entry points"""
    out = large_tables(name)
    for row in LARGE_SETS[name]:
        s = len(row)
        iu, ju = np.triu_indices(s, 1)
        for pairs in (zip(iu, ju), large_pair_list(s)):
            out += 2 * [(row[i][0], row[j][0], row[i][1], row[j][1]) for i, j in pairs]
    return out
