"""Pair sweeps: the Fisher and chi2 pair kernels against a per-table reference on EVERY p-value of every row, at the
sample counts where their hand-out machinery changes shape, under every launch knob, and with more junctions than
resident waves.

The Fisher pair kernel (csrc/fisher.hip) hands pairs out in order through a two-register window of the pair table, keeps
finished walk sums in a 512-slot LDS ring and turns a block of 256 pairs into p-values once the block is complete; the
hand-out may run two blocks ahead of the pmf pass.  What is swept:

- s = 2, 3 (one or three pairs), 23 / 24 (253 / 276 pairs: one block, then the first pair of a second), 33 (528: the
  ring wraps), 46 / 47 (1035 / 1081: the fourth and fifth blocks), 64 / 65, 200, 513 and 8192 (33.5 million pairs in
  one row, the documented limit, 135 168 B of LDS);
- fisher.unroll 4 .. 24 (every template instance), each with and without fisher.count_steps (bit for bit the same
  p-values), times fisher.refill 1, 12, 63 and 64;
- fisher.table_max at a total of T - 1 (the last table entry) and T (device lgamma in the second kernel) in one row,
  flagged and unflagged rows side by side, then back to the default table;
- 20 000 junctions at s = 24 (several junctions per wave, handed out by the counter) into an output filled with NaN
  first, with a guard row behind it that must stay untouched;
- chi2 at the same sample counts, its grid-stride row loop (more rows than n_cu * 32 blocks) and its n_bad count;
- s = 8193 refused by both.

Palette rows make the full check cheap at any s: every sample of a row takes its (incl, excl) from a palette of P
entries, so a row holds at most P^2 distinct tables whatever s is.  The reference (scipy.stats.fisher_exact, which the
reference project calls, and an exact rational sum where the margins are small; scipy chi2_contingency and the restated
Yates p) is computed once per distinct table and scattered to the pair indices q = i*s - i(i+1)/2 + (j-i-1).

The CPU self-checks (not gpu-marked) show that the scatter equals the per-pair oracle element for element, that the
rational sum agrees with scipy, and that every palette reaches what it is there for.
"""
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle_np as O
from splicedice_amd.engine import SdiceError

P_RTOL_TIGHT = 1e-9    # p-values (tests/test_gpu_parity.py)
P_RTOL_BIG = 1e-7      # Fisher tables with a total above 5e4: pmf(a) = exp of nine log-factorials (test_fisher_fuzz_tables)
BIG_TOTAL = 50_000
EXACT_MAX_TOTAL = 400  # the rational sum is used where the total (so every margin) is at most this
gpu = pytest.mark.gpu

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


def _is_tie(t):
    """some k != a of the support has pmf(k) == pmf(a) exactly"""
    a, b, c, d = t
    n1, n2, n = a + b, c + d, a + c
    wa = math.comb(n1, a) * math.comb(n2, n - a)
    return any(math.comb(n1, k) * math.comb(n2, n - k) == wa for k in range(max(0, n - n2), min(n1, n) + 1) if k != a)


def _down_steps(t):
    """the support below a: min(a, d) (the kernel walks k = a - 1 .. lo)"""
    return min(t[0], t[3])


def _up_steps(t):
    """the support above a: min(b, c)"""
    return min(t[1], t[2])


def _margins_nonzero(t):
    a, b, c, d = t
    return a + b > 0 and c + d > 0 and a + c > 0 and b + d > 0


# ------------------------------------------------------------------------------ CPU self-checks of the fixtures
@pytest.mark.parametrize("s", [2, 3, 7, 12])
def test_palette_scatter_is_the_per_pair_oracle(s):
    """the palette-and-scatter reference equals O.fisher_pairs / O.chi2_pairs element for element (same scipy calls,
    so the pair order and the scatter are what is checked)"""
    ref = PaletteRef(PALETTES)
    incl, excl, pid, pi = ref.rows(s, seed=1)
    ids = ref.pair_ids(pid, pi)
    fp, _ = ref.fisher()
    cp, _ = ref.chi2()
    assert np.array_equal(fp[ids], O.fisher_pairs(incl, excl))
    bad = np.isnan(cp[ids])
    good_rows = ~bad.any(axis=1)
    assert bad.any() and good_rows.any()
    assert np.array_equal(cp[ids][good_rows], O.chi2_pairs(incl[good_rows], excl[good_rows]))
    for r in np.flatnonzero(~good_rows):                       # rows where scipy raises: the restated Yates p per pair
        for q, (i, j) in enumerate(O.pair_list(s)):
            try:
                want = O.chi2_yates_restated(incl[r, i], incl[r, j], excl[r, i], excl[r, j])
            except ValueError:
                want = math.nan
            got = cp[ids[r, q]]
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12 * want, (r, q, got, want)


@pytest.mark.parametrize("s", [24, 65, 300])
def test_pair_ids_follow_the_row_major_pair_order(s):
    """the i-at-a-time scatter against np.triu_indices (the pair order of pairwise_fisher.py) at larger s"""
    ref = PaletteRef(SWEEP)
    _, _, pid, pi = ref.rows(s, reps=2, seed=2)
    iu, ju = np.triu_indices(s, 1)
    ids = ref.pair_ids(pid, pi)
    assert np.array_equal(ids, ref.ids[pid[:, None], pi[:, iu], pi[:, ju]])
    for r in range(len(pid)):                                  # every table of the row's palette is in the row
        p = len(PALETTES[ref.names[pid[r]]])
        assert np.array_equal(np.unique(ids[r]), np.unique(ref.ids[pid[r], :p, :p]))


def test_rational_sum_agrees_with_scipy():
    """the exact sum and scipy on every small-total table of the palettes; the restated Yates p and scipy's chi2 too"""
    ref = PaletteRef(PALETTES)
    n = 0
    for t in ref.tables:
        t = tuple(int(v) for v in t)
        c = chi2_scipy(t)
        try:
            r = O.chi2_yates_restated(*t)
        except ValueError:
            r = math.nan
        assert (math.isnan(c) and math.isnan(r)) or abs(c - r) <= 1e-12 * c, (t, c, r)
        if sum(t) <= EXACT_MAX_TOTAL:
            e, s = exact_two_sided(*t), fisher_scipy(t)
            assert abs(e - s) <= 1e-12 * s, (t, e, s)
            n += 1
    assert n > 150


def test_palettes_reach_what_they_claim():
    ref = PaletteRef(PALETTES)
    fp, _ = ref.fisher()
    cp, _ = ref.chi2()

    def of(name):
        k = ref.names.index(name)
        p = len(PALETTES[name])
        i = np.unique(ref.ids[k, :p, :p])
        return [tuple(int(v) for v in t) for t in ref.tables[i]], fp[i], cp[i]

    tabs, p, c = of("zeros")
    assert any(not _margins_nonzero(t) for t in tabs) and (p == 1.0).any() and np.isnan(c).any()
    live = [t for t in tabs if _margins_nonzero(t)]
    assert any(_down_steps(t) == 0 < _up_steps(t) for t in live)               # a == lo: an up-walk only
    assert any(_up_steps(t) == 0 < _down_steps(t) for t in live)               # a == hi: a down-walk only
    assert any(t[0] == t[1] and t[2] == t[3] and c_ == 1.0 for t, c_ in zip(tabs, c))        # observed == expected
    tabs, p, c = of("ties")
    assert sum(_is_tie(t) for t in tabs) >= 8 and (p < 1.0).any()
    tabs, p, c = of("small")
    assert max(sum(t) for t in tabs) <= EXACT_MAX_TOTAL and (p < 1e-70).any()
    assert any(_down_steps(t) == 0 < _up_steps(t) for t in tabs) and any(_up_steps(t) == 0 < _down_steps(t) for t in tabs)
    tabs, p, c = of("thousands")
    assert min(_down_steps(t) + _up_steps(t) for t in tabs) >= 5000 and max(sum(t) for t in tabs) <= BIG_TOTAL
    tabs, p, c = of("big")
    assert min(sum(t) for t in tabs) > BIG_TOTAL
    tabs, p, c = of("tiny")
    assert (p < 1e-250).any() and (p > 1e-3).any() and np.isnan(c).any()
    tabs, p, c = of("edge")
    live = [t for t in tabs if _margins_nonzero(t)]
    assert {TABLE_MAX_T - 2, TABLE_MAX_T - 1, TABLE_MAX_T} <= {sum(t) for t in live}
    assert max(sum(t) for t in tabs) == TABLE_MAX_T
    tabs, p, c = of("under")
    assert max(sum(t) for t in tabs) < TABLE_MAX_T
    tabs, p, c = of("mix")
    assert (p == 1.0).any() and (p < 1e-200).any() and np.isnan(c).any() and any(_is_tie(t) for t in tabs)
    # every Fisher p above scipy's erratic range; chi2 either 0 or a normal number (no subnormal comparisons)
    assert (fp >= 1e-280).all()
    assert np.all(np.isnan(cp) | (cp == 0.0) | (cp >= 1e-300))


# ------------------------------------------------------------------------------ Fisher on the GPU
@gpu
@pytest.mark.parametrize("s", [2, 3, 23, 24, 33, 46, 47, 64, 65, 200, 513])
def test_fisher_pairs_sample_count_sweep(ctx, s):
    ref = PaletteRef(SWEEP)
    reps = 3 if s <= 65 else 1
    incl, excl, pid, pi = ref.rows(s, reps=reps, seed=3, weights={"mix": MIX_WEIGHTS})
    got = ctx.fisher_pairs(incl, excl)
    _check_fisher(ref, got, ref.pair_ids(pid, pi), f"fisher s={s}")


@gpu
def test_fisher_pairs_at_the_sample_limit(ctx):
    """s = 8192: one row, 33 550 336 pairs, 135 168 B of dynamic LDS (inputs as doubles + the 512-slot ring)"""
    ref = PaletteRef(["mix"])
    incl, excl, pid, pi = ref.rows(8192, seed=4, weights={"mix": MIX_WEIGHTS})
    got = ctx.fisher_pairs(incl, excl)
    _check_fisher(ref, got, ref.pair_ids(pid, pi), "fisher s=8192")


@gpu
@pytest.mark.parametrize("s", [24, 65, 200])
def test_fisher_launch_knobs(ctx, s):
    """every unroll instance, counting and plain (bit for bit the same), times four refill thresholds"""
    ref = PaletteRef(SWEEP)
    incl, excl, pid, pi = ref.rows(s, reps=1, seed=5, weights={"mix": MIX_WEIGHTS})
    ids = ref.pair_ids(pid, pi)
    for unroll in (4, 8, 12, 16, 20, 24):
        for refill in (1, 12, 63, 64):
            knobs = {"fisher.unroll": unroll, "fisher.refill": refill}
            with ctx.params({**knobs, "fisher.count_steps": 0}):
                plain = ctx.fisher_pairs(incl, excl)
            with ctx.params({**knobs, "fisher.count_steps": 1}):
                counted = ctx.fisher_pairs(incl, excl)
                useful, issued = ctx.fisher_step_stats()
            what = f"fisher s={s} unroll={unroll} refill={refill}"
            assert np.array_equal(plain.view(np.uint64), counted.view(np.uint64)), what
            assert 0 < useful <= issued and issued % (64 * unroll) == 0, (what, useful, issued)
            _check_fisher(ref, plain, ids, what)


@gpu
def test_fisher_table_max_boundary(ctx):
    """fisher.table_max = T: totals of T - 1 read the last table entry, totals of T leave the pair kernel as markers that
    fisher_beyond_table_kernel completes with lgamma -- both in one row, flagged rows beside unflagged ones; then the
    default table again (the knob rebuilds it) and the same answers"""
    ref = PaletteRef(["edge", "edge", "under", "edge", "under", "zeros"])
    incl, excl, pid, pi = ref.rows(200, reps=8, seed=6)
    ids = ref.pair_ids(pid, pi)
    totals = ref.total[ids]
    assert ((totals == TABLE_MAX_T).any(axis=1).sum() >= 24 and (totals.max(axis=1) < TABLE_MAX_T).sum() >= 16)
    with ctx.params({"fisher.table_max": TABLE_MAX_T}):
        got = ctx.fisher_pairs(incl, excl)
    _check_fisher(ref, got, ids, f"fisher table_max={TABLE_MAX_T}")
    _check_fisher(ref, ctx.fisher_pairs(incl, excl), ids, "fisher table_max restored")


@gpu
def test_fisher_many_junctions_fill_every_slot(ctx):
    """20 000 junctions at s = 24, more than the resident waves (at most n_cu * 32), so waves take junction after
    junction from the counter; the output starts as NaN (0xFF bytes) with one guard row behind it"""
    n, s = 20_000, 24
    assert n > ctx.device_info()["compute_units"] * 32
    ref = PaletteRef(SWEEP)
    reps = -(-n // len(SWEEP))
    incl, excl, pid, pi = ref.rows(s, reps=reps, seed=7, weights={"mix": MIX_WEIGHTS})
    perm = np.random.default_rng(7).permutation(len(pid))[:n]    # palettes interleaved: walk lengths vary wave to wave
    incl, excl, pid, pi = incl[perm], excl[perm], pid[perm], pi[perm]
    n_pairs = s * (s - 1) // 2
    d_incl, d_excl = ctx.to_device(incl), ctx.to_device(excl)
    d_p = ctx.empty((n + 1, n_pairs), np.float64).memset(0xFF)
    ctx.fisher_pairs_dev(d_incl, d_excl, d_p)
    out = d_p.to_host()
    assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
    assert not np.isnan(out[:n]).any(), int(np.isnan(out[:n]).sum())
    _check_fisher(ref, out[:n], ref.pair_ids(pid, pi), "fisher n=20000")


# ------------------------------------------------------------------------------ chi2 on the GPU
@gpu
@pytest.mark.parametrize("s", [2, 3, 23, 24, 33, 46, 47, 64, 65, 200, 513])
def test_chi2_pairs_sample_count_sweep(ctx, s):
    ref = PaletteRef(SWEEP)
    reps = 3 if s <= 65 else 1
    incl, excl, pid, pi = ref.rows(s, reps=reps, seed=8, weights={"mix": MIX_WEIGHTS})
    p, n_bad = ctx.chi2_pairs(incl, excl)
    _check_chi2(ref, p, n_bad, ref.pair_ids(pid, pi), f"chi2 s={s}")


@gpu
def test_chi2_pairs_at_the_sample_limit(ctx):
    """s = 8192: 131 072 B of dynamic LDS, one block walking 33.5 million pairs"""
    ref = PaletteRef(["mix"])
    incl, excl, pid, pi = ref.rows(8192, seed=9, weights={"mix": MIX_WEIGHTS})
    p, n_bad = ctx.chi2_pairs(incl, excl)
    assert n_bad > 0
    _check_chi2(ref, p, n_bad, ref.pair_ids(pid, pi), "chi2 s=8192")


@gpu
def test_chi2_row_loop_and_bad_count(ctx):
    """10 000 rows at s = 12: more rows than the n_cu * 32 blocks of the grid, so blocks loop over rows and each adds
    its bad tables to n_bad once; output pre-filled with 0xFF bytes, a guard row behind it"""
    n, s = 10_000, 12
    assert n > ctx.device_info()["compute_units"] * 32
    ref = PaletteRef(SWEEP)
    incl, excl, pid, pi = ref.rows(s, reps=-(-n // len(SWEEP)), seed=10, weights={"mix": MIX_WEIGHTS})
    incl, excl, pid, pi = incl[:n], excl[:n], pid[:n], pi[:n]
    n_pairs = s * (s - 1) // 2
    d_p = ctx.empty((n + 1, n_pairs), np.float64).memset(0xFF)
    d_bad = ctx.empty(1, np.int64).memset(0xFF)
    ctx.chi2_pairs_dev(ctx.to_device(incl), ctx.to_device(excl), d_p, d_bad)
    out = d_p.to_host()
    assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
    ids = ref.pair_ids(pid, pi)
    n_bad = int(d_bad.to_host()[0])
    assert n_bad > 1000
    _check_chi2(ref, out[:n], n_bad, ids, "chi2 n=10000")
    # the sentinel is a NaN too: the NaNs left must be exactly the bad tables
    assert np.array_equal(np.isnan(out[:n]), np.isnan(ref.chi2()[0])[ids])


@gpu
def test_pair_kernels_refuse_more_than_8192_samples(ctx):
    incl = np.ones((1, 8193), np.int32)
    excl = np.ones((1, 8193), np.int64)
    with pytest.raises(SdiceError, match="8192"):
        ctx.fisher_pairs(incl, excl)
    with pytest.raises(SdiceError, match="8192"):
        ctx.chi2_pairs(incl, excl)
    # the context is still usable
    got = ctx.fisher_pairs(incl[:, :3], excl[:, :3])
    np.testing.assert_allclose(got, [[fisher_scipy((1, 1, 1, 1))] * 3], rtol=P_RTOL_TIGHT, atol=0)
