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
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle_np as O  # noqa: E402
from pair_fixtures import (BIG_TOTAL, EXACT_MAX_TOTAL, MIX_WEIGHTS, P_RTOL_TIGHT, PALETTES, SWEEP, TABLE_MAX_T, PaletteRef,  # noqa: E402
                           _check_chi2, _check_fisher, chi2_scipy, exact_two_sided, fisher_scipy)
from splicedice_amd.engine import SdiceError  # noqa: E402

gpu = pytest.mark.gpu


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
