"""Count sweeps: every kernel that reproduces a float summation order (numpy's pairwise tree for np.mean, a left-to-right
float64 loop, statsmodels' BH quotient) against a plain reference at EVERY count its unrolled plan has to cover, not
only at the counts random NaNs happen to leave.

- rank-sum (compare_sample_sets): group 1 of row i keeps 3 + i values, group 2 keeps G - i, so both groups take every
  count from 3 to G, through each kernel class (lane, wave, counting, block) and every pairwise-sum depth up to six
  levels (depth d first appears at nv = 129, 249, 489, 969, 1929, 3849);
- findOutliers row statistics at every K = 1..1024;
- sdice_excl_f64 / sdice_ps_f64 on list lengths around the 4-wide unroll, on values whose sums depend on the order,
  and past the first grid-stride step;
- BH bit for bit against the restated statsmodels definition on the vector, masked, column and pitched paths.

The CPU self-checks (not gpu-marked) show that the rank-sum fixtures tell numpy's tree from a sequential sum and from a
tree that splits at n/2 without the multiple-of-8 adjustment.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bh_fixtures import bh_columns_values as _bh_columns_values, bh_values as _bh_values  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import PLACEMENTS, _kept_positions, _values, tree_sum  # noqa: E402

P_RTOL_TIGHT = 1e-9    # p-values (tests/test_gpu_parity.py); every other output below is bit-exact
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------ rank-sum fixtures
def sweep_table(n1, n2, flavour, seed=0):
    """-> (ps float32[rows, n1 + n2], g1, g2, nv1, nv2).  Row pair i keeps nv1 = 3 + i % (n1 - 2) values of group 1
    and nv2 = n2 - i % (n2 - 2) of group 2, with two NaN placements per count; one row with nv1 = 2 before the
    nv1 = 3 rows and one with nv2 = 2 after the nv2 = 3 rows (both untested).  g1 and g2 interleave in table
    order: a random split of the columns, each half sorted."""
    rng = np.random.default_rng(seed * 100003 + n1 * 8191 + n2 * 31 + (flavour == "q3"))
    s = n1 + n2
    perm = rng.permutation(s)
    g1, g2 = np.sort(perm[:n1]).astype(np.int32), np.sort(perm[n1:]).astype(np.int32)
    plan = [(2, n2, 0)]
    for i in range(max(n1, n2) - 2):
        a, b = 3 + i % (n1 - 2), n2 - i % (n2 - 2)
        plan += [(a, b, i % 4), (a, b, (i + 2) % 4)]
    plan.append((n1, 2, 1))
    ps = np.full((len(plan), s), np.nan, np.float32)
    for r, (a, b, pl) in enumerate(plan):
        ps[r, g1[_kept_positions(n1, a, PLACEMENTS[pl], rng)]] = _values(rng, a, flavour)
        ps[r, g2[_kept_positions(n2, b, PLACEMENTS[(pl + 1) % 4], rng)]] = _values(rng, b, flavour)
    nv1 = np.array([a for a, _, _ in plan])
    nv2 = np.array([b for _, b, _ in plan])
    return ps, g1, g2, nv1, nv2


# ------------------------------------------------------------------------------ CPU self-checks of the fixtures
@pytest.mark.parametrize("n1,n2", [(8, 8), (64, 64), (1024, 1024), (4096, 4096), (64, 3), (5, 1024), (4096, 5)])
def test_sweep_table_realises_every_count(n1, n2):
    ps, g1, g2, nv1, nv2 = sweep_table(n1, n2, "cont")
    assert np.array_equal(np.sort(np.r_[g1, g2]), np.arange(n1 + n2))
    got1, got2 = (~np.isnan(ps[:, g1])).sum(axis=1), (~np.isnan(ps[:, g2])).sum(axis=1)
    assert np.array_equal(got1, nv1) and np.array_equal(got2, nv2)
    assert set(got1.tolist()) == set(range(2, n1 + 1)) or (n1 == 3 and set(got1.tolist()) == {2, 3})
    assert set(got2.tolist()) == set(range(2, n2 + 1)) or (n2 == 3 and set(got2.tolist()) == {2, 3})
    assert got1[0] == 2 and got2[-1] == 2 and ((got1 < 3) | (got2 < 3)).sum() == 2


@pytest.mark.parametrize("flavour", ["q3", "cont"])
def test_sweep_table_tells_the_tree_apart(flavour):
    """On rows with more than 128 values a sequential float32 sum, and a tree without `n2 -= n2 % 8`, give a mean
    other than np.mean's often enough that a kernel doing either fails the sweep; the restated tree itself is np.sum"""
    ps, g1, g2, nv1, nv2 = sweep_table(4096, 4096, flavour)
    n = seq_diff = tree_diff = 0
    for r in range(ps.shape[0]):
        for g, nv in ((g1, nv1[r]), (g2, nv2[r])):
            if nv <= 128:
                continue
            x = ps[r, g]
            x = x[~np.isnan(x)]
            assert tree_sum(x) == np.sum(x)
            want = np.mean(x)
            n += 1
            seq_diff += np.cumsum(x, dtype=np.float32)[-1] / np.float32(nv) != want
            tree_diff += tree_sum(x, split8=False) / np.float32(nv) != want
    assert n > 2 * 3900
    assert seq_diff >= 0.5 * n, (seq_diff, n)
    assert tree_diff >= 0.1 * n, (tree_diff, n)


# ------------------------------------------------------------------------------ rank-sum sweep on the GPU
def _check_ranksum(got, want):
    assert np.array_equal(got["tested"], want["tested"])
    t = want["tested"].astype(bool)
    for k in ("med1", "med2", "mean1", "mean2", "delta"):
        bad = np.flatnonzero(got[k][t] != want[k][t])
        assert bad.size == 0, (k, bad.size, np.flatnonzero(t)[bad[:5]])       # float32, bit-exact
        assert not got[k][~t].any()
    assert np.array_equal(got["z"][t], want["z"][t])                           # z bit-exact
    np.testing.assert_allclose(got["p"][t], want["p"][t], rtol=P_RTOL_TIGHT, atol=0)


# forced variants (0 auto, 1 lane, 2 block, 3 wave, 4 lane pair, 5 counting + wave) beside auto
FORCED = {17: (1, 4), 64: (1, 4), 129: (3, 5), 1024: (2, 3, 5), 4096: (2,)}


@gpu
@pytest.mark.parametrize("flavour", ["q3", "cont"])
@pytest.mark.parametrize("n1,n2", [(g, g) for g in (8, 16, 17, 63, 64, 65, 128, 129, 1024, 1025, 2048, 4096)]
                         + [(64, 3), (5, 1024), (4096, 5)])
def test_ranksum_count_sweep(ctx, n1, n2, flavour):
    ps, g1, g2, nv1, nv2 = sweep_table(n1, n2, flavour)
    want = O.compare_rows(ps, g1, g2)            # real np.mean / np.median / scipy ranksums, once for every variant
    assert not want["tested"][0] and not want["tested"][-1]
    assert want["tested"][1:-1].all()
    variants = (0,) + (FORCED.get(n1, ()) if n1 == n2 else ())
    for variant in variants:
        with ctx.params({"ranksum.variant": variant}):
            got = ctx.ranksum(ps, g1, g2)
            _check_ranksum(got, want)


@gpu
def test_ranksum_group_limit(ctx):
    from splicedice_amd.engine import SdiceError
    ps = np.random.default_rng(1).random((2, 4100)).astype(np.float32)
    with pytest.raises(SdiceError, match="4096"):
        ctx.ranksum(ps, np.arange(4097), np.arange(4097, 4100))


# ------------------------------------------------------------------------------ findOutliers row statistics
def _rowstats_table(k, dtype, rng):
    """rows with 0, 1, K/2, K-1 and K NaNs among the selected columns (front, back, spread, random), continuous and
    3-decimal values; the columns outside idx hold values that would show if they were read"""
    s = k + 37
    idx = np.sort(rng.choice(s, k, replace=False)).astype(np.int32)
    other = np.setdiff1d(np.arange(s), idx)
    plan = sorted({(c, how) for c in (0, 1, k // 2, k - 1, k) for how in PLACEMENTS})
    data = np.empty((len(plan), s), dtype)
    for r, (n_nan, how) in enumerate(plan):
        vals = rng.random(s) ** 2 if r % 2 else np.round(rng.random(s), 3)
        data[r] = vals.astype(dtype)
        data[r, other] = rng.choice([np.nan, 1e30, -7.0], size=other.size)
        data[r, idx[_kept_positions(k, n_nan, how, rng)]] = np.nan          # here the kept positions are the NaNs
    return data, idx


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rowstats_every_column_count(ctx, dtype):
    """np.nanmean / np.nanstd on each 1-D row (findOutliers.py:130-135 of the reference), bit for bit, K = 1..1024"""
    rng = np.random.default_rng(2024 + (dtype == np.float64))
    for k in range(1, 1025):
        data, idx = _rowstats_table(k, dtype, rng)
        mean, std, n_nan = ctx.rowstats(data, idx)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want_mean = np.array([np.nanmean(r[idx]) for r in data], dtype=dtype)
            want_std = np.array([np.nanstd(r[idx]) for r in data], dtype=dtype)
        assert mean.dtype == dtype and std.dtype == dtype
        assert np.array_equal(n_nan, np.isnan(data[:, idx]).sum(axis=1)), k
        assert np.array_equal(mean, want_mean, equal_nan=True), k
        assert np.array_equal(std, want_std, equal_nan=True), k


# ------------------------------------------------------------------------------ float64 list sums (psf64.hip)
LIST_LENGTHS = tuple(range(10)) + (33,)


def _f64_lists(n_out, n_rows, s, rng):
    """CSR of n_out lists over n_rows rows (rows n_out.. are sources only), lengths cycling through LIST_LENGTHS,
    entries distinct within a list and in random order; a count table whose sums depend on the order of the
    additions: 2^53 next to ones, tenths, thirds, values that add up to within an ulp of an integer"""
    deg = np.array(LIST_LENGTHS)[np.arange(n_out) % len(LIST_LENGTHS)]
    row_ptr = np.r_[0, np.cumsum(deg)].astype(np.int64)
    col = np.concatenate([rng.choice(n_rows, d, replace=False) for d in deg] or [[]]).astype(np.int32)
    pool = np.array([2.0 ** 53, 1.0, 0.1, 0.2, 0.7, 0.3, 1.0 / 3.0, 2.0 / 3.0, 0.05, 1e-3, 2.5, 0.0, 17.125])
    counts = pool[rng.integers(0, pool.size, size=(n_rows, s))]
    frac = rng.random((n_rows, s)) < 0.3
    counts[frac] = np.round(rng.random(frac.sum()) * 50.0, rng.integers(1, 4))
    return counts, row_ptr, col


def _sequential_sums(counts, row_ptr, col, n_out, start=None):
    """left-to-right float64 sums of the listed rows, one IEEE addition per entry (starting from `start` when given)"""
    s = counts.shape[1]
    deg = np.diff(row_ptr[: n_out + 1])
    acc = np.zeros((n_out, s)) if start is None else start.copy()
    first = start is None
    for k in range(int(deg.max(initial=0))):
        r = np.flatnonzero(deg > k)
        v = counts[col[row_ptr[r] + k]]
        if first and k == 0:
            acc[r] = v
        else:
            acc[r] += v
    return acc


@gpu
@pytest.mark.parametrize("s,n_out", [(1, 500), (2, 700), (63, 300), (64, 300), (65, 300), (130, 200), (2, 70_000)])
def test_excl_and_ps_f64_sum_order(ctx, s, n_out):
    """sdice_excl_f64 and sdice_ps_f64 (include/sdice.h): float64 sums of the listed rows left to right in list
    order, bit for bit, for every remainder of the 4-wide unroll and with n_out = 70 000 past the capped grid"""
    rng = np.random.default_rng(s * 1000 + n_out)
    n_rows = n_out + 41
    counts, row_ptr, col = _f64_lists(n_out, n_rows, s, rng)
    excl = ctx.excl_f64(counts, row_ptr, col, n_out=n_out)
    want = _sequential_sums(counts, row_ptr, col, n_out)
    assert excl.shape == (n_out, s)
    assert np.array_equal(excl.view(np.uint64), want.view(np.uint64))
    if s >= 2:                    # np.sum(counts[rows], axis=0) as the reference writes it (a column sum of 2-D rows)
        for r in range(0, n_out, max(1, n_out // 400)):
            rows = col[row_ptr[r]:row_ptr[r + 1]]
            ref = np.sum(counts[rows], axis=0) if rows.size else np.zeros(s)
            assert np.array_equal(excl[r].view(np.uint64), ref.view(np.uint64)), r
    # the fixture can tell the order apart: reversing the lists changes the sums of many rows
    rows = np.repeat(np.arange(n_out), np.diff(row_ptr))
    pos = np.arange(row_ptr[-1])
    col_rev = col[row_ptr[rows] + row_ptr[rows + 1] - 1 - pos]
    assert (_sequential_sums(counts, row_ptr, col_rev, n_out) != want).any(axis=1).mean() > 0.1
    ps = ctx.ps_f64(counts, row_ptr, col, n_out=n_out)
    want_ps = O.write_ps_values_f64(counts, row_ptr, col, n_out)
    with np.errstate(invalid="ignore", divide="ignore"):
        alt = counts[:n_out] / _sequential_sums(counts, row_ptr, col, n_out, start=counts[:n_out].copy())
    assert np.array_equal(want_ps, alt, equal_nan=True)
    assert np.array_equal(ps, want_ps, equal_nan=True)
    assert np.array_equal(np.isnan(ps), np.isnan(want_ps))


@gpu
def test_fractional_tables_truncate_the_table_order_sum(ctx):
    """pairwise on fractional counts (pairwise.fractional_tables): np.sum(counts[rows], axis=0) over each event's rows
    in table order, then np.trunc, as pairwise_fisher.py:158-160 and scipy's int64 cast compute it"""
    from splicedice_amd import pairwise
    rng = np.random.default_rng(58)
    n, s = 900, 5
    deg = np.array(LIST_LENGTHS)[np.arange(n) % len(LIST_LENGTHS)]
    row_ptr = np.r_[0, np.cumsum(deg)].astype(np.int64)
    col = np.concatenate([rng.choice(n, d, replace=False) for d in deg]).astype(np.int32)      # lists unsorted
    pool = np.array([1.0, 0.1, 0.2, 0.7, 0.3, 1.0 / 3.0, 2.0 / 3.0, 0.05, 0.95, 0.0, 2.5, 0.4, 0.6])
    counts = pool[rng.integers(0, pool.size, size=(n, s))]
    frac = rng.random((n, s)) < 0.2
    counts[frac] = np.round(rng.random(frac.sum()) * 20.0, 2)
    incl, excl = pairwise.fractional_tables(ctx, counts, row_ptr, col)
    want_excl = np.zeros((n, s))
    rev_excl = np.zeros((n, s))
    for r in range(n):
        rows = np.sort(col[row_ptr[r]:row_ptr[r + 1]])
        if rows.size:
            want_excl[r] = np.sum(counts[rows], axis=0)
            rev_excl[r] = np.sum(counts[rows[::-1]], axis=0)
    assert (np.trunc(want_excl) != np.trunc(rev_excl)).any()        # the fixture truncates differently by order
    assert incl.dtype == np.int32 and excl.dtype == np.int64
    assert np.array_equal(incl, np.trunc(counts).astype(np.int32))
    assert np.array_equal(excl, np.trunc(want_excl).astype(np.int64))


# ------------------------------------------------------------------------------ BH, bit for bit
@gpu
@pytest.mark.parametrize("m", [1, 2, 257, 16_385, 262_145, 1_000_003, 2_097_153])
def test_bh_vector_paths_bit_exact(ctx, m):
    """bh.vector_path 1 (radix) and 2 (sample sort; 16384 <= m <= 2^21, an error outside), plain and masked, equal
    to the restated statsmodels p_(i) / (i/m) in every bit"""
    from splicedice_amd.engine import SdiceError
    rng = np.random.default_rng(m)
    p = _bh_values(m, rng)
    tested = (rng.random(m) < 0.67).astype(np.uint8)
    want = O.bh_fdr(p)
    want_masked = np.zeros(m)
    want_masked[tested != 0] = O.bh_fdr(p[tested != 0])
    supported = 16384 <= m <= 2 << 20
    for path in (1, 2):
        with ctx.params({"bh.vector_path": path}):
            d_p, d_q = ctx.to_device(p), ctx.empty(m, np.float64)
            d_t, d_neg = ctx.to_device(tested), ctx.to_device(np.where(tested != 0, p, -1.0))
            if path == 2 and not supported:
                with pytest.raises(SdiceError, match="vector_path"):
                    ctx.bh_dev(d_p, d_q)
                with pytest.raises(SdiceError, match="vector_path"):
                    ctx.bh_masked_dev(d_p, d_t, d_q)
                continue
            ctx.bh_dev(d_p, d_q)
            assert np.array_equal(d_q.to_host().view(np.uint64), want.view(np.uint64)), path
            ctx.bh_masked_dev(d_p, d_t, d_q)
            assert np.array_equal(d_q.to_host().view(np.uint64), want_masked.view(np.uint64)), path
            ctx.bh_masked_dev(d_neg, None, d_q)
            assert np.array_equal(d_q.to_host().view(np.uint64), want_masked.view(np.uint64)), path


@gpu
@pytest.mark.parametrize("n", [262_143, 262_144, 262_145])
def test_bh_columns_paths_bit_exact(ctx, n):
    """bh.columns_path 1 (radix) and 2 (sample sort, columns of at most 2^18 values: its reciprocal rank step
    is exact up to there, an error above)"""
    from splicedice_amd.engine import SdiceError
    rng = np.random.default_rng(n)
    p = _bh_columns_values(n, 3, rng)
    want = O.bh_columns(p)
    for path in (1, 2):
        with ctx.params({"bh.columns_path": path}):
            if path == 2 and n > 1 << 18:
                with pytest.raises(SdiceError, match="columns_path"):
                    ctx.bh_columns(p)
                continue
            assert np.array_equal(ctx.bh_columns(p).view(np.uint64), want.view(np.uint64)), path


@gpu
@pytest.mark.parametrize("n,pitch,c0,cols", [(1025, 9, 3, 4), (5000, 37, 5, 20), (70_001, 5, 1, 3)])
def test_bh_columns_pitched_range(ctx, n, pitch, c0, cols):
    """sdice_bh_columns_pitched_dev on columns c0..c0+cols of a row-major [n, pitch] table: the range corrected bit for
    bit, every other column untouched"""
    assert c0 + cols <= pitch
    rng = np.random.default_rng(n + pitch)
    table = _bh_columns_values(n, pitch, rng)
    want = table.copy()
    want[:, c0:c0 + cols] = O.bh_columns(table[:, c0:c0 + cols])
    for path in (1, 2):
        with ctx.params({"bh.columns_path": path}):
            d = ctx.to_device(table)
            ctx.bh_columns_pitched_dev(d.offset(c0, (n * pitch - c0,)), n, cols, pitch)
            assert np.array_equal(d.to_host().view(np.uint64), want.view(np.uint64)), path
