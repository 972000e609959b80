"""sdice_spearman sweeps: one 1 M-row table past the grid cap of every lane-group kernel (8, 16, 32 and 64 lanes a row;
every row of every output of every call compared), a table with more rows than the workgroup kernel has workgroups,
tables that select fewer rows per wave chunk -- each of them has twice as many
chunks as the capped grid has waves, so the wave-per-row kernel (70 and 130 columns: 2 and 4 a lane) strides too -- and a p ladder from 1 down to 0 at
1024 and 4096 columns with rho of either sign -- against tests/spearman_referee.py under the bars of
tests/test_gpu_spearman.py.

Big tables are a palette (a few hundred distinct rows of every kind) fancy-indexed into n rows, so the referee runs once
per palette row.  Tests without the gpu mark check on the CPU that the tables are what they claim."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spearman_referee as SP  # noqa: E402
from rank_support import NOMINAL_CUS, P_FLOOR, chunk_table_rows, palette_index, rows_per_wave, scatter  # noqa: E402
from test_gpu_spearman import KINDS, OUTS, check, make_row, design, covariate, sorted_design  # noqa: E402

gpu = pytest.mark.gpu

BIG_ROWS = 1_048_576 + 37
BIG_MS = (6, 12, 24, 40)            # one column count per lane-group width: 8, 16, 32, 64 lanes
BIG_S = 44
PALETTE_VARIANTS = 16               # x 12 kinds = 192 palette rows
# (columns, rows per wave chunk): fewer rows in a chunk than groups side by side in a wave (4 < 8 at 8 lanes a row), as
# many, and more; the wave-per-row kernel with 2 and with 4 columns a lane
CHUNK_CASES = ((5, 4), (5, 8), (12, 16), (20, 2), (40, 32), (70, 16), (130, 4), (130, 1))


@functools.lru_cache(maxsize=None)
def palette(m):
    """-> (rows float32[192, max(BIG_S, m + 3)]: every kind 16 times at m listed columns, cols: design(m)'s, which lie
    inside the first m + 3 columns; the other columns hold what would show if one were read)"""
    rng = np.random.default_rng(31000 + m)
    cols, _ = design(m)
    rows = []
    for v in range(PALETTE_VARIANTS):
        for k in range(len(KINDS)):
            row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=max(BIG_S, m + 3))
            row[cols] = make_row(rng, k, v % 6, m)
            rows.append(row)
    return np.stack(rows), cols


@functools.lru_cache(maxsize=None)
def palette_reference(m, which="tied"):
    rows, cols = palette(m)
    return SP.table_reference(rows, *sorted_design(cols, covariate(m, which)))


def test_big_table_is_past_every_grid_cap():
    """for a nominal 256 compute units: 64 rows per wave chunk, more chunks than the capped grid has waves (32 per compute
    unit), a partial last chunk, every palette row in use"""
    assert rows_per_wave(BIG_ROWS, NOMINAL_CUS) == 64 and -(-BIG_ROWS // 64) > 32 * NOMINAL_CUS and BIG_ROWS % 64
    idx = palette_index(BIG_ROWS, PALETTE_VARIANTS * len(KINDS))
    assert np.unique(idx).size == PALETTE_VARIANTS * len(KINDS) and (idx[1:] != idx[:-1]).all()
    assert max(BIG_MS) + 3 <= BIG_S and [8 if m <= 8 else 16 if m <= 16 else 32 if m <= 32 else 64 for m in BIG_MS] == [8, 16, 32, 64]
    ref = palette_reference(12)
    assert 0.6 < ref["tested"].mean() < 0.95 and np.unique(ref["rho"]).size > 60
    quarter = big_table_quarters(BIG_ROWS)
    assert [int((quarter == q).sum()) >= BIG_ROWS // 4 for q in range(4)] == [True] * 4
    assert (quarter[: 64 * 32 * NOMINAL_CUS] < 2).all() and quarter[-1] == 3       # the grid's first pass ends inside quarter 1


@functools.lru_cache(maxsize=None)
def cross_reference(m_rows, m_cols):
    """the palette built for m_rows listed columns under the column list and covariate of m_cols: what the quarter of the
    big table that holds that palette gives in the call with m_cols columns (the listed columns then hold a mix of the
    palette's values and of what its spare columns are filled with: NaN, 1e30, -7, 0.12345)"""
    if m_rows == m_cols:
        return palette_reference(m_cols)
    return SP.table_reference(palette(m_rows)[0], *sorted_design(design(m_cols)[0], covariate(m_cols, "tied")))


def big_table_quarters(n):
    return np.minimum(np.arange(n) * len(BIG_MS) // n, len(BIG_MS) - 1)


def test_big_table_references_cover_every_row():
    """every row of the big table has a reference under each of the four column lists, and the foreign quarters are tables
    worth comparing: most of their rows are tested"""
    for m_cols in BIG_MS:
        for m_rows in BIG_MS:
            ref = cross_reference(m_rows, m_cols)
            assert ref["tested"].shape == (PALETTE_VARIANTS * len(KINDS),)
            if m_rows > m_cols:
                assert ref["tested"].mean() > 0.5, (m_rows, m_cols)


@gpu
def test_spearman_million_rows_every_lane_group(ctx):
    """one resident 1 M-row table, grid-strided by the kernels of 8, 16, 32 and 64 lanes a row (m = 6, 12, 24, 40 of its 44
    columns): EVERY row of every output of every call against the referee -- both passes of the capped grid and the
    partial last chunk, for each kernel.  The rows of the four m-column palettes sit in consecutive quarters of the table;
    a call with m columns meets its own palette in one quarter and the other palettes' rows in the other three."""
    from splicedice_amd.engine import spearman_order
    cus = ctx.device_info()["compute_units"]
    n = BIG_ROWS
    assert rows_per_wave(n, cus) == 64 and -(-n // 64) > 32 * cus and n % 64
    idx = palette_index(n, PALETTE_VARIANTS * len(KINDS))
    quarter = big_table_quarters(n)
    ps = np.empty((n, BIG_S), np.float32)
    for q, m in enumerate(BIG_MS):
        sel = quarter == q
        ps[sel] = palette(m)[0][idx[sel]]
    d_ps = ctx.to_device(ps)
    out = {name: ctx.empty(n, dt) for name, dt in SP.FIELDS}
    try:
        for m in BIG_MS:
            cols, xg = spearman_order(design(m)[0], covariate(m, "tied"))
            d_cols, d_xg = ctx.to_device(cols, np.int32), ctx.to_device(xg, np.int32)
            ctx.spearman_dev(d_ps, d_cols, d_xg, out)
            got = {name: v.to_host() for name, v in out.items()}
            d_cols.free()
            d_xg.free()
            ref = {name: np.empty(n, dt) for name, dt in SP.FIELDS}
            for q, m_rows in enumerate(BIG_MS):
                sel = quarter == q
                for name in ref:
                    ref[name][sel] = cross_reference(m_rows, m)[name][idx[sel]]
            check(got, ref, f"m={m} all {n} rows on {cus} CUs")
    finally:
        for d in (d_ps, *out.values()):
            d.free()


@gpu
@pytest.mark.parametrize("m", (257, 1025))
def test_spearman_workgroup_kernel_strides_over_rows(ctx, m):
    """more rows than the workgroup kernel's capped grid has workgroups (8 per compute unit), one and a half times as many
    and 37: every workgroup takes a second row, some a third, after rows of every kind -- rows with fewer than 3 kept among
    them -- have left their values in its LDS; every row of every output against the referee"""
    from test_gpu_spearman import reference, table
    cus = ctx.device_info()["compute_units"]
    n = 12 * cus + 37
    assert n > 8 * cus
    rows, cols, _ = table(m)
    idx = palette_index(n, rows.shape[0])
    got = ctx.spearman(np.ascontiguousarray(rows[idx]), cols, covariate(m, "tied"))
    check(got, scatter(reference(m, "tied"), idx), f"m={m} n={n} on {cus} CUs")


@gpu
@pytest.mark.parametrize("m,ch", CHUNK_CASES)
def test_spearman_rows_per_wave(ctx, m, ch):
    """ch rows per wave chunk, 64 / P of them side by side: every row of every output against the referee"""
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    assert -(-n // ch) > 32 * cus                       # more chunks than the capped grid has waves
    rows, cols = palette(m)
    idx = palette_index(n, rows.shape[0])
    got = ctx.spearman(np.ascontiguousarray(rows[idx]), cols, covariate(m, "tied"))
    check(got, scatter(palette_reference(m), idx), f"m={m} ch={ch} n={n} on {cus} CUs")


# ------------------------------------------------------------------------------ the p ladder
LADDER_DENSE = 40
P_BANDS = ((1e-3, 1.0 + 1e-9), (1e-20, 1e-3), (1e-100, 1e-20), (1e-200, 1e-100), (1e-280, 1e-200))


def ladder_shuffled(m):
    """how many of the m samples are shuffled at each step: dense from all of them down to 55 %, then 45 %, 35 %, 25 %,
    15 %, 5 %, two samples and none"""
    dense = np.rint(m * (1.0 - 0.45 * (np.arange(LADDER_DENSE) / (LADDER_DENSE - 1)) ** 1.5)).astype(int)
    return dense.tolist() + [round(m * f) for f in (0.45, 0.35, 0.25, 0.15, 0.05)] + [2, 0]


@functools.lru_cache(maxsize=None)
def ladder(m):
    """-> (ps float32[2 * 47, m + 3], cols, x): a PS monotone in the covariate with a growing share of its samples shuffled
    among themselves, every step twice: rising and falling.  The covariate has m / 4 distinct values; steps alternate
    between distinct off-grid values and 3-decimal values (ties from 1001 columns up); the last step is a function of the
    covariate, tied where it ties."""
    rng = np.random.default_rng(5500 + m)
    cols = rng.permutation(m + 3)[:m].astype(np.int32)
    x = np.sort(rng.integers(0, max(2, m // 4), size=m)).astype(np.float64)
    rows = []
    for t, sh in enumerate(ladder_shuffled(m)):
        if t % 2:
            y = (np.rint((np.arange(m) + 0.5) / m * 1000.0) / 1000.0).astype(np.float32)
        else:
            y = ((np.arange(m, dtype=np.float32) + np.float32(1)) / np.float32(m + 2)) * np.float32(1.7) - np.float32(0.3)
        if sh == 0:
            y = ((x + 1.0) / (x.max() + 2.0)).astype(np.float32)          # ties where the covariate ties: |rho| = 1
        pick = rng.choice(m, size=sh, replace=False)
        y[pick] = y[rng.permutation(pick)]
        for v in (y, np.float32(1) - y):          # (a decreasing map: the same ties, rho of the other sign)
            row = np.full(m + 3, np.nan, np.float32)
            row[cols] = v
            rows.append(row)
    return np.stack(rows), cols, x


@functools.lru_cache(maxsize=None)
def ladder_reference(m):
    ps, cols, x = ladder(m)
    return SP.table_reference(ps, cols, x)              # (x is sorted already and the library's sort is stable)


@pytest.mark.parametrize("m", [1024, 4096])
def test_ladder_walks_from_1_to_0(m):
    """by the referee alone: at least three quarters of the ladder rows have p >= 1e-280, p passes through every band and
    ends at 0 (|rho| = 1 exactly on the last, unshuffled step), rho comes in both signs"""
    ref = ladder_reference(m)
    p, rho = ref["p"], ref["rho"]
    assert ref["tested"].all() and (ref["n_kept"] == m).all()
    assert (p >= P_FLOOR).sum() >= 0.75 * p.size, (m, int((p >= P_FLOOR).sum()), p.size)
    for lo, hi in P_BANDS:
        assert ((p >= lo) & (p < hi)).sum() >= 2, (m, lo, hi)
    assert (p < P_FLOOR).sum() >= 4 and p[-2:].tolist() == [0.0, 0.0] and rho[-2:].tolist() == [1.0, -1.0]
    assert (rho[0::2][-8:] > 0).all() and (rho[1::2][-8:] < 0).all() and p[:20].max() > 0.3


@gpu
@pytest.mark.parametrize("m", [1024, 4096])
def test_spearman_p_ladder(ctx, m):
    ps, cols, x = ladder(m)
    got = ctx.spearman(ps, cols, x)
    check(got, ladder_reference(m), f"ladder m={m}")
    assert set(OUTS) == set(got)
