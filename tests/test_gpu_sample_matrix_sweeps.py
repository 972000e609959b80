"""sdice_sample_gram sweeps: every column count from 2 to 130 (every partial tile and partial register block), the tile
edges up to 4096 columns, a row ladder across the 4096-row limit of a 32-bit accumulator, every kind of row slice through
the knob gram.rows_per_wg, and a 1 M-row table under the default launch -- the four integer matrices compared for equality,
whole, with tests/sample_matrix_referee.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_matrix_referee as SM  # noqa: E402
from test_gpu_sample_matrix import check  # noqa: E402

gpu = pytest.mark.gpu

MIN_SLICE = 64                      # the smallest row slice the knob gives (smaller values are raised to it)


@gpu
def test_every_column_count_2_to_130(ctx):
    rng = np.random.default_rng(101)
    for m in range(2, 131):
        s = m + 3
        ps = SM.random_table(rng, 97, s)
        cols = rng.permutation(s)[:m].astype(np.int32)
        check(ctx.sample_gram(ps, cols), ps, cols, f"m = {m}")


@gpu
@pytest.mark.parametrize("m", [255, 256, 257, 1023, 1024, 1025, 4095, 4096])
def test_tile_edges(ctx, m):
    rng = np.random.default_rng(103 + m)
    s = m + 3 if m < 4096 else 4099
    ps = SM.random_table(rng, 33, s)
    cols = rng.permutation(s)[:m].astype(np.int32)
    check(ctx.sample_gram(ps, cols), ps, cols, f"m = {m}")


@gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 10_000])
def test_row_ladder(ctx, n):
    """two columns of 1.000 (prod = n * 10^6: past 2^32 from 4295 rows on), one all NaN, one of 0.000, one random"""
    rng = np.random.default_rng(107 + n)
    ps = np.empty((n, 5), np.float32)
    ps[:, 0] = ps[:, 3] = np.float32(1.0)
    ps[:, 1] = np.nan
    ps[:, 2] = np.float32(0.0)
    ps[:, 4] = SM.random_table(rng, n, 1)[:, 0]
    cols = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    got = ctx.sample_gram(ps, cols)
    assert got["prod"][0, 3] == n * 10 ** 6 and got["sum2"][3, 0] == n * 10 ** 6 and got["shared"][0, 3] == n
    check(got, ps, cols, f"n = {n}")
    # the same under slices longer than the accumulators hold: the fold inside a workgroup
    with ctx.params({"gram.rows_per_wg": 16_384}):
        check(ctx.sample_gram(ps, cols), ps, cols, f"n = {n}, one slice")


@gpu
def test_row_slices(ctx):
    """n = 5000, m = 70 (three tile pairs, one off the diagonal) under every kind of slice: the smallest, one that does
    not divide n, 4096, one above n, and the default"""
    rng = np.random.default_rng(109)
    n, s, m = 5000, 75, 70
    ps = SM.random_table(rng, n, s)
    ps[:, 11] = np.float32(1.0)                     # the largest sums there are, in both tiles
    ps[:, 70] = np.float32(1.0)
    cols = np.concatenate([[11], np.setdiff1d(rng.permutation(s), [11, 70])[:m - 2], [70]]).astype(np.int32)
    assert cols.size == m and n % 1024 and n % MIN_SLICE
    want = SM.gram(ps, cols)
    assert want["prod"][0, m - 1] == n * 10 ** 6
    for rows_per_wg in (1, MIN_SLICE, 1000, 4096, 8192, 0):
        with ctx.params({"gram.rows_per_wg": rows_per_wg}):
            got = ctx.sample_gram(ps, cols)
        for name in want:
            assert np.array_equal(got[name], want[name]), (rows_per_wg, name)
    assert ctx.get_param("gram.rows_per_wg") == 0


@gpu
def test_a_million_rows(ctx):
    """1 000 000 x 16 under the default launch: compared in full"""
    rng = np.random.default_rng(113)
    block = SM.random_table(rng, 50_000, 16)
    ps = np.tile(block, (20, 1))
    ps[rng.integers(0, 1_000_000, 5000), rng.integers(0, 16, 5000)] = np.nan      # no two blocks alike
    cols = rng.permutation(16).astype(np.int32)
    check(ctx.sample_gram(ps, cols), ps, cols, "1 M x 16")
