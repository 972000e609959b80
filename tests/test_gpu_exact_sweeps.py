"""sdice_ranksum_exact / sdice_signedrank_exact where only the shape of the call differs: groups wider than the limits
(40 v 40, 4096 columns) whose rows are eligible only where NaNs leave few values, more rows than one launch's grid, and
row slices of 1, 63, 64 and 65 rows.  Bars and tables: tests/test_gpu_exact.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_referee as ER  # noqa: E402
import test_gpu_exact as TE  # noqa: E402

gpu = pytest.mark.gpu

# The grid of a launch (exactrank.hip, ex_plan): at most 8 workgroups per CU, each with as many lane groups (rows) as fit
# 64 KB of LDS and 256 threads.  The 20 v 20 table's largest state is that of 16 v 16, 64 + 17 x 513 words = 35.2 KB: one
# row per workgroup, 8 x CUs rows per pass.  The 34-pair table's is 64 + 993 words (padded to 1088) = 4.3 KB: four groups
# of 64 lanes per workgroup, 32 x CUs rows per pass.
RS_ROWS_PER_CU = 8
SR_ROWS_PER_CU = 32


def wide_table(cols, rows, rng, paired):
    """`rows` rows over two sets of `cols` columns: most keep nearly everything (not eligible), every fourth keeps
    3..16 values a set (paired: the same 3..16 pairs on both sides); 3-decimal values with ties"""
    s = 2 * cols + 1
    ps = (rng.integers(0, 1001, size=(rows, s)) / 1000.0).astype(np.float32)
    ps[rng.random((rows, s)) < 0.03] = np.nan
    g1, g2 = np.arange(0, cols, dtype=np.int32), np.arange(cols + 1, s, dtype=np.int32)
    for r in range(0, rows, 4):
        for g in (g1, g2):
            if g is g1 or not paired:
                gone = rng.permutation(cols)[int(rng.integers(3, 17)):]
            ps[r, g[gone]] = np.nan
    return ps, g1, g2


@gpu
@pytest.mark.parametrize("cols,rows", [(40, 240), (4096, 12)])
@pytest.mark.parametrize("paired", [False, True])
def test_groups_wider_than_the_limit(ctx, paired, cols, rows):
    """test 3 of the issue: such groups are legal, their rows are eligible only where NaNs make them"""
    ps, c1, c2 = wide_table(cols, rows, np.random.default_rng(cols + paired), paired)
    ref = ER.table_reference(ps, c1, c2, paired)
    assert rows // 8 <= ref[0].sum() <= rows // 2
    if paired:
        got, base = ctx.signedrank_exact(ps, c1, c2), ctx.signedrank(ps, c1, c2)
    else:
        got, base = ctx.ranksum_exact(ps, c1, c2), ctx.ranksum(ps, c1, c2)
    assert base["tested"].sum() > ref[0].sum()
    TE.check(got, base, ref, f"{cols} v {cols} paired={paired}")


@functools.lru_cache(maxsize=None)
def repeated(paired, rows):
    """the distinct rows of the table of tests/test_gpu_exact.py repeated to at least `rows` rows, and the reference
    repeated with them"""
    ps, c1, c2, _, _ = TE.sr_table() if paired else TE.rs_table()
    exact, p = TE.sr_reference() if paired else TE.rs_reference()
    times = -(-rows // ps.shape[0])
    big = np.ascontiguousarray(np.tile(ps, (times, 1)))
    big.setflags(write=False)
    return big, c1, c2, (np.tile(exact, times), np.tile(p, times))


@gpu
@pytest.mark.parametrize("paired", [False, True])
def test_more_rows_than_the_grid_and_row_slices(ctx, paired):
    """test 4 of the issue: every row of a table longer than one pass of the grid, and the same table as row slices of
    1, 63, 64 and 65 rows from several offsets"""
    per_pass = ctx.device_info()["compute_units"] * (SR_ROWS_PER_CU if paired else RS_ROWS_PER_CU)
    ps, c1, c2, ref = repeated(paired, per_pass + 700)
    assert ps.shape[0] > per_pass + 600
    exact_call, plain_call = (ctx.signedrank_exact, ctx.signedrank) if paired else (ctx.ranksum_exact, ctx.ranksum)
    got, base = exact_call(ps, c1, c2), plain_call(ps, c1, c2)
    TE.check(got, base, ref, f"{ps.shape[0]} rows over a grid of {per_pass} paired={paired}")
    for length in (1, 63, 64, 65):
        for lo in (0, 101, ps.shape[0] - length):
            part = exact_call(ps[lo: lo + length], c1, c2)
            for name in TE.OUTS:
                assert np.array_equal(TE.bits(part[name]), TE.bits(got[name][lo: lo + length])), (length, lo, name)
