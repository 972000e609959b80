"""sdice_ks where only a sweep decides: the exact p at every kept pair (n1', n2') up to N = 32 and the fall-back at N =
33, through both kernels; more rows than one pass of the grid (a 1 M-row table for each kernel class, every row compared);
every rows-per-wave choice of the lane-group kernel; and a ladder of D from 0 to 1 that takes p from 1 to under the
float64 range.

The bars are those of tests/test_gpu_ks.py (its check()); the 1 % cap on cells under the p floor does not apply to the
ladders, whose purpose is to go there.  A block of 4096 distinct rows is checked against the referee once and tiled; every
output row of the big call must then be, bit for bit, what its source row gave."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_fixtures as KF  # noqa: E402
import rank_support as RS  # noqa: E402
import test_gpu_ks as T  # noqa: E402
from ks_fixtures import OUTS  # noqa: E402

gpu = pytest.mark.gpu


def same_bits(got, want, label):
    for name in OUTS:
        RS.assert_same_bits(got[name], want[name], (label, name))


@gpu
@pytest.mark.parametrize("n1,n2", [(30, 30), (40, 40)])
def test_exact_at_every_kept_pair(ctx, n1, n2):
    """every (n1', n2') with 3 <= n1', n2' and N <= 32, and N = 33 (asymptotic, mark 0), tied and untied: 30 v 30 columns
    through the lane-group kernel, 40 v 40 through the workgroup kernel, NaNs leaving the pair"""
    ps, g1, g2, pairs = KF.pair_table(n1, n2)
    ref = KF.pair_reference(n1, n2)
    out = T.check(ctx.ks(ps, g1, g2, exact=True), ref, f"pairs in {n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))
    assert out["exact"] == 2 * (len(KF.kept_pairs()) - 28) and out["tested"] == ps.shape[0]
    same_bits(T.dev_table(ctx, ps, g1, g2, True), ctx.ks(ps, g1, g2, exact=True), "_dev call")


@gpu
@pytest.mark.parametrize("n1,n2", [(3, 3), (33, 33)])
def test_more_rows_than_one_grid_pass(ctx, n1, n2):
    """1 M rows: the lane-group kernel's waves (3 v 3) and the workgroup kernel's workgroups (33 v 33) stride over the
    rows; every row of the tiled table is its source row's result"""
    rows = 1_000_000
    ps, g1, g2 = KF.block(n1, n2)
    first = ctx.ks(ps, g1, g2, exact=True)
    T.check(first, KF.block_reference(n1, n2), f"block {n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))
    src = np.arange(rows) % KF.BLOCK
    big = np.ascontiguousarray(ps[src])
    got = T.dev_table(ctx, big, g1, g2, True)
    for name in OUTS:
        RS.assert_same_bits(got[name], first[name][src], (n1, n2, name), where=lambda r: (r % KF.BLOCK).tolist())


@gpu
@pytest.mark.parametrize("ch", [64, 32, 16, 8, 4, 2, 1])
def test_every_rows_per_wave_choice(ctx, ch):
    """the smallest table that selects each chunk length of the lane-group kernel, plus a ragged tail; 4 v 5 columns"""
    cus = ctx.device_info()["compute_units"]
    n = RS.chunk_table_rows(ch, cus)
    ps, g1, g2 = KF.block(4, 5)
    first = ctx.ks(ps, g1, g2, exact=True)
    if ch == 64:
        T.check(first, KF.block_reference(4, 5), "block 4 v 5", plain=ctx.ranksum(ps, g1, g2))
    src = RS.palette_index(n, KF.BLOCK)
    got = ctx.ks(np.ascontiguousarray(ps[src]), g1, g2, exact=True)
    for name in OUTS:
        RS.assert_same_bits(got[name], first[name][src], (ch, n, name))


@gpu
@pytest.mark.parametrize("n1,n2,steps", KF.LADDERS)
def test_p_ladder(ctx, n1, n2, steps):
    """D from 0 to 1 at 1024 v 1024 and 4096 v 4096: p from 1 into the region under 1e-280 and to 0, compared under the
    floor rule with no share cap; rows on both sides of the floor and at p = 0"""
    ps, g1, g2 = KF.ladder(n1, n2, steps)
    ref = KF.ladder_reference(n1, n2, steps)
    got = ctx.ks(ps, g1, g2, exact=True)
    out = T.check(got, ref, f"ladder {n1} v {n2}", floor_share=False, plain=ctx.ranksum(ps, g1, g2))
    p = got["p"]
    assert out["below"] >= 3 and (ref["p"] >= RS.P_FLOOR).sum() >= 3 and (p == 0).any() and (ref["p"] == 0).any()
    assert np.all(p[ref["p"] == 0] < 2 * RS.P_FLOOR) and p[0] == 1.0
