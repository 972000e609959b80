"""sdice_walsh over more rows than one grid pass of each kernel and at every rows-per-wave choice of the lane-group kernel:
every row of a tiled table is its source row's result, and the source rows are the referee's (tests/test_gpu_walsh.py has
the bars).  The row counts come from the device's compute-unit count.

The lane-group kernel is reached at 3 pairs (eight rows side by side in a wave); the workgroup kernel takes 65 pairs and more,
so its table has 65, the fewest it can be given."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import test_gpu_walsh as T  # noqa: E402
import walsh_fixtures as WF  # noqa: E402
from walsh_referee import OUTS  # noqa: E402

gpu = pytest.mark.gpu


def _tiled(ctx, m, n, label):
    """n rows drawn from the 4-per-kind palette of m pairs through both entry points against the palette's own results"""
    ps, a, b, _ = WF.table(m, "mixed", 4)
    first = ctx.walsh(ps, a, b)
    T.check(first, WF.reference(m, "mixed", 4), f"palette of {m} pairs", plain=ctx.signedrank(ps, a, b))
    src = RS.palette_index(n, ps.shape[0])
    big = np.ascontiguousarray(ps[src])
    for entry in ("host", "dev"):
        got = T.call(ctx, entry, big, a, b)
        for name in OUTS:
            RS.assert_same_bits(got[name], first[name][src], (label, entry, name), where=lambda r: src[r].tolist())


@gpu
def test_more_rows_than_the_lane_group_kernel_has_waves(ctx):
    """3 pairs, one row per chunk: twice as many chunks as the grid has waves, and a ragged tail"""
    cus = ctx.device_info()["compute_units"]
    n = RS.chunk_table_rows(1, cus)
    assert n > 32 * cus
    _tiled(ctx, WF.GROUP_PALETTE, n, f"{n} rows of {WF.GROUP_PALETTE} pairs")


@gpu
def test_more_rows_than_the_workgroup_kernel_has_workgroups(ctx):
    """65 pairs: more rows than the 8 workgroups per compute unit of the launch, so every workgroup takes a second row, a
    grid row after an off-grid one and the other way round"""
    cus = ctx.device_info()["compute_units"]
    n = 2 * 8 * cus + 37
    _tiled(ctx, WF.BLOCK_PALETTE, n, f"{n} rows of {WF.BLOCK_PALETTE} pairs")


@gpu
@pytest.mark.parametrize("ch", [64, 32, 16, 8, 4, 2, 1])
def test_every_rows_per_wave_choice(ctx, ch):
    """the smallest table that selects each chunk length of the lane-group kernel, plus a ragged tail; 3 pairs (eight rows
    side by side in a wave)"""
    n = RS.chunk_table_rows(ch, ctx.device_info()["compute_units"])
    ps, a, b, _ = WF.table(WF.GROUP_PALETTE, "mixed", 4)
    first = ctx.walsh(ps, a, b)
    src = RS.palette_index(n, ps.shape[0])
    got = ctx.walsh(np.ascontiguousarray(ps[src]), a, b)
    for name in OUTS:
        RS.assert_same_bits(got[name], first[name][src], (ch, n, name))
