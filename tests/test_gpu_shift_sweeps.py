"""sdice_shift over more rows than one grid pass of each kernel and at every rows-per-wave choice of the lane-group
kernel: every row of a tiled table is its source row's result, and the source rows are the referee's
(tests/test_gpu_shift.py has the bars).

The lane-group kernel is reached at 6 selected columns (3 v 3); the workgroup kernel takes 65 columns and more, so its
table has 65 (32 v 33), the fewest it can be given."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import shift_fixtures as SF  # noqa: E402
import test_gpu_shift as T  # noqa: E402
from shift_referee import OUTS  # noqa: E402

gpu = pytest.mark.gpu


def _tiled(ctx, n1, n2, n, label):
    """n rows drawn from the 4-per-kind palette of n1 v n2 through both entry points against the palette's own results"""
    ps, g1, g2, _ = SF.table(n1, n2, "mixed", 4)
    first = ctx.shift(ps, g1, g2)
    T.check(first, SF.reference(n1, n2, "mixed", 4), f"palette {n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))
    src = RS.palette_index(n, ps.shape[0])
    big = np.ascontiguousarray(ps[src])
    for entry in ("host", "dev"):
        got = T.call(ctx, entry, big, g1, g2)
        for name in OUTS:
            RS.assert_same_bits(got[name], first[name][src], (label, entry, name), where=lambda r: src[r].tolist())


@gpu
def test_more_rows_than_the_lane_group_kernel_has_waves(ctx):
    """6 columns, one row per chunk: twice as many chunks as the grid has waves, and a ragged tail"""
    cus = ctx.device_info()["compute_units"]
    n = RS.chunk_table_rows(1, cus)
    assert n > 32 * cus
    _tiled(ctx, 3, 3, n, f"{n} rows of 3 v 3")


@gpu
def test_more_rows_than_the_workgroup_kernel_has_workgroups(ctx):
    """65 columns: more rows than the 8 workgroups per compute unit of the launch, so every workgroup takes a second row"""
    cus = ctx.device_info()["compute_units"]
    n = 2 * 8 * cus + 37
    _tiled(ctx, 32, 33, n, f"{n} rows of 32 v 33")


@gpu
@pytest.mark.parametrize("ch", [64, 32, 16, 8, 4, 2, 1])
def test_every_rows_per_wave_choice(ctx, ch):
    """the smallest table that selects each chunk length of the lane-group kernel, plus a ragged tail; 3 v 3 columns (eight
    rows side by side in a wave)"""
    n = RS.chunk_table_rows(ch, ctx.device_info()["compute_units"])
    ps, g1, g2, _ = SF.table(3, 3, "mixed", 4)
    first = ctx.shift(ps, g1, g2)
    src = RS.palette_index(n, ps.shape[0])
    got = ctx.shift(np.ascontiguousarray(ps[src]), g1, g2)
    for name in OUTS:
        RS.assert_same_bits(got[name], first[name][src], (ch, n, name))
