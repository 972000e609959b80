"""sdice_ranksum_strata where only size or the p tail decides: more rows than one pass of the grid (both kernels, host and
_dev call), row slices at odd offsets, and a ladder of group separations that takes p from 1 to under the float64 range.

The bars are those of tests/test_gpu_strata.py (its check()); the 1 % cap on cells under the p floor does not apply to the
ladders, whose purpose is to go there.  A block of 4096 distinct rows is checked against the referee once and tiled; every
output row of the big call must then be, bit for bit, what its source row gave."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import strata_referee as VR  # noqa: E402
import test_gpu_strata as T  # noqa: E402

gpu = pytest.mark.gpu
BLOCK = 4096


@functools.lru_cache(maxsize=None)
def block(n1, n2, H):
    """BLOCK distinct rows, the kinds of test_gpu_strata cycling -> (ps, g1, g2, strat1, strat2)"""
    rng = np.random.default_rng(99 + n1 + H)
    g1, g2, s1, s2, s = T.draw_lists(rng, n1, n2, H)
    ps = np.stack([T.make_row(rng, r % len(T.KINDS), r // len(T.KINDS), g1, g2, s1, s2, H, s) for r in range(BLOCK)])
    ps.setflags(write=False)
    return ps, g1, g2, s1, s2


@functools.lru_cache(maxsize=None)
def block_reference(n1, n2, H):
    ps, g1, g2, s1, s2 = block(n1, n2, H)
    return VR.table_reference(ps, g1, g2, s1, s2)


def dev_call(ctx, d_ps, lists, H, n):
    """the _dev entry point on a resident table (or a view of it) -> host copies of the outputs"""
    from splicedice_amd.engine import RANKSUM_FIELDS, field_shapes
    held = [ctx.to_device(v, np.int32) for v in lists]
    out = {name: ctx.empty(*sd) for name, sd in field_shapes(RANKSUM_FIELDS, n).items()}
    try:
        ctx.ranksum_strata_dev(d_ps, *held, H, out)
        ctx.sync()
        return {name: a.to_host() for name, a in out.items()}
    finally:
        for a in (*held, *out.values()):
            a.free()


def same_bits(got, want, label):
    for name in T.OUTS:
        RS.assert_same_bits(got[name], want[name], (label, name))


@pytest.mark.parametrize("n1,n2,H", [(4, 4, 2), (40, 40, 3)])
def test_blocks_are_mixed(n1, n2, H):
    ref = block_reference(n1, n2, H)
    t = ref["tested"].astype(bool)
    assert 0.6 * BLOCK < t.sum() < 0.9 * BLOCK and ref["cond"][t].max() <= T.COND_MAX and (ref["p"][t] >= T.P_FLOOR).all()
    assert (ref["grid"][t]).sum() > 1000 and (~ref["grid"][t]).sum() > 1000 and np.unique(ref["z"][t]).size > (60 if n1 == 4 else 1000)


@gpu
@pytest.mark.parametrize("n1,n2,H,rows", [(4, 4, 2, 300_000), (40, 40, 3, 40_000)])
def test_more_rows_than_one_grid_pass(ctx, n1, n2, H, rows):
    """the lane-group kernel's waves and the workgroup kernel's workgroups stride over the rows: every row of the tiled
    table is its source row's result, through the host call and through the _dev call; so are row slices ps[a:b] at odd
    a and b"""
    ps, g1, g2, s1, s2 = block(n1, n2, H)
    first = ctx.ranksum_strata(ps, g1, g2, s1, s2)
    T.check(first, block_reference(n1, n2, H), f"block {n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))
    src = np.arange(rows) % BLOCK
    big = np.ascontiguousarray(ps[src])
    want = {name: first[name][src] for name in T.OUTS}
    same_bits(ctx.ranksum_strata(big, g1, g2, s1, s2), want, "host call")
    d_ps = ctx.to_device(big, np.float32)
    try:
        same_bits(dev_call(ctx, d_ps, (g1, g2, s1, s2), H, rows), want, "_dev call")
        for a, b in ((1, 4099), (4097, rows - 1), (rows - 77, rows)):
            cut = {name: want[name][a:b] for name in T.OUTS}
            same_bits(dev_call(ctx, d_ps.offset(a * big.shape[1], (b - a, big.shape[1])), (g1, g2, s1, s2), H, b - a), cut, f"_dev [{a}:{b}]")
            if b - a < 5000:
                same_bits(ctx.ranksum_strata(big[a:b], g1, g2, s1, s2), cut, f"host [{a}:{b}]")
    finally:
        d_ps.free()


@functools.lru_cache(maxsize=None)
def ladder(n1, n2, H, steps):
    """rows whose group 1 moves from evenly mixed with group 2 to wholly above it: in row t the first round((1/2 + t /
    (2 (steps - 1))) n1) columns of group 1 (dealt to the strata in turn) lie above all columns of group 2 and the rest
    below.  Even rows hold 3-decimal values (heavy ties), odd rows distinct off-grid values."""
    rng = np.random.default_rng(n1 + H)
    s = n1 + n2
    g1, g2 = np.arange(0, s, 2, dtype=np.int32)[:n1], np.arange(1, s, 2, dtype=np.int32)[:n2]
    s1, s2 = (np.arange(n1) % H).astype(np.int32), (np.arange(n2) % H).astype(np.int32)
    ps = np.zeros((steps, s), np.float32)
    for t in range(steps):
        up = int(round((0.5 + t / (2.0 * (steps - 1))) * n1))
        if t % 2 == 0:
            x = np.concatenate([rng.integers(600, 1001, size=up), rng.integers(0, 401, size=n1 - up)]) / 1000.0
            y = rng.integers(401, 600, size=n2) / 1000.0
        else:
            x = np.concatenate([2.0 + rng.permutation(n1)[:up] / 7919.0, -1.0 - rng.permutation(n1)[: n1 - up] / 7919.0])
            y = rng.permutation(9973)[:n2] / 9973.0
        ps[t, g1], ps[t, g2] = x.astype(np.float32), y.astype(np.float32)
    ps.setflags(write=False)
    return ps, g1, g2, s1, s2


@functools.lru_cache(maxsize=None)
def ladder_reference(n1, n2, H, steps):
    ps, g1, g2, s1, s2 = ladder(n1, n2, H, steps)
    return VR.table_reference(ps, g1, g2, s1, s2)


LADDERS = [(4096, 4096, 2, 48), (32, 32, 4, 17)]


@pytest.mark.parametrize("n1,n2,H,steps", LADDERS)
def test_ladders_reach_where_they_should(n1, n2, H, steps):
    ref = ladder_reference(n1, n2, H, steps)
    assert ref["tested"].all() and ref["cond"].max() <= T.COND_MAX and ref["grid"][::2].all() and not ref["grid"][1::2].any()
    assert ref["p"][0] > 0.3 and np.all(np.diff(ref["z"][1::2]) > 0) and np.all(np.diff(ref["z"][::2]) > 0)
    if n1 == 4096:
        p = ref["p"]
        assert (p < T.P_FLOOR).sum() >= 10 and ((p >= T.P_FLOOR) & (p < 1e-100)).sum() >= 3 and (p == 0).any()
        assert ((p > 1e-100) & (p < 1e-3)).sum() >= 3
    else:
        assert 1e-12 < ref["p"][-1] < 1e-9                 # complete separation of 32 v 32: |z| = 6.9 at most


@gpu
@pytest.mark.parametrize("n1,n2,H,steps", LADDERS)
def test_p_ladder(ctx, n1, n2, H, steps):
    """p from 1 into the region under 1e-280 (4096 v 4096) with the bars of check(); the 1 % cap is not for ladders"""
    ps, g1, g2, s1, s2 = ladder(n1, n2, H, steps)
    T.check(ctx.ranksum_strata(ps, g1, g2, s1, s2), ladder_reference(n1, n2, H, steps), f"ladder {n1} v {n2} H={H}",
            floor_share=False, plain=ctx.ranksum(ps, g1, g2))
