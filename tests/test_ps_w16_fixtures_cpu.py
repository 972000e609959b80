"""What ps_w16_fixtures.py says about its tables, asserted without a GPU in integer and rational arithmetic: every named
tile sits on the edge it is named after, and the arithmetic that would be wrong there gives other numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402
import ps_w16_fixtures as WF  # noqa: E402

S = 260


def _designed(fx):
    """every designed cell against the rational oracle"""
    ps, excl, _ = fx.want
    for r, c in fx.designed_cells():
        want_ps, want_excl = PC.fraction_cell(fx.counts, fx.row_ptr, fx.col, r, c)
        assert excl[r, c] == want_excl and PC.same_ps(ps[r, c], want_ps), (r, c)


def test_tiles_are_whole_and_apart():
    for fx in (WF.limits(S), WF.maxima(S), WF.dense(S)):
        assert fx.n % WF.TILE == 0
        for name, r0 in fx.marks.items():
            assert r0 % WF.TILE == 0, name
            # the tile in front of a named tile and the one behind its rows hold small counts only, but for a special row
            if name.startswith(("fan", "star")):
                assert fx.counts[r0 - WF.TILE:r0].max() < 4, name


def test_fans_at_the_packed_sum_limit():
    fx = WF.limits(S)
    deg = np.diff(fx.row_ptr)
    for k, cap in WF.FANS_AT_LIMIT + WF.FANS_PAST_LIMIT:
        r0 = fx.marks[f"fan{k}x{cap}"]
        bound = WF.window_max(fx, r0)
        assert bound == cap and (deg[r0:r0 + k] == k - 1).all() and deg[r0 + k:r0 + WF.TILE].max() == 0
        product = (k - 1 + 1) * bound
        total = int(fx.counts[r0:r0 + k, 0].sum())
        assert total == product == k * cap                      # column 0 reaches the product
        if (k, cap) in WF.FANS_AT_LIMIT:
            assert product == 0xFFFF
            assert (WF.wrapped_total(fx, r0) == fx.counts[r0:r0 + k].sum(0)).all()       # the halves hold every total
        else:
            assert product == 0x10000
            assert WF.wrapped_total(fx, r0)[0] == 0 and total == 1 << 16                 # a half would wrap to 0
            assert bound < 0xFFFF and product < PC.F24                                   # tier 2 is exact
    _designed(fx)


@pytest.mark.parametrize("value", WF.MAXIMA)
def test_window_maxima(value):
    fx = WF.maxima(S)
    deg = np.diff(fx.row_ptr)
    _, excl, _ = fx.want
    for where in WF.WHERE:
        r0 = fx.marks[f"{where}{value}"]
        own_max = int(fx.counts[r0:r0 + WF.TILE].max())
        bound = WF.window_max(fx, r0)
        special = {"own": r0 + 50, "below": r0 - 1, "above": r0 + WF.TILE, "beyond": WF.TILE // 2}[where]
        for i in WF.LISTERS:
            assert fx.col[fx.row_ptr[r0 + i + 1] - 1] == special and deg[r0 + i] in (1, 6), (where, i)
        if where == "beyond":
            assert bound == WF.SMALL and abs(special - r0) > WF.TILE + 32            # no window of the tile holds it
            assert fx.counts[special].max() == PC.I31
        else:
            assert bound == value and (own_max == value) == (where == "own")
            assert fx.counts[special, 0] == value and fx.counts[special, 1] == value - 1
            assert r0 - WF.HALO <= special < r0 + WF.TILE + WF.HALO
        # the sums a saturated window would give differ exactly where a listed count is beyond 0xFFFF
        for i in WF.LISTERS:
            sat = WF.saturated_sums(fx, r0 + i)
            wrong = sat != excl[r0 + i]
            assert wrong.any() == (fx.counts[special].max() > 0xFFFF), (where, i)
            assert (wrong == (fx.counts[special] > 0xFFFF)).all()
    if value == 65534:
        assert all(WF.window_max(fx, fx.marks[f"{w}{value}"]) < 0xFFFF for w in ("own", "below", "above"))
    if value == 65535:
        # the saturated value IS the count: the kernel cannot tell and must not trust it; its sums would still be right
        assert all(WF.window_max(fx, fx.marks[f"{w}{value}"]) == 0xFFFF for w in ("own", "below", "above"))


def test_maxima_cells_in_rational_arithmetic():
    _designed(WF.maxima(S))


def test_dense_loci():
    fx = WF.dense(S)
    deg = np.diff(fx.row_ptr)
    r0 = fx.marks["fan40_small"]
    assert (deg[r0:r0 + 40] == 39).all() and 40 * WF.window_max(fx, r0) <= 0xFFFF
    r0 = fx.marks["fan40_large"]
    assert (deg[r0:r0 + 40] == 39).all() and 0xFFFF < 40 * WF.window_max(fx, r0) < PC.F24 and WF.window_max(fx, r0) < 0xFFFF
    r0 = fx.marks["star300"]
    assert deg[r0] == 300 >= 254 and (deg[r0 + 1:r0 + 301] == 1).all()
    r0 = fx.marks["fan45"]
    assert (deg[r0:r0 + 45] == 44).all() and fx.row_ptr[r0 + WF.TILE] - fx.row_ptr[r0] == 45 * 44 > 16 * WF.TILE
    _designed(fx)
