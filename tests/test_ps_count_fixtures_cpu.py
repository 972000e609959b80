"""CPU: the count fixtures of ps_count_fixtures.py are what the GPU tests take them for, and their oracle is the
contract's arithmetic: every designed cell equals its value in rational arithmetic, every cell that is there to show a
wrongly taken 32-bit path differs under 32-bit arithmetic, every named tile sits where it claims on the 2^24 bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

F24 = PC.F24


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    """float32 bit patterns, any NaN equal to any NaN"""
    return PC.same_ps(a, b)


def _fixtures():
    out = [(f"palette{s}", PC.palette(s)) for s in (8, 9, 260)]
    out += [(f"palette_dev{s}", PC.palette_on_device_lists(s)) for s in (8, 9)]
    out += [(f"bound{s}", PC.bound(s)) for s in (8, 9)]
    out += [("large_sums", PC.large_sums()), ("dense_star", PC.dense("star")), ("dense_hb", PC.dense("hb"))]
    return out


@pytest.mark.parametrize("name,fx", _fixtures(), ids=[n for n, _ in _fixtures()])
def test_oracle_equals_rational_arithmetic_on_every_designed_cell(name, fx):
    ps, excl, _ = fx.want
    cells = fx.designed_cells()
    assert len(cells) >= 24
    for r, c in cells:
        want_ps, want_excl = PC.fraction_cell(fx.counts, fx.row_ptr, fx.col, r, c)
        assert excl[r, c] == want_excl, (name, r, c)
        assert _same(ps[r, c], want_ps), (name, r, c)


def test_oracle_np_meets_the_same_condition():
    """oracle_np.calculate_psi_vectorised widens the counts to int64 before it sums and divides in float64: nothing
    passes through float32, and it agrees with the integer oracle wherever it is cheap enough to run"""
    for fx in (PC.palette(9), PC.bound(8), PC.large_sums(), PC.dense("star")):
        ps, excl = O.calculate_psi_vectorised(fx.counts, fx.row_ptr, fx.col)
        assert excl.dtype == np.int64 and np.array_equal(excl, fx.want[1])
        assert _same(ps, fx.want[0])


def test_palette_holds_every_magnitude_and_edge():
    for s in (8, 9, 260):
        fx = PC.palette(s)
        ps, excl, _ = fx.want
        hub = fx.marks["hub"]
        assert np.diff(fx.row_ptr)[hub] == PC.STAR_D and set(np.diff(fx.row_ptr)[hub + 1:hub + 1 + PC.STAR_D]) == {1}
        for v in PC.PALETTE:
            assert (fx.counts[hub + 1:hub + 1 + PC.STAR_D] == v).any(), v
            assert (fx.counts[hub] == v).any() or s < 260, v
        assert fx.counts.max() == PC.I31 and (fx.counts == 0).any() and (fx.counts == 1).any()
        assert np.isnan(ps[:, s - 1]).all() and (ps == 0).any() and (ps == 1).any()
        leaves = ps[hub + 1:hub + 1 + PC.STAR_D, 1]                  # over a hub at 0: 1, or 0 / 0 where the leaf is 0 too
        assert ps[hub, 1] == 0 and ((leaves == 1) | np.isnan(leaves)).all() and (leaves == 1).sum() > 20 and ps[hub, 3] == 1
        assert excl[hub].max() > 2 ** 33
    dev = PC.palette_on_device_lists(8)
    assert np.array_equal(np.diff(dev.row_ptr), np.diff(PC.palette(8).row_ptr))
    assert np.array_equal(dev.want[1], PC.palette(8).want[1])


@pytest.mark.parametrize("s", [8, 9, 260])
def test_bound_tiles_sit_on_either_side_of_2_24(s):
    fx = PC.bound(s)
    R = PC.BOUND_R
    per_tile, per_row = PC.tile_bounds(fx, R, PC.BOUND_HALO)
    assert fx.n % R == 0 and set(fx.marks) == set(PC.BOUND_TILES)
    for name, (product, side) in PC.BOUND_TILES.items():
        r0 = fx.marks[name]
        assert r0 % R == 0 and per_tile[r0] == product, (name, per_tile[r0])
        assert (product < F24) == (side == "fast"), name
    assert {F24 - 1, F24, F24 + 1} <= set(per_tile.values())
    # where the count that decides stands: in an own row, in the row in front of the tile, in the row behind it
    for name in PC.BOUND_TILES:
        r0 = fx.marks[name]
        own, lo, hi = fx.counts[r0:r0 + R].max(), fx.counts[r0 - PC.BOUND_HALO:r0].max(), fx.counts[r0 + R:r0 + R + PC.BOUND_HALO].max()
        if name.startswith(("below", "above")):
            # the count that decides stands in one halo row, which rows of the tile list (and which lists nobody); the own
            # rows alone, at the tile's largest degree, would leave every item fast
            halo_row = r0 - 1 if name.startswith("below") else r0 + R
            if name.startswith("below"):
                assert lo > own and lo > hi and fx.counts[halo_row].max() == lo
            else:
                assert hi > own and hi > lo and fx.counts[halo_row].max() == hi
            assert fx.row_ptr[halo_row + 1] == fx.row_ptr[halo_row]
            listers = [r for r in range(r0, r0 + R) if halo_row in fx.col[fx.row_ptr[r]:fx.row_ptr[r + 1]]]
            assert listers == [r0 + i for i in PC.HALO_LISTERS]
            dmax1 = int(np.diff(fx.row_ptr)[r0:r0 + R].max()) + 1
            assert dmax1 == 17 and dmax1 * int(own) < F24
            assert (dmax1 * int(fx.counts[halo_row].min()) >= F24) == name.endswith("slow")
            tot_l = (fx.want[1] + fx.counts)[listers]
            if name.endswith("slow"):
                assert (tot_l > F24).all() and (tot_l % 2 == 1).all()
                assert sum(1 for r, c in fx.show if r in listers) >= 4 * len(listers)
            else:
                assert (tot_l < F24).all() and per_tile[r0] == F24 - 1
        else:
            assert own > lo and own > hi
    # the far neighbour: outside every window of the tile that lists it, and larger than anything the tile staged
    r0 = fx.marks["outside"]
    row = r0 + 17
    far = int(fx.col[fx.row_ptr[row + 1] - 1])
    assert far < r0 - PC.BOUND_HALO and (fx.counts[far] == PC.I31).all() and fx.counts[r0 - 16:r0 + R + 16].max() == PC.CAP16
    assert fx.want[1][row].min() > PC.I31
    # one tile, both decisions: the rows of the short fan are below the bound, those of the long fan are not
    r0 = fx.marks["per_item"]
    assert (per_row[r0:r0 + 16] < F24).all() and (per_row[r0 + 16:r0 + 33] >= F24).all()
    assert fx.counts[r0:r0 + 33].max() == PC.CAP16
    # totals of exactly 2^24 and 2^24 + 1 exist
    tot = fx.want[1] + fx.counts
    assert (tot == F24).any() and (tot == F24 + 1).any() and (tot == F24 - 1).any()
    # a tile at exactly 2^24 holds no total beyond 2^24: nothing there could show the float32 path
    r0 = fx.marks["own_slow16"]
    assert tot[r0:r0 + R].max() == F24


@pytest.mark.parametrize("s", [8, 9, 260])
def test_show_cells_differ_under_32_bit_arithmetic(s):
    """every cell listed in Fixture.show has an odd total above 2^24, and the float32 sum (the exact total rounded to
    float32, which is what the fast item's 32-bit sum becomes) followed by a float32 division gives other bits than the
    contract: a kernel that takes the 32-bit path there cannot pass.  At least four such cells in every tile that has
    any.  (Sums accumulated in float32 in list order are looked at too: they differ on most of these cells.)"""
    fx = PC.bound(s)
    ps, excl, _ = fx.want
    per_tile, in_order = {}, 0
    for r, c in fx.show:
        tot = int(excl[r, c]) + int(fx.counts[r, c])
        assert tot > F24 and tot % 2 == 1, (r, c, tot)
        a, b = PC.float32_path(fx.counts, fx.row_ptr, fx.col, r, c)
        assert _bits(a) != _bits(ps[r, c]), (r, c)
        in_order += int(_bits(b) != _bits(ps[r, c]))
        per_tile[r // PC.BOUND_R * PC.BOUND_R] = per_tile.get(r // PC.BOUND_R * PC.BOUND_R, 0) + 1
    assert set(per_tile) == {fx.marks[name] for name in PC.SHOW_TILES}
    assert min(per_tile.values()) >= 4 and in_order > len(fx.show) // 2
    # on the fast side the 32-bit path is the contract
    for name, (_, side) in PC.BOUND_TILES.items():
        if side == "fast":
            r0 = fx.marks[name]
            for r in range(r0, r0 + 3):
                for c in range(min(s, 8)):
                    a, _ = PC.float32_path(fx.counts, fx.row_ptr, fx.col, r, c)
                    assert _bits(a) == _bits(ps[r, c]), (name, r, c)


def test_large_sums():
    fx = PC.large_sums()
    ps, excl, q = fx.want
    for d in (600, 3000):
        hub = fx.marks[f"star{d}"]
        assert (excl[hub] == d * PC.I31).all() and (excl[hub + 1:hub + 1 + d] == PC.I31).all()
        assert _bits(ps[hub, 0]) == _bits(np.float32(1.0 / (d + 1)))
    assert excl.max() == 3000 * PC.I31 > 2 ** 40
    z = fx.marks["zeros"]
    assert np.isnan(ps[z:z + 4]).all() and not np.isnan(ps[fx.marks["star600"]:fx.marks["star600"] + 601]).any()
    o = fx.marks["one_zero"]
    assert (ps[o] == 1).all() and (ps[o + 1] == 0).all()
    # ties: PS = k / 2000 from totals of 2000 x 2^20; float32(k / 2000) is not the tie itself, and the '.3f' store goes
    # the way of the float32 value (oracle_np.quantize3 formats the exact binary value)
    t = fx.marks["ties"]
    rows = slice(t, t + 2 * len(PC.TIE_KEYS))
    assert ((excl + fx.counts)[rows] == 2000 * PC.TIE_UNIT).all()
    assert _same(q[rows], O.quantize3(ps[rows]))
    keys = np.rint(q[rows].astype(np.float64) * 1000)
    exact = fx.counts[rows] / PC.TIE_UNIT / 2.0                       # k / 2 = thousandths, always x.5
    assert (np.abs(keys - exact) == 0.5).all() and (keys > exact).any() and (keys < exact).any()


@pytest.mark.parametrize("name", ["star", "hb"])
def test_dense_loci_hold_a_large_count_in_every_row(name):
    fx = PC.dense(name)
    assert (fx.counts.max(1) >= F24).all() and fx.counts.max() == PC.I31
    deg = np.diff(fx.row_ptr)
    if name == "star":
        assert sorted(deg[deg > 1].tolist()) == [252, 253, 254, 255, 256, 300]
    else:
        assert deg.max() == 2 * 257
    # (a count of 2^24 or more in every row, first assertion: whatever the tile shape, its bound is at least 2^24 and
    # no item with a neighbour is fast)
    assert fx.want[1].max() > 2 ** 32                            # exclusion sums that need 64 bits


def test_gene_table_has_a_far_reaching_pair():
    for n, s in ((300, 520), (700, 100)):
        fx = PC.gene_table(n, s)
        rows = np.repeat(np.arange(n), np.diff(fx.row_ptr))
        reach = np.abs(fx.col - rows)
        assert reach.max() == n - 3 and (reach > 64).sum() == 2
        assert np.isnan(fx.want[0]).any() and fx.counts.max() == PC.I31 and fx.want[1].max() >= PC.I31


def test_wide_rows_fixture():
    counts, row_ptr, col, ps, excl, spans = PC.wide(1000)
    want_ps, want_excl = PC.oracle(counts, row_ptr, col)
    assert np.array_equal(excl, want_excl) and _same(ps, want_ps)
    assert spans == [(0, 128), (384, 512), (896, 1000)] and np.isnan(ps[:, 200]).all() and counts.max() >= 2 ** 30
