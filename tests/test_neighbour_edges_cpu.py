"""The fixtures of tests/neighbour_edge_fixtures.py hit exactly the edges of neighbours_kernel they are named after
(checked with tests/cluster_referee.py on the host): test_gpu_neighbour_edges.py cannot pass on inputs that miss one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbour_edge_fixtures as F  # noqa: E402
from neighbour_edge_fixtures import T, HB, HF, KMAX, STAGE  # noqa: E402


def _list(name, r):
    row_ptr, col = F.reference(name)
    return col[row_ptr[r]:row_ptr[r + 1]]


def test_every_fixture_is_small_and_in_row_order():
    for name in F.NAMES:
        cr = F.junctions(name)[0]              # (arrays() asserts the row order and that the junctions are distinct)
        assert 1 <= cr.size < 3000, name


@pytest.mark.parametrize("at", [511, 512])
@pytest.mark.parametrize("m,two", [(127, False), (128, False), (129, False), (63, True), (64, True), (65, True)])
def test_forward_fan_runs(at, m, two):
    name = f"ffan-{'two' if two else 'one'}-{at}-{m}"
    f = F.facts(name)
    r = f["fan_row"]
    assert r == at and r % T == (T - 1 if at == 511 else 0)
    cr, left, right, strand = F.junctions(name)
    earlier, later = F.split(name)
    assert later[r] == m and earlier[r] == 0
    lst = _list(name, r)
    assert lst[-1] == f["last_later_row"] == r + (2 * m if two else m)
    assert (strand[lst] == strand[r]).all()
    if two:                                    # the rows in between are of the other strand, one for one
        assert np.array_equal(strand[r:r + 2 * m + 1], np.tile([0, 1], m + 1)[:2 * m + 1])
        assert np.array_equal(lst, r + 2 * np.arange(1, m + 1))
    else:
        assert (strand == 0).all() and np.array_equal(lst, r + np.arange(1, m + 1))
    # a fan at a tile's last row: the window of its tile ends at row r + HF (exclusive r + HF + 1): the run ends one row
    # inside, at the window's last row, one row beyond
    if at == 511:
        window_last = r + HF
        assert lst[-1] - window_last == {127: -1, 128: 0, 129: 1, 63: -2, 64: 0, 65: 2}[m]
    # every row the fan covers lists it as its only earlier neighbour
    assert (earlier[lst] == 1).all()


@pytest.mark.parametrize("chrom", [False, True])
@pytest.mark.parametrize("m", [255, 256, 257])
def test_backward_fan_counts(m, chrom):
    name = f"bfan-chrom-{m}" if chrom else f"bfan-{m}"
    r = F.facts(name)["target_row"]
    assert r == 2 * T and r % T == 0
    cr, left, right, _ = F.junctions(name)
    earlier, later = F.split(name)
    assert earlier[r] == m > KMAX and later[r] == 0
    assert np.array_equal(_list(name, r), r - np.arange(1, m + 1))
    # the window of tile 2 starts at row r - HB: the earliest of the fan is inside it, its first row, one row before it
    assert (r - m) - (r - HB) == {255: 1, 256: 0, 257: -1}[m]
    wlo = r - HB
    maxlen = int((right.astype(np.int64) - left).max())
    exact = cr[r] != cr[wlo] or int(left[wlo]) + maxlen < int(left[r])
    if chrom:
        assert cr[r - m - 1] != cr[r - m] and cr[r - m] == cr[r]
        assert right[r - m - 1] >= left[r - m]    # numerically the last row before the change reaches into the fan
        assert exact == (m == 255)             # the window starts on the chromosome before: the count stays inside it
    else:
        assert (cr == 0).all() and not exact   # the longest junction could reach from before the window


def test_kmax_edge_rows():
    name = "kmax"
    earlier, later = F.split(name)
    cr, left, right, _ = F.junctions(name)
    targets = F.facts(name)["targets"]
    assert sorted(targets) == sorted((b, f) for b in (15, 16, 17) for f in (0, 1, 40))
    maxlen = int((right.astype(np.int64) - left).max())
    tiles = set()
    for (b, f), r in targets.items():
        assert (earlier[r], later[r]) == (b, f), (b, f)
        wlo = max(0, r // T * T - HB)
        assert wlo > 0 and int(left[wlo]) + maxlen < int(left[r])       # `exact`: the count comes from the window
        tiles.add(r // T)
    assert tiles == {1, 2}                     # the cases lie on both sides of a tile's end
    # 16 earlier + 40 later: more than KMAX in all, KMAX earlier ones (kept in LDS); 17 earlier: one too many (redone)
    assert earlier[targets[(16, 40)]] == KMAX and earlier[targets[(17, 0)]] == KMAX + 1
    row_ptr = F.reference(name)[0]
    for t0 in range(0, cr.size, T):
        assert row_ptr[min(t0 + T, cr.size)] - row_ptr[t0] <= STAGE   # every tile is staged


def test_chromosome_changes():
    name = "chrom"
    cr, left, right, strand = F.junctions(name)
    row_ptr, col = F.reference(name)
    changes = (np.flatnonzero(np.diff(cr)) + 1).tolist()
    assert tuple(changes) == F.CHROM_CHANGES == (300, 560, 1100)
    assert 0 < 300 < T and T - HB <= 300 < T                 # inside tile 0, and in the back halo of tile 1
    assert T <= 560 < T + HF                                  # in the front halo of tile 0 (and inside tile 1)
    assert 2 * T <= 1100 < 2 * T + HF                         # in the front halo of tile 1
    for c in changes:
        # numerically the rows on either side overlap: only the chromosome keeps them apart
        a, b = np.arange(c - 20, c), np.arange(c, c + 20)
        hits = 0
        for i in a:
            same = b[strand[b] == strand[i]]
            hits += int(((left[same] <= right[i]) & (right[same] >= left[i])).sum())
        assert hits >= 10
    rows = np.repeat(np.arange(cr.size), np.diff(row_ptr))
    assert (cr[rows] == cr[col]).all() and (strand[rows] == strand[col]).all()
    assert np.diff(row_ptr).max() == 18 and np.array_equal(strand, np.arange(cr.size) % 2)


def test_ties():
    name = "ties"
    nm = F.facts(name)["named"]
    cr, left, right, strand = F.junctions(name)
    assert min(nm.values()) < T <= max(nm.values())            # the group straddles the end of tile 0
    for s in (0, 1):
        A, B, C, D, E, Fj, G = (nm[k, s] for k in "ABCDEFG")
        assert left[A] == left[B] == left[C] and right[A] < right[B] < right[C]
        assert right[A] == left[D] and right[A] == left[E] - 1
        assert right[C] == left[Fj] - 1 and right[Fj] == left[G]
        assert sorted(_list(name, A).tolist()) == sorted([B, C, D])
        assert sorted(_list(name, E).tolist()) == sorted([B, C, D])
        assert sorted(_list(name, C).tolist()) == sorted([A, B, D, E])
        assert _list(name, Fj).tolist() == [G] and _list(name, G).tolist() == [Fj]
        assert (strand[_list(name, C)] == s).all()


def test_dense_tile_total():
    name = "dense"
    row_ptr, col = F.reference(name)
    assert row_ptr.size - 1 == 600 and (np.diff(row_ptr) == 599).all()
    assert row_ptr[T] - row_ptr[0] == T * 599 > STAGE == 11 * 512
    assert row_ptr[600] - row_ptr[T] == 88 * 599 > STAGE
    assert (F.junctions(name)[3] == 0).all()


def test_row_counts():
    sizes = [F.junctions(f"genes-{n}")[0].size for n in (1, 2, 511, 512, 513, 1537)]
    assert sizes == [1, 2, 511, 512, 513, 1537]
    assert np.diff(F.reference("genes-1537")[0]).max() >= 4 and F.reference("genes-1")[1].size == 0
