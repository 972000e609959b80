"""Host-side proofs behind test_gpu_large_paths.py (no GPU): the builders of large_path_fixtures.py make what they claim.

1. star_table's closed form (row_of, row_ptr, col) equals oracle_np.cluster_csr (the reference's loop) whole, and
   cluster_referee.row_order / row_ptr, at a few thousand rows with the scan block scaled down to 64: the same code
   with the same rules then states the expected value at 8.4 M rows, where neither referee is affordable.
2. The layout at the real sizes (the piece list alone, no rows built) puts the stars where the GPU tests need them.
3. junction_keys, bh_pvalues, digit_mask_keys, quantize_values and low_indices have the structure their tests rely on.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_referee as CR  # noqa: E402
import large_path_fixtures as LP  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

B_SMALL = 64
SMALL_BOUNDS = (20 * B_SMALL, 40 * B_SMALL)
SMALL_SIZES = [40 * B_SMALL, 40 * B_SMALL + 1, 40 * B_SMALL + 2 * B_SMALL + 5]      # the shapes of N0, N0 + 1, N0 + 2 B + 5


@pytest.mark.parametrize("n", [1, 2, 7, 2693, 8_388_608, 8_388_609, 8_392_709, 3_000_000])
def test_shuffle_is_a_permutation(n):
    src = LP.shuffle_index(n)
    assert src.min() == 0 and src.max() == n - 1 and np.all(np.bincount(src, minlength=n) == 1)
    if n > 100:
        assert np.abs(np.diff(src[:50])).min() > n // 4      # neighbours of the input are far apart in the order


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_star_table_equals_oracle_and_referee(n):
    t = LP.star_table(n, B_SMALL, SMALL_BOUNDS)
    a = LP.star_input(t)
    want_row_of, want_row_ptr, want_col = O.cluster_csr(*a)
    assert np.array_equal(t.row_of, want_row_of)
    assert np.array_equal(t.row_ptr, want_row_ptr)
    assert np.array_equal(t.col, want_col)
    assert np.array_equal(CR.row_order(*a), t.row_of)
    assert np.array_equal(CR.row_ptr(*a), t.row_ptr)
    assert t.row_of.dtype == np.int32 and t.row_ptr.dtype == np.int64 and t.col.dtype == np.int32


def _check_layout(n, B, bounds, pieces):
    """what the GPU tests need from the layout, from the piece list alone"""
    assert pieces[0][1] == 0 and all(p[1] + p[2] == q[1] for p, q in zip(pieces, pieces[1:]))
    assert pieces[-1][1] + pieces[-1][2] == n and all(p[2] >= 1 for p in pieces)
    stars = [(i, p) for i, p in enumerate(pieces) if p[0] == "star"]
    assert sum(p[3] for p in pieces) >= 5                                     # several chromosomes
    reach = [(s + 1, s + k) for _, (_, s, k, _) in stars]                     # rows whose prefix maximum is the star's right
    for lo, hi in reach:
        assert hi - lo > 3 * B - 16 and lo // B + 2 <= (hi - 1) // B          # across at least two block boundaries
    for bnd in bounds:
        if bnd + B < n:
            assert any(lo < bnd - B // 2 and bnd + B // 2 < hi for lo, hi in reach), bnd
    # the last star runs up to the last two rows of the table (into the partial scan block when n % B > 2), which are
    # another chromosome
    i, (_, s, k, _) = stars[-1]
    assert s + k == n - 2 and pieces[i + 1][3] and pieces[i + 1][2] == 2 and i + 2 == len(pieces)
    # every boundary star's tail block also holds the start of the next chromosome; the first star's does not
    for i, (_, s, k, _) in stars[1:]:
        assert pieces[i + 1][3] and pieces[i + 1][1] // B == (s + k - 1) // B
    assert not pieces[stars[0][0] + 1][3]


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_star_layout_small(n):
    t = LP.star_table(n, B_SMALL, SMALL_BOUNDS)
    _check_layout(n, B_SMALL, SMALL_BOUNDS, t.pieces)
    # lefts restart below the right end of the star that ended the chromosome before: a maximum that leaked across
    # the segment boundary would add neighbours
    order = np.argsort(t.row_of)
    cr, left, right = t.cr[order], t.left[order], t.right[order]
    for (kind, s, k, _), nxt in zip(t.pieces, t.pieces[1:]):
        if kind == "star" and nxt[3]:
            assert cr[nxt[1]] == cr[s] + 1 and left[nxt[1]:nxt[1] + nxt[2]].max() < right[s]
    assert np.array_equal(t.strand, t.cr & 1) and t.n_chrom == cr[-1] + 1


@pytest.mark.parametrize("n", LP.LARGE_SIZES)
def test_star_layout_at_the_real_sizes(n):
    pieces = LP.star_pieces(n)
    _check_layout(n, LP.SCAN_BLOCK, (LP.MID, LP.TOP), pieces)
    stars = [p for p in pieces if p[0] == "star"]
    assert len(stars) == 3                                                    # early, across MID, the last one
    if n > LP.N0 + LP.SCAN_BLOCK:
        assert stars[-1][1] < LP.TOP - LP.SCAN_BLOCK // 2 and stars[-1][1] + stars[-1][2] > LP.TOP + LP.SCAN_BLOCK


def test_fast_path_limit_fills_every_bucket():
    """at exactly N0 junctions the sort stage of the fast clustering plans all 4096 buckets, every one of them holds
    keys and none exceeds its slot: the default run of the GPU test stays on the fast path"""
    t = LP.star_table(LP.N0)
    plan = CR.sort_plan(t.cr, t.left, t.right)
    assert plan.B == LP.MAX_BUCKETS == CR.MAX_BUCKETS and (plan.count > 0).all()
    assert not plan.overflow and plan.count.max() <= plan.slot_cap // 2
    assert CR.sort_plan(t.cr[:9], t.left[:9], t.right[:9]).B == 1 and LP.N0 == CR.MAX_BUCKETS * CR.BUCKET_MEAN


def _check_keys(n, B, bounds, pair_at, keys, s):
    assert np.all(s[1:] >= s[:-1])
    flag = np.r_[1, (s[1:] != s[:-1]).astype(np.int64)]
    runs = LP.zero_runs(n, B, bounds)
    assert len(runs) == sum(b - 3 * B - 77 > 0 and b - 3 * B - 77 < n - 3 * B for b in bounds) >= 1
    for lo, hi in runs:
        assert hi - lo > 3 * B and flag[lo] == 1 and not flag[lo + 1:hi].any() and (hi == n or flag[hi] == 1)
        blocks = flag[: n // B * B].reshape(-1, B).sum(axis=1)
        assert (blocks[lo // B + 1:(hi - B + 1) // B] == 0).all() and (hi - B + 1) // B - (lo // B + 1) >= 2
    for bnd in bounds:                                                        # a run lies across every boundary the input reaches
        if bnd + 1 <= n - 1:
            assert any(lo < bnd - B and bnd < hi for lo, hi in runs)
    assert pair_at % B == 0 and flag[pair_at - 1:pair_at + 2].tolist() == [1, 0, 1]
    assert flag[n // 4:n // 4 + 2 * B].all()                                  # a stretch of distinct keys
    mixed = flag[n // 8:n // 4]
    assert 0.4 < mixed.mean() < 0.6
    # the key layout: chrom 12 | left 31 | span 20 | strand 1
    assert int(s.max() >> np.uint64(52)) < 32 and int(((s >> np.uint64(1)) & np.uint64(0xFFFFF)).max()) < 2 ** 11
    assert LP.varying_bits(keys) & 1


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_junction_keys_small(n):
    keys, s = LP.junction_keys(n, B=B_SMALL, bounds=SMALL_BOUNDS, pair_at=30 * B_SMALL)
    assert np.array_equal(np.sort(keys), s)
    _check_keys(n, B_SMALL, SMALL_BOUNDS, 30 * B_SMALL, keys, s)


def test_junction_keys_at_the_largest_size():
    n = LP.LARGE_SIZES[-1]
    keys, s = LP.junction_keys(n)
    _check_keys(n, LP.SCAN_BLOCK, (LP.MID, LP.TOP), 1500 * LP.SCAN_BLOCK, keys, s)
    assert len(LP.zero_runs(n)) == 2 and len(LP.zero_runs(LP.N0)) == 2 and LP.zero_runs(LP.N0)[1][1] == LP.N0
    # real junction keys: chromosome ranks below 32 leave the top seven bits constant
    assert (LP.varying_bits(keys) >> 57) == 0


def _check_p(m, B, bounds, p, ps):
    assert np.all(np.diff(ps) >= 0)
    assert ps[:2].tolist() == [0.0, 5e-324] and ps[2] == 1e-300
    assert abs((p == 1.0).mean() - 0.3) < 1e-3
    rev = ps[::-1]
    raw_rev = rev * m / np.arange(m, 0, -1)
    for lo, hi in LP.bh_tie_runs(m, B, bounds):
        assert hi - lo > 3 * B and np.all(rev[lo:hi] == rev[lo]) and rev[lo - 1] != rev[lo] and rev[hi] != rev[lo]
        assert np.all(np.diff(raw_rev[lo:hi]) > 0)                            # the minimum of the run is its first entry
        assert (hi - 1) // B - lo // B >= 3
    (lo, hi), (lo2, hi2) = LP.bh_tie_runs(m, B, bounds)
    assert lo < bounds[0] - B and bounds[0] + B < hi and lo2 < bounds[1] - B
    assert hi2 == m - 2 and (m <= bounds[1] + B or hi2 > bounds[1] + B)
    d = np.diff(ps[2 + (hi2 - lo2):m - int(0.3 * m)])
    close = (d > 0) & (d < 1e-14)
    assert close.sum() > 5                                                    # distinct values a few ulps apart


@pytest.mark.parametrize("m", SMALL_SIZES)
def test_bh_pvalues_small(m):
    p, ps = LP.bh_pvalues(m, B=B_SMALL, bounds=SMALL_BOUNDS)
    assert np.array_equal(np.sort(p), ps)
    _check_p(m, B_SMALL, SMALL_BOUNDS, p, ps)


def test_bh_pvalues_at_the_largest_size():
    m = LP.LARGE_SIZES[-1]
    p, ps = LP.bh_pvalues(m)
    _check_p(m, LP.SCAN_BLOCK, (LP.MID, LP.TOP), p, ps)


def test_digit_mask_keys():
    for name, mask, const in LP.MASK_SHAPES:
        for n in LP.MASK_SIZES:
            keys = LP.digit_mask_keys(n, mask, const)
            assert keys.size == n and LP.varying_bits(keys) == (mask if n > 1 else 0), (name, n)
            assert int(keys[0]) & const == const
    digits = {name: {d for d in range(8) if (mask >> (8 * d)) & 0xFF} for name, mask, _ in LP.MASK_SHAPES}
    assert [digits[f"digit_{d}"] for d in range(8)] == [{d} for d in range(8)]
    assert digits["digits_0_7"] == {0, 7} and digits["digits_0_2_5"] == {0, 2, 5} and digits["digits_1_3_4_6"] == {1, 3, 4, 6}
    assert digits["all_digits"] == set(range(8)) and digits["ff_between"] == {2, 4}
    assert bin(dict((s[0], s[1]) for s in LP.MASK_SHAPES)["one_bit"]).count("1") == 1
    assert (int(LP.digit_mask_keys(9, *LP.MASK_SHAPES[-1][1:])[3]) >> 24) & 0xFF == 0xFF


def test_quantize_values_and_low_indices():
    for n in (LP.QUANTIZE_GRID, LP.QUANTIZE_GRID + 1, 2 * LP.QUANTIZE_GRID + 3):
        v = LP.quantize_values(n)
        assert v.dtype == np.float32 and v.size == n and np.isnan(v).any() and (v == 0).any() and (v == 1).any()
        # the tail holds '.3f' ties, which only the round-half-even of the exact product decides
        assert v[-3:].tolist() == np.float32([0.9985, 0.9995, 0.0005]).tolist()
        assert np.array_equal(O.quantize3_fast(v[-3:]), O.quantize3(v[-3:]))
    for n_low in (LP.MARK_LOW_GRID, LP.MARK_LOW_GRID + 1, 1_300_003):
        idx = LP.low_indices(n_low, 3_000_000)
        assert idx.dtype == np.int64 and idx.size == n_low and idx.min() == 0 and idx.max() == 2_999_999
        assert np.unique(idx).size < n_low and (idx == idx[-1]).sum() == 1
