"""The branches of the shared primitives that only an input size selects, at the sizes production reaches:

  scan.hip      the three-launch scan (scan_sums_kernel + scan_apply_kernel) beyond 4096 blocks of 2048, for all three
                operators: the prefix sum of the junction union and of row_ptr, the prefix maximum of the generic
                clustering, the running minimum of BH on the radix path -- and the two-launch scan at exactly 4096 blocks
  cluster       the hand-over of sdice_cluster_dev to the generic chain above 8 388 608 junctions, and the fast path at
                exactly 8 388 608 with all 4096 buckets
  radix.hip     digit skipping with gaps and odd / even pass counts; the switch between the two bin-scan kernels
  bh.hip        the second row chunk of the pitched transpose; the column groups of a table that does not fit at once
  ps.hip        the grid-stride passes of quantize3_kernel and mark_low_kernel

Every expected value comes from numpy, oracle_np or the closed form of large_path_fixtures.star_table (proved against the
oracle and the cluster referee in test_large_path_fixtures_cpu.py); comparisons are integer or bit equality, except BH
against the oracle at rtol 1e-14.  Wherever a case names a path, the launch counts of the context profile prove that it
ran and that the other one did not.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_path_fixtures as LP  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd.engine import SdiceError  # noqa: E402

pytestmark = pytest.mark.gpu

B, N0 = LP.SCAN_BLOCK, LP.N0
ABOVE = N0 + 2 * B + 5
KERNELS = ("scan_reduce_kernel", "scan_apply_self_kernel", "scan_sums_kernel", "scan_apply_kernel",
           "radix_hist_kernel", "radix_binscan_small_kernel", "radix_binscan_kernel", "transpose_f64_kernel",
           "bucket_sort_kernel", "bh_keys_kernel", "bhs_finish_kernel")


@contextlib.contextmanager
def _launches(ctx):
    """`with _launches(ctx) as c:` -> c[kernel] = launches inside the block (filled when it ends)"""
    c = {}
    ctx.prof_enable(1)
    ctx.prof_reset()
    try:
        yield c
    finally:
        rep = ctx.prof_report()
        ctx.prof_enable(0)
        c.update({k: rep.get(k, (0, 0.0))[0] for k in KERNELS})


def _scans(c):
    """(two-launch scans, three-launch scans) among the launches"""
    assert c["scan_sums_kernel"] == c["scan_apply_kernel"]
    assert c["scan_reduce_kernel"] == c["scan_apply_self_kernel"] + c["scan_sums_kernel"]
    return c["scan_apply_self_kernel"], c["scan_sums_kernel"]


def _scan_path(n):
    """what one scan over n elements must launch"""
    return (1, 0) if -(-n // B) <= LP.SCAN_SELF_MAX else (0, 1)


def test_the_sizes_sit_on_the_switch():
    assert _scan_path(N0) == (1, 0) and _scan_path(N0 + 1) == (0, 1) and LP.LARGE_SIZES == (N0, N0 + 1, ABOVE)
    assert N0 == LP.MAX_BUCKETS * 2048 and N0 > LP.BH_VECTOR_SAMPLESORT_MAX


# ---------------------------------------------------------------------------------------------- prefix sum with total
@pytest.mark.parametrize("n", LP.LARGE_SIZES)
def test_sort_unique_scan_paths(ctx, n):
    """the junction union at 4096 full scan blocks (two launches), with one key in block 4096 and with a partial block
    4098 (three): flags with whole blocks of zeros across the iteration boundaries of scan_sums_kernel, all-ones
    stretches and a duplicate pair across a block boundary"""
    keys, _ = LP.junction_keys(n)
    want = np.unique(keys)
    digits = sum(1 for d in range(8) if (LP.varying_bits(keys) >> (8 * d)) & 0xFF)
    try:
        with _launches(ctx) as c:
            got = ctx.sort_unique_u64(keys)
        assert got.size == want.size
        assert np.array_equal(got, want)
        assert _scans(c) == _scan_path(n)
        assert c["radix_binscan_kernel"] == digits and c["radix_binscan_small_kernel"] == 0
    finally:
        ctx.trim()


# ---------------------------------------------------------------------------------------------- radix digit masks
@pytest.mark.parametrize("rounds", [12, 4])
def test_radix_digit_masks(ctx, rounds):
    """every shape of the varying-bit mask at the wave-quarter and tile edges of both tile sizes and at 256 | 257 tiles
    (the loop of radix_binscan_kernel): one pass per varying digit, the last one into the output buffer"""
    with ctx.params({"sort.rounds": rounds}):
        for name, mask, const in LP.MASK_SHAPES:
            digits = sum(1 for d in range(8) if (mask >> (8 * d)) & 0xFF)
            pool = LP.digit_mask_keys(LP.MASK_SIZES[-1], mask, const)
            for n in LP.MASK_SIZES:
                keys = pool[:n]
                assert LP.varying_bits(keys) == (mask if n > 1 else 0), (name, n)
                with _launches(ctx) as c:
                    got = ctx.sort_unique_u64(keys)
                assert np.array_equal(got, np.unique(keys)), (name, n, rounds)
                assert c["radix_hist_kernel"] == (digits if n > 1 else 0), (name, n, rounds)
                assert c["radix_binscan_kernel"] + c["radix_binscan_small_kernel"] == c["radix_hist_kernel"]
    assert -(-LP.MASK_SIZES[-1] // LP.RADIX_TILE[12]) == 257 and LP.MASK_SIZES[-2] // LP.RADIX_TILE[12] == 256


# ---------------------------------------------------------------------------------------------- generic clustering
_stars = {}


def _star(n):
    if n not in _stars:
        _stars[n] = LP.star_table(n)
    return _stars[n]


def _same_lists(got, t, what):
    assert np.array_equal(got[0], t.row_of), (what, "row_of")
    assert np.array_equal(got[1], t.row_ptr), (what, "row_ptr")
    assert got[2].size == t.col.size and np.array_equal(got[2], t.col), (what, "col")


@pytest.mark.parametrize("knob", [None, "cluster.generic", "cluster.legacy"])
def test_cluster_above_the_fast_path_limit(ctx, knob):
    """8 388 608 + 2 * 2048 + 5 junctions: sdice_cluster_dev hands over to the generic chain by itself; the two-sort
    chain and the chain by knob give the same.  The prefix maximum over n and the prefix sum over n + 1 both take three
    launches; stars put the maximum of one row onto rows several scan blocks further on, across the blocks 2047 | 2048
    and 4095 | 4096 and into the last, partial one, and chromosomes end inside a star's last block."""
    t = _star(ABOVE)
    try:
        with ctx.params({knob: 1} if knob else {}):
            with _launches(ctx) as c:
                got = ctx.cluster(*LP.star_input(t))
        _same_lists(got, t, knob)
        assert _scans(c) == (0, 2)
        assert c["bucket_sort_kernel"] == 0 and c["radix_binscan_kernel"] >= 1 and c["radix_binscan_small_kernel"] == 0
    finally:
        ctx.trim()


def test_cluster_at_the_fast_path_limit(ctx):
    """exactly 8 388 608 junctions: the largest table of the fast path, all 4096 buckets in use, no fallback; the generic
    chain by knob scans its maxima over N0 with two launches and its degrees over N0 + 1 with three"""
    t = _star(N0)
    a = LP.star_input(t)
    try:
        d = [ctx.to_device(x) for x in a]
        d_row_of, d_row_ptr = ctx.empty(N0, np.int32), ctx.empty(N0 + 1, np.int64)
        with _launches(ctx) as c:
            d_col, _ = ctx.cluster_dev(*d, d_row_of, d_row_ptr, sync=False)
            nnz, _ = ctx.cluster_status()            # raises if a bucket overflowed or the look-back gave up
        assert c["bucket_sort_kernel"] == 1 and c["radix_hist_kernel"] == 0 and _scans(c) == (0, 0)
        fast = (d_row_of.to_host(), d_row_ptr.to_host(), d_col.offset(0, (nnz,)).to_host())
        _same_lists(fast, t, "fast path")
        del d, d_row_of, d_row_ptr
        with ctx.params({"cluster.legacy": 1}):
            with _launches(ctx) as c:
                legacy = ctx.cluster(*a)
        assert c["bucket_sort_kernel"] == 0
        assert _scans(c) == (1, 1)                   # max over N0: two launches; sum over N0 + 1: three
        _same_lists(legacy, t, "cluster.legacy")
        for f, g, what in zip(fast, legacy, ("row_of", "row_ptr", "col")):
            assert np.array_equal(f, g), what
    finally:
        ctx.trim()


# ---------------------------------------------------------------------------------------------- running minimum
@pytest.mark.parametrize("m", LP.LARGE_SIZES)
def test_bh_vector_radix_path(ctx, m):
    """BH of one vector on the radix path with its grid-wide running minimum: 30 % exact ones, tie runs longer than
    three scan blocks across the blocks 2047 | 2048 and 4095 | 4096 of the scanned (reversed) order, values ulps apart,
    0, 5e-324 and 1e-300; then the masked entry point by flag and by negative p"""
    p, _ = LP.bh_pvalues(m)
    tested = (np.random.default_rng(m).random(m) < 0.67).astype(np.uint8)
    t = tested != 0
    try:
        with ctx.params({"bh.vector_path": 1}):
            d_p, d_q = ctx.to_device(p), ctx.empty(m, np.float64)
            with _launches(ctx) as c:
                ctx.bh_dev(d_p, d_q)
            assert _scans(c) == _scan_path(m)
            np.testing.assert_allclose(d_q.to_host(), O.bh_fdr(p), rtol=1e-14, atol=0)
            want = O.bh_fdr(p[t])
            d_t = ctx.to_device(tested)
            d_q.memset(0xFF)
            with _launches(ctx) as c:
                ctx.bh_masked_dev(d_p, d_t, d_q)
            assert _scans(c) == _scan_path(m)
            got = d_q.to_host()
            np.testing.assert_allclose(got[t], want, rtol=1e-14, atol=0)
            assert not got.view(np.uint64)[~t].any()                          # absent entries: exactly +0.0
            d_p.upload(np.where(t, p, -1.0))
            d_q.memset(0xFF)
            with _launches(ctx) as c:
                ctx.bh_masked_dev(d_p, None, d_q)
            assert _scans(c) == _scan_path(m)
            got = d_q.to_host()
            np.testing.assert_allclose(got[t], want, rtol=1e-14, atol=0)
            assert not got.view(np.uint64)[~t].any()
    finally:
        ctx.trim()


# ---------------------------------------------------------------------------------------------- generic column BH
def _columns(n, cols, seed):
    """the column kinds of test_bh_columns_samplesort_vs_generic: continuous with 30 % ones, discrete levels, one value,
    values ulps apart, a crowd of distinct values below 1, a crowd around an ordinary value"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, cols)) ** 2
    p[rng.random((n, cols)) < 0.3] = 1.0
    if cols > 1:
        p[:, 1] = rng.choice([1.0, 0.5, 0.0286, 0.2, 1e-5], size=n)
    if cols > 2:
        p[:, 2] = 0.25
    if cols > 3:
        p[:, 3] = 0.5 + rng.integers(0, 7, size=n) * 2.0 ** -53
    if cols > 5:
        q = rng.random(n)
        p[q < 0.06, 5] = 1.0
        crowd = (q >= 0.06) & (q < 0.14)
        p[crowd, 5] = 1.0 - rng.integers(1, 900, size=int(crowd.sum())) * 2.0 ** -53
    if cols > 6:
        crowd = rng.random(n) < 0.3
        p[crowd, 6] = 0.3 + (rng.standard_cauchy(int(crowd.sum())) * 40).astype(np.int64).clip(-10 ** 7, 10 ** 7) * 2.0 ** -54
    return p


def test_bh_columns_second_transpose_chunk(ctx):
    """[65535 * 32 + 1, 3]: one row into the second chunk of transpose() (in + r0 * cols, out + r0), dense and as
    columns 1..3 of a table of pitch 5; [65535 * 32, 2]: exactly one chunk"""
    n = LP.TRANSPOSE_CHUNK + 1
    assert n > LP.BH_COLS_SAMPLESORT_MAX
    p = _columns(n, 3, 71)
    p[:, 2] = 0.5 + np.random.default_rng(72).integers(0, 7, size=n) * 2.0 ** -53
    p[-1] = (3e-9, 1e-5, 0.5)                                                 # the row of the second chunk matters
    want = O.bh_columns(p)
    try:
        with ctx.params({"bh.columns_path": 1}):
            d = ctx.to_device(p)
            with _launches(ctx) as c:
                ctx.bh_columns_dev(d)
            assert c["transpose_f64_kernel"] == 3                             # two chunks in, one launch back
            np.testing.assert_allclose(d.to_host(), want, rtol=1e-14, atol=0)
            # pitched: guard columns of arbitrary bit patterns on either side
            wide = np.random.default_rng(73).integers(0, 1 << 63, size=(n, 5), dtype=np.uint64).view(np.float64)
            wide[:, 1:4] = p
            d = ctx.to_device(wide)
            with _launches(ctx) as c:
                ctx.bh_columns_pitched_dev(d.offset(1, (n, 3)), n, 3, 5)
            assert c["transpose_f64_kernel"] == 3
            got = d.to_host()
            np.testing.assert_allclose(got[:, 1:4], want, rtol=1e-14, atol=0)
            assert np.array_equal(got[:, [0, 4]].view(np.uint64), wide[:, [0, 4]].view(np.uint64))
            del d
            one = np.ascontiguousarray(p[:LP.TRANSPOSE_CHUNK, :2])
            d = ctx.to_device(one)
            with _launches(ctx) as c:
                ctx.bh_columns_dev(d)
            assert c["transpose_f64_kernel"] == 2
            np.testing.assert_allclose(d.to_host(), O.bh_columns(one), rtol=1e-14, atol=0)
    finally:
        ctx.trim()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_bh_columns_in_groups(ctx):
    """The column-group loop of both column paths, which otherwise runs only when memory is short: bh.max_group cuts the
    37 columns 2..38 of a [1025, 41] table into 1, 3 (16 + 16 + 5; 21 rounds down to 16), 3, 8 (7 x 5 + 2) and 37 groups.
    Every grouping gives the oracle's bits, leaves the two guard columns on each side alone and launches once per group;
    then a dense [1025, 37] table in groups of 16"""
    n, cols, pitch, c0 = 1025, 37, 41, 2
    p = _columns(n, cols, 83)
    want = O.bh_columns(p)
    table = np.random.default_rng(84).integers(0, 1 << 64, size=(n, pitch), dtype=np.uint64).view(np.float64)
    table[:, c0:c0 + cols] = p
    guards = [0, 1, pitch - 2, pitch - 1]

    def check(path, c, groups):
        if path == 1:
            assert c["bh_keys_kernel"] == groups and c["transpose_f64_kernel"] == 2 * groups
        else:
            assert c["bhs_finish_kernel"] == groups and c["radix_hist_kernel"] == 0

    try:
        for path in (1, 2):
            for max_group, groups in ((0, 1), (21, 3), (16, 3), (5, 8), (1, 37)):
                with ctx.params({"bh.columns_path": path, "bh.max_group": max_group}):
                    d = ctx.to_device(table)
                    with _launches(ctx) as c:
                        ctx.bh_columns_pitched_dev(d.offset(c0, (n * pitch - c0,)), n, cols, pitch)
                    got = d.to_host()
                    assert _same_bits(got[:, c0:c0 + cols], want), (path, max_group)
                    assert _same_bits(got[:, guards], table[:, guards]), (path, max_group)
                    check(path, c, groups)
            with ctx.params({"bh.columns_path": path, "bh.max_group": 16}):
                d = ctx.to_device(p)
                with _launches(ctx) as c:
                    ctx.bh_columns_dev(d)
                assert _same_bits(d.to_host(), want), path
                check(path, c, 3)
    finally:
        ctx.trim()


@pytest.mark.parametrize("n,cols,small", [(64 * 3072, 64, True), (64 * 3072 + 1, 64, False), (64 * 3072 + 1, 63, False)])
def test_bh_columns_binscan_switch(ctx, n, cols, small):
    """64 | 65 tiles at 64 segments and 65 tiles at 63: radix_binscan_small_kernel takes n_tiles <= 64 && segs >= 64
    only; against the sample-sort column path bit for bit, and the oracle"""
    assert -(-n // LP.RADIX_TILE[12]) == (64 if small else 65) and n <= LP.BH_COLS_SAMPLESORT_MAX
    assert small == (-(-n // 3072) <= LP.BINSCAN_SMALL_MAX_TILES and cols >= LP.BINSCAN_SMALL_MIN_SEGS)
    p = _columns(n, cols, n * 31 + cols)
    try:
        with ctx.params({"bh.columns_path": 1}):
            d = ctx.to_device(p)
            with _launches(ctx) as c:
                ctx.bh_columns_dev(d)
            generic = d.to_host()
        if small:
            assert c["radix_binscan_small_kernel"] >= 1 and c["radix_binscan_kernel"] == 0
        else:
            assert c["radix_binscan_kernel"] >= 1 and c["radix_binscan_small_kernel"] == 0
        assert c["transpose_f64_kernel"] == 2
        with ctx.params({"bh.columns_path": 2}):
            d = ctx.to_device(p)
            with _launches(ctx) as c:
                ctx.bh_columns_dev(d)
            assert c["radix_hist_kernel"] == 0
            assert np.array_equal(generic.view(np.uint64), d.to_host().view(np.uint64))
        np.testing.assert_allclose(generic, O.bh_columns(p), rtol=1e-14, atol=0)
    finally:
        ctx.trim()


# ---------------------------------------------------------------------------------------------- grid-stride kernels
@pytest.mark.parametrize("n", [LP.QUANTIZE_GRID, LP.QUANTIZE_GRID + 1, 2 * LP.QUANTIZE_GRID + 3])
def test_quantize3_grid_stride(ctx, n):
    """one full pass of the capped grid, one value beyond it (the scalar tail alone), two passes and a tail of three"""
    vals = LP.quantize_values(n)
    want = O.quantize3_fast(vals)
    assert np.array_equal(ctx.quantize3(vals).view(np.uint32), want.view(np.uint32))
    d = ctx.to_device(vals)
    ctx.quantize3_dev(d)
    assert np.array_equal(d.to_host().view(np.uint32), want.view(np.uint32))
    # views that start 1, 2 and 3 floats past a 16-byte boundary (the kernel peels scalars up to the next one), with
    # every length modulo 4, below one grid pass and at this case's size, and views shorter than the peel: the view is
    # quantised bit for bit, the cells on either side of it keep their values
    raw, qraw = vals.view(np.uint32), want.view(np.uint32)
    assert d.ptr % 16 == 0
    for off in (1, 2, 3):
        lengths = [1024 + r for r in range(4)] + [(n - 8) // 4 * 4 + r for r in range(4)] + [1, 2]
        for m in lengths:
            assert off + m < n
            d.upload(vals)
            ctx.quantize3_dev(d.offset(off, (m,)))
            expect = raw.copy()
            expect[off:off + m] = qraw[off:off + m]
            got = d.to_host().view(np.uint32)
            assert np.array_equal(got[:off], raw[:off]) and np.array_equal(got[off + m:], raw[off + m:]), (off, m)
            assert np.array_equal(got, expect), (off, m)
    ctx.trim()


_ps = {}


def _ps_cells():
    if "x" not in _ps:
        _ps["x"] = np.random.default_rng(81).random(3_000_000).astype(np.float32)
        _ps["x"].setflags(write=False)
    return _ps["x"]


@pytest.mark.parametrize("n_low", [LP.MARK_LOW_GRID, LP.MARK_LOW_GRID + 1, 1_300_003])
def test_mark_low_grid_stride(ctx, n_low):
    """one full pass of the capped grid, one index beyond it, two and a half passes: exactly the listed cells (repeats,
    cell 0, the last cell, a cell that only the last entry names) are NaN, every other cell keeps its bits"""
    ps = _ps_cells()
    idx = LP.low_indices(n_low, ps.size)
    low = np.zeros(ps.size, bool)
    low[idx] = True
    got = ctx.mark_low(ps.copy(), idx)
    assert np.array_equal(np.isnan(got), low)
    assert np.array_equal(got.view(np.uint32)[~low], ps.view(np.uint32)[~low])
    ctx.trim()


def test_mark_low_guard_drops_what_the_host_refuses(ctx):
    """indices -1, n_elems and beyond in a list longer than one grid pass: sdice_mark_low refuses the list, the kernel
    behind sdice_mark_low_dev skips them (the cells in front of and behind the array stay as they were)"""
    ps = _ps_cells()
    n, pad = ps.size, 64
    idx = LP.low_indices(LP.MARK_LOW_GRID + 1, n)
    idx[[5, 300_000]] = -1
    idx[[9, LP.MARK_LOW_GRID - 1]] = n
    idx[77], idx[78] = n + 12345, -(1 << 40)
    valid = idx[(idx >= 0) & (idx < n)]
    assert valid.size == idx.size - 6 and idx[-1] == n - 3
    with pytest.raises(SdiceError, match="out of range"):
        ctx.mark_low(ps.copy(), idx)
    low = np.zeros(n, bool)
    low[valid] = True
    host = np.concatenate([np.full(pad, 3.5, np.float32), ps, np.full(pad, 4.5, np.float32)])
    d, d_idx = ctx.to_device(host), ctx.to_device(idx)
    rc = ctx.lib.sdice_mark_low_dev(ctx.h, n, d.offset(pad, (n,)).ptr, d_idx.ptr, idx.size)
    assert rc == 0
    got = d.to_host()
    assert np.array_equal(np.isnan(got[pad:pad + n]), low)
    assert np.array_equal(got[pad:pad + n].view(np.uint32)[~low], ps.view(np.uint32)[~low])
    assert np.array_equal(got[:pad], host[:pad]) and np.array_equal(got[pad + n:], host[pad + n:])
    ctx.trim()
