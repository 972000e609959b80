"""Load sequence of the register-staged PS kernel (ps.hip, ps_tile_v3_kernel): a thread holds up to four vectors of the
tile's own rows, of which the LAST one a tile shape has is loaded behind the lists together with the halo run above the
tile, a vector that no tile of the launch has is not loaded at all, and each halo run takes one vector per thread.

Every case is bit-exact against oracle.calculate_psi_vectorised and against the first-generation kernel (ps.gen1 = 1) on
the same device inputs: PS with its NaNs, int64 exclusion sums, the fused '.3f' store.  Small tables with ps.threads and
ps.tile_rows forced so that several tiles exist at every number of own vectors per thread (1 .. 4), chunked (s = 500:
32, 32, 32 and 29 vectors per row segment; s = 260: a last chunk of 4 columns) and unchunked (s = 100, 256).
"""
import functools

import numpy as np
import pytest

from oracle import oracle_np as O
from splicedice_amd import synth

BIG = (1 << 24) - 1          # (degree + 1) * BIG >= 2^24 for every degree >= 1: items that meet it take 64-bit sums
STEP = 10

# (s, ps.threads, ps.tile_rows): own vectors per thread = ceil(tile_rows * LV / threads), LV = 32 (chunked) or s / 4
SHAPES = {
    1: [(500, 1024, 32), (100, 1024, 32)],
    2: [(500, 512, 32), (100, 512, 32)],
    3: [(500, 512, 48), (260, 512, 48), (100, 512, 48), (256, 1024, 48)],
    4: [(500, 512, 64), (260, 512, 64), (100, 512, 80), (256, 1024, 64)],
}
ALL = [(k,) + shape for k, shapes in SHAPES.items() for shape in shapes]
SOME = [(3, 500, 512, 48), (3, 100, 512, 48), (4, 500, 512, 64), (4, 100, 512, 80), (2, 500, 512, 32)]


def _vectors(s, threads, rows):
    lv = (128 if s > 256 else s) // 4
    return -(-rows * lv // threads)


def test_shapes_cover_one_to_four_vectors_per_thread():
    for k, s, threads, rows in ALL:
        assert _vectors(s, threads, rows) == k and rows % 16 == 0          # (whole reach blocks: reach words are used)


def _ladder(n, fan_at=None, fan=80, star=False):
    """one strand of one chromosome in row order: junction i lists three rows on either side; fan_at: from that row on,
    in place of the ladder, `fan` junctions that share their left end (every one lists all the others) -- or, star: one
    junction over fan - 1 disjoint short ones (it lists them all, each of them lists it)"""
    left = 100 + STEP * np.arange(n, dtype=np.int64)
    if fan_at is not None:
        left[fan_at:] += 100 * STEP                      # a gap in front of the locus and behind it
        left[fan_at + fan:] += 100 * STEP
    right = left + 3 * STEP + STEP // 2
    if fan_at is not None and not star:
        left[fan_at:fan_at + fan] = left[fan_at]
        right[fan_at:fan_at + fan] = left[fan_at] + 1 + np.arange(fan)
    elif fan_at is not None:
        right[fan_at + 1:fan_at + fan] = left[fan_at + 1:fan_at + fan] + 3
        right[fan_at] = right[fan_at + fan - 1] + 1
    z = np.zeros(n, np.int32)
    return z, left.astype(np.int32), right.astype(np.int32), z.astype(np.int8)


def test_fixture_lists():
    """the hand-made loci are what the GPU tests take them for"""
    for at, fan, star, want in ((96, 80, False, [79] * 80), (96, 45, True, [44] + [1] * 44)):
        junc = _ladder(293, fan_at=at, fan=fan, star=star)
        row_of, row_ptr, col = O.cluster_csr(*junc)
        assert np.array_equal(row_of, np.arange(293)) and np.diff(row_ptr)[at:at + fan].tolist() == want
    assert np.diff(O.cluster_csr(*_ladder(293))[1])[:5].tolist() == [3, 4, 5, 6, 6]


@functools.lru_cache(maxsize=None)
def _counts(n, s):
    return synth.make_counts(n, s, 11)


class _Case:
    """junctions clustered on the device, counts in row order on the device, the oracle's answer"""

    def __init__(self, ctx, junc, s, edit=None):
        self.ctx, self.s = ctx, s
        n = junc[0].size
        d = [ctx.to_device(x) for x in junc]
        d_row_of, self.d_rp = ctx.empty(n, np.int32), ctx.empty(n + 1, np.int64)
        self.d_col, nnz = ctx.cluster_dev(*d, d_row_of, self.d_rp, sync=True)
        self.row_ptr, self.col = self.d_rp.to_host(), self.d_col.to_host()
        want = O.cluster_csr(*junc)
        assert np.array_equal(self.row_ptr, want[1]) and np.array_equal(self.col, want[2])
        counts = np.zeros((n, s), np.int32)
        counts[d_row_of.to_host()] = _counts(n, s)
        if edit is not None:
            edit(counts)
        self.d_counts = ctx.to_device(counts)
        self.ps, self.excl = O.calculate_psi_vectorised(counts, self.row_ptr, self.col)
        self.q = O.quantize3_fast(self.ps)
        self.d_excl, self.d_ps = ctx.empty((n, s), np.int64), ctx.empty((n, s), np.float32)

    def launch(self, knobs, want_excl, d_col=None):
        with self.ctx.params(knobs):
            self.d_ps.memset(0xFF)
            if want_excl:
                self.d_excl.memset(0xFF)
            self.ctx.ps_dev(self.d_counts, self.d_rp, self.d_col if d_col is None else d_col,
                            self.d_excl if want_excl else None, self.d_ps)
            return self.d_ps.to_host(), self.d_excl.to_host() if want_excl else None

    def check(self, threads, rows, d_col=None, extra=None):
        """PS + excl, PS alone and the fused '.3f' PS: second-generation kernel == oracle == first-generation kernel"""
        base = {"ps.threads": threads, "ps.tile_rows": rows, **(extra or {})}
        for q3, want_excl in ((0, True), (0, False), (1, False), (1, True)):
            want = self.q if q3 else self.ps
            ps, excl = self.launch({**base, "ps.quantize3": q3}, want_excl, d_col)
            ps1, excl1 = self.launch({**base, "ps.quantize3": q3, "ps.gen1": 1}, want_excl, d_col)
            assert np.array_equal(ps, want, equal_nan=True), (q3, want_excl)
            assert np.array_equal(ps, ps1, equal_nan=True), (q3, want_excl)
            if want_excl:
                assert excl.dtype == np.int64 and np.array_equal(excl, self.excl) and np.array_equal(excl, excl1)


@pytest.mark.gpu
@pytest.mark.parametrize("last", ["short", "long"])
@pytest.mark.parametrize("k,s,threads,rows", ALL)
def test_gene_shaped_tables(ctx, k, s, threads, rows, last):
    """gene-shaped junctions, n no multiple of 16: a last tile of 5 rows (a single vector of it exists), or one that
    lacks 3 rows (its last vector is partly there)"""
    n = 6 * rows + (5 if last == "short" else rows - 3)
    assert n % 16
    _Case(ctx, synth.make_junctions(n, 3), s).check(threads, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [500, 100])
def test_default_geometry(ctx, s):
    """no knob forced: one tile, or a few, of the production shape (three vectors per thread at s = 500)"""
    _Case(ctx, synth.make_junctions(293, 3), s).check(1024, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("star", [False, True])
@pytest.mark.parametrize("k,s,threads,rows", SOME)
def test_dense_loci(ctx, k, s, threads, rows, star):
    """from the first row of tile 2 on: 80 mutually overlapping junctions (lists beyond the LDS stage, reach beyond the
    halo), or one junction over the 44 rows behind it (a halo run above the tile as long as the window allows)"""
    at = 2 * rows
    _Case(ctx, _ladder(at + 197, fan_at=at, fan=45 if star else 80, star=star), s).check(threads, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["last_vector", "first_vector", "halo_below", "halo_above"])
@pytest.mark.parametrize("k,s,threads,rows", SOME)
def test_count_bound_comes_from_every_load(ctx, k, s, threads, rows, where):
    """one row of counts of 2^24 - 1 ((degree + 1) * count >= 2^24: every item that can meet it takes 64-bit sums) that
    tile 2 sees only through the last own vector of its threads, only through the first one, only in the halo run below
    it, only in the run above it: the tile's bound is the maximum over everything it loaded"""
    row = {"last_vector": 3 * rows - 2, "first_vector": 2 * rows + 3, "halo_below": 2 * rows - 1,
           "halo_above": 3 * rows}[where]

    def edit(counts):
        counts[row] = BIG

    case = _Case(ctx, _ladder(4 * rows + 37), s, edit)
    assert case.excl.max() >= BIG
    case.check(threads, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("k,s,threads,rows", SOME)
def test_without_reach_words(ctx, k, s, threads, rows):
    """the same lists from a copy of the context's list, and with ps.use_reach = 0: both halo runs at their full length"""
    case = _Case(ctx, synth.make_junctions(6 * rows + 5, 3), s)
    case.check(threads, rows, d_col=ctx.to_device(case.col))
    case.check(threads, rows, extra={"ps.use_reach": 0})
