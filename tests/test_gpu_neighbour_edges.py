"""neighbours_kernel (cluster_fast.hip) at the edges of its search, its count and its window: the fixtures of
tests/neighbour_edge_fixtures.py (test_neighbour_edges_cpu.py proves on the host that each one hits the edge it is
named after).  Constants of the kernel: T = 512, HB = 256, HF = 128, KMAX = 16, STAGE = 11 T.

For every fixture, with the kernel's grid as the device holds it and capped at 3 workgroups (each then walks several
tiles), all by integer or bit equality:
  * row_ptr and col of sdice_cluster, element for element, against cluster_referee (closed-form row_ptr, brute-force
    row_list of every row), and row_of against the identity (the fixtures are in row order);
  * the same arrays from the generic chain (cluster.generic = 1);
  * cluster_dev -> ps_dev on the context's own lists (what the 16-row reach words are for) with an 8-column count
    table against oracle_np.calculate_psi_vectorised: PS with its NaNs, int64 exclusion sums.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbour_edge_fixtures as F  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

pytestmark = pytest.mark.gpu

COLS = 8


@functools.lru_cache(maxsize=None)
def _counts(name):
    n = F.junctions(name)[0].size
    rng = np.random.default_rng(sum(map(ord, name)))
    c = rng.integers(0, 50, (n, COLS)).astype(np.int32)
    c[rng.random(n) < 0.1] = 0                 # (0 / 0 -> NaN)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ps_want(name):
    row_ptr, col = F.reference(name)
    return O.calculate_psi_vectorised(_counts(name), row_ptr, col)


def _check_lists(got, name, what):
    row_of, row_ptr, col = got
    want_ptr, want_col = F.reference(name)
    assert np.array_equal(row_of, np.arange(want_ptr.size - 1)), f"{name} {what}: row_of"
    assert row_ptr.shape == want_ptr.shape and np.array_equal(row_ptr, want_ptr), f"{name} {what}: row_ptr"
    assert col.shape == want_col.shape and np.array_equal(col, want_col), f"{name} {what}: col"


@pytest.mark.parametrize("nb_grid", [0, 3])
@pytest.mark.parametrize("name", F.NAMES)
def test_neighbour_edges(ctx, name, nb_grid):
    junc = F.junctions(name)
    n = junc[0].size
    with ctx.params({"cluster.nb_grid": nb_grid}):
        _check_lists(ctx.cluster(*junc), name, "fast chain")
        with ctx.params({"cluster.generic": 1}):
            _check_lists(ctx.cluster(*junc), name, "generic chain")
        # PS on the device lists: the tile halos come from the reach words the neighbour kernel wrote
        d = [ctx.to_device(x) for x in junc]
        d_row_of, d_row_ptr = ctx.empty(n, np.int32), ctx.empty(n + 1, np.int64)
        d_col, nnz = ctx.cluster_dev(*d, d_row_of, d_row_ptr, sync=True)
    want_ptr, want_col = F.reference(name)
    assert nnz == want_col.size
    assert np.array_equal(d_row_ptr.to_host(), want_ptr)
    if nnz:
        assert np.array_equal(d_col.offset(0, (nnz,)).to_host(), want_col)
    d_counts = ctx.to_device(_counts(name), np.int32)
    d_excl, d_ps = ctx.empty((n, COLS), np.int64), ctx.empty((n, COLS), np.float32)
    d_excl.memset(0xFF)
    d_ps.memset(0xFF)
    ctx.ps_dev(d_counts, d_row_ptr, d_col, d_excl, d_ps)
    want_ps, want_excl = _ps_want(name)
    assert np.array_equal(d_excl.to_host(), want_excl), f"{name}: exclusion sums"
    assert np.array_equal(d_ps.to_host(), want_ps, equal_nan=True), f"{name}: PS"
