"""The 16-bit-window PS kernel (ps.hip, ps_tile_w16_kernel; plan: psplan.cpp, kern 3) against the integer oracle of
ps_count_fixtures and against the register-staged kernel (ps.w16 = 0) on the same device inputs, bit for bit (NaN = NaN):
exclusion sums alone, the fused '.3f' PS alone, and both outputs, on outputs filled with 0xA5.  Every launch asserts the
plan it ran (sdice_ps_last_plan).

Shapes: s = 260 (a last chunk of 4 columns), 500 (the headline pitch) and 516 (128-byte-aligned rows) at n = 1, 95, 96, 97
and 193 rows (ps.w16 = 2 takes tables shorter than a tile to the kernel); counts on either side of every bound the kernel
has (ps_w16_fixtures.py, proven on the host by test_ps_w16_fixtures_cpu.py), the 2^24 fixtures and the palette up to
2^31 - 1 of ps_count_fixtures, dense loci, and lists clustered on the device (reach words) with and without ps.use_reach.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402
import ps_w16_fixtures as WF  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

pytestmark = pytest.mark.gpu

W16 = {"chunk_cols": 256, "threads": 1024}             # the kernel's geometry
ON = 2                                                 # ps.w16: the kernel at any row count
# (want_excl, want_ps, ps.quantize3): WEXCL alone, WPS + Q3, both outputs
OUTPUTS = ((True, False, 0), (False, True, 1), (True, True, 0))
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def _check(res, knobs=None, expect=None, what=""):
    """every output set through kern 3 and through kern 0: the oracle's bits from both, and the plans"""
    ps_want, excl_want, q_want = res.want
    n, s = res.n, res.s
    rows = min(WF.TILE, n)
    want_plan = {"kern": 3, "vec": 4, **W16, "tile_rows": rows, "halo": WF.HALO, "n_tiles": -(-n // rows),
                 "n_chunks": -(-s // W16["chunk_cols"]), "nt": 0, **(expect or {})}
    for want_excl, want_ps, q3 in OUTPUTS:
        got = {}
        for w16 in (ON, 0):
            ps, excl, plan, ran = res.launch({**(knobs or {}), "ps.w16": w16, "ps.quantize3": q3}, want_excl, want_ps)
            tag = f"{what} n={n} s={s} w16={w16} excl={want_excl} ps={want_ps} q3={q3} plan={plan}"
            if w16:
                for key, value in want_plan.items():
                    assert plan[key] == value, f"{key}: {tag}"
            else:
                assert plan["kern"] == 0 and plan["chunk_cols"] == 128, tag
            assert sum(ran.values()) == 1, tag
            if want_ps:
                assert PC.same_ps(ps, q_want if q3 else ps_want), PC._first_diff(ps, q_want if q3 else ps_want, tag)
            else:
                assert (ps.view(np.uint32) == FILL32).all(), tag
            if want_excl:
                assert excl.dtype == np.int64 and np.array_equal(excl, excl_want), PC._first_diff(excl, excl_want, tag)
            else:
                assert (excl.view(np.uint64) == FILL64).all(), tag
            got[w16] = (ps, excl)
        assert PC.same_ps(got[ON][0], got[0][0]) and np.array_equal(got[ON][1], got[0][1])


def _resident(ctx, fx):
    return PC.Resident(ctx, fx.counts, fx.row_ptr, fx.col, fx.want)


def _table(n, s):
    if n > 8:
        return PC.gene_table(n, s)                        # gene-shaped lists, a far pair, palette rows, a row at 2^31 - 1
    rng = np.random.default_rng([n, s])
    counts = rng.integers(0, 40, (n, s))
    counts[0, ::7] = np.resize(np.asarray(PC.PALETTE, np.int64), len(range(0, s, 7)))
    return PC.Fixture(counts, np.zeros(n + 1, np.int64), np.zeros(0, np.int32))


@pytest.mark.parametrize("n", [1, 95, 96, 97, 193])
@pytest.mark.parametrize("s", [260, 500, 516])
def test_shapes(ctx, s, n):
    """one row, a tile that lacks a row, one whole tile, a last tile of one row, two tiles and one row"""
    res = _resident(ctx, _table(n, s))
    _check(res, what="shapes")
    # the default, ps.w16 = 1: a table shorter than one tile keeps the register-staged kernel
    ps, excl, plan, _ = res.launch({}, True, True)
    assert plan["kern"] == (3 if n >= WF.TILE else 0), plan
    assert PC.same_ps(ps, res.want[0]) and np.array_equal(excl, res.want[1]), plan


@pytest.mark.parametrize("s", [260, 500])
def test_window_maxima(ctx, s):
    """a tile maximum of 65534, 65535, 65536 and 2^31 - 1 in an own row, in either halo run and beyond the window"""
    _check(_resident(ctx, WF.maxima(s)), what="maxima")


@pytest.mark.parametrize("s", [260, 500])
def test_packed_sum_limit(ctx, s):
    """(degree + 1) x bound at 65535 (the halves hold the totals) and at 65536 (they do not)"""
    _check(_resident(ctx, WF.limits(s)), what="limits")


@pytest.mark.parametrize("s", [260])
def test_dense_loci(ctx, s):
    """degrees 39 (tier 1 and tier 2), 300 (beyond the degree cutoff) and lists beyond the offset stage"""
    _check(_resident(ctx, WF.dense(s)), what="dense")


def test_the_2_24_fixtures_and_the_palette(ctx):
    """the tiles around 2^24 of ps_count_fixtures (laid out for 128-row tiles: here they fall on the kernel's 96-row
    tiles, the bits are the oracle's all the same), sums past 2^40, and every magnitude up to 2^31 - 1 on a star"""
    _check(_resident(ctx, PC.bound(260)), what="bound")
    _check(_resident(ctx, PC.large_sums(260)), what="large sums")
    _check(_resident(ctx, PC.palette(260)), what="palette")


@pytest.mark.parametrize("s", [260, 500])
def test_reach_words_of_the_context_lists(ctx, s):
    """gene-shaped junctions clustered on the device: the halo runs are sized from the reach words (capacity 24 rows: a
    thread holds one vector of a run, two where a run is longer than 16 rows); ps.use_reach 0 stages 16 rows on either side"""
    from splicedice_amd import synth
    n = 500
    junc = synth.make_junctions(n, 3)
    d = [ctx.to_device(x) for x in junc]
    d_row_of, d_rp = ctx.empty(n, np.int32), ctx.empty(n + 1, np.int64)
    d_col, nnz = ctx.cluster_dev(*d, d_row_of, d_rp, sync=True)
    row_ptr, col = d_rp.to_host(), d_col.to_host()
    counts = PC.gene_table(n, s).counts
    ps, excl = PC.oracle(counts, row_ptr, col)
    res = PC.Resident(ctx, counts, row_ptr, col, (ps, excl, O.quantize3_fast(ps)), d_rp=d_rp, d_col=d_col)
    _check(res, expect={"use_reach": 1, "halo": 24}, what="reach")
    _check(res, {"ps.use_reach": 0}, {"use_reach": 0}, what="no reach")


def test_halo_runs_of_two_vectors_per_thread(ctx):
    """ps.halo_rows 32 on lists given by the caller: both runs are staged in full, 32 rows each -- two vectors per thread;
    the window then leaves 83 rows to a tile"""
    res = _resident(ctx, PC.gene_table(193, 500))
    _check(res, {"ps.halo_rows": 32}, {"tile_rows": 83, "halo": 32, "n_tiles": 3}, what="halo 32")
    _check(res, {"ps.halo_rows": 0}, {"tile_rows": 96, "halo": 0, "n_tiles": 3}, what="halo 0")


def test_tile_knobs_keep_the_register_staged_kernel(ctx):
    """the kernel has one geometry: a call that sets a knob of the tile shape gets the kernel that takes any shape"""
    res = _resident(ctx, PC.gene_table(193, 260))
    for knobs in ({"ps.tile_rows": 32}, {"ps.chunk_cols": 128}, {"ps.threads": 512}, {"ps.lds_bytes": 160 * 1024}):
        ps, excl, plan, _ = res.launch({**knobs, "ps.w16": ON}, True, True)
        assert plan["kern"] == 0, (knobs, plan)
        assert PC.same_ps(ps, res.want[0]) and np.array_equal(excl, res.want[1]), plan
