"""GPU: a result must not depend on what the context held before the call.

The library keeps device memory between calls and works in it again without clearing it: the arena (every call's scratch
starts at offset 0 of the same chunk), the neighbour-list and block-reach buffers of the clustering, which only grow.
What is right after a fresh hipMalloc (zeros, usually) is exactly what a missing memset needs, so the cases of
call_order_fixtures.py are run here

  b. after every other case of the catalogue on the shared context, against a run alone on a context of their own;
  c. on scratch regions (Context.scratch_regions) filled with 0x5A, 0xFF and 0x00 over their whole length (a case that
     takes nothing from the arena runs on the filled arena of another call);
  a. with the region list itself checked;
  d. in sequences that exercise the state that is not scratch: the grown clustering caches and whose reach they hold,
     the status block after a refused clustering, an asynchronous clustering resolved after another call, a caller's
     copy of the lists, the log-factorial table of Fisher at two lengths, sdice_trim, the two BH column paths in turn.

Every comparison with a referee is the case's own (call_order_fixtures.py); every comparison between two runs is
np.array_equal on the bit patterns.  Every input is a valid call sequence; the fill bytes stand for what another call may
leave, since the library promises nothing about the contents of scratch.

The order test runs first and is quadratic in the number of cases: every case is a successor, and every case a predecessor.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import fisher_referee as FR  # noqa: E402
import pair_fixtures as PF  # noqa: E402
import rank_support as RS  # noqa: E402
from bh_fixtures import bh_values  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd.engine import Context, SdiceError  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(CF.CASES)
PREDECESSORS = NAMES
FILLS = (0x5A, 0xFF, 0x00)
SDICE_ERR_ARG = -1


def assert_same_run(got, base, label):
    """two runs of one case: every field equal in every bit"""
    assert list(got) == list(base), label
    for name in base:
        assert got[name].dtype == base[name].dtype and got[name].shape == base[name].shape, (label, name)
        assert np.array_equal(RS.bits(got[name]), RS.bits(base[name])), (label, name, "differs from the other run")


def regions_of(ctx):
    return [(name, d.ptr, d.nbytes) for name, d in ctx.scratch_regions()]


# ================================================================================================ b. real leftovers
@pytest.mark.parametrize("name", NAMES)
def test_result_ignores_what_the_call_before_left(ctx, name):
    case = CF.CASES[name]
    with Context(ctx.device) as own:
        base = case.run(own)
    case.check(base, "alone on a context of its own")
    for other in PREDECESSORS:
        if other == name:
            continue
        CF.CASES[other].run(ctx)
        assert_same_run(case.run(ctx), base, f"{name} after {other}")


# ================================================================================================ c. filled scratch
@pytest.mark.parametrize("fill", FILLS, ids=lambda b: f"fill_{b:02X}")
@pytest.mark.parametrize("name", NAMES)
def test_result_ignores_scratch_contents(ctx, name, fill):
    case = CF.CASES[name]
    ctx.trim()                              # (the arena then has this case's size, not that of the largest call so far)
    if not case.arena:                      # (a call that takes nothing from the arena would leave none to fill: the chunk of
        CF.CASES["bh vector radix"].run(ctx)    # another call, which Arena::reset keeps, stands for what came before it)
    first = case.run(ctx)
    case.check(first, "first run")
    for _ in range(3):                      # until a run leaves the regions as it found them (a call that grew the arena by
        before = regions_of(ctx)            # chunks gets one chunk of the whole size at the next reset)
        assert_same_run(case.run(ctx), first, f"{name} again")
        if regions_of(ctx) == before:
            break
    else:
        raise AssertionError(f"{name}: the scratch regions never settle")
    filled = ctx.scratch_regions()
    assert filled, f"{name}: no scratch region to fill"
    for _, d in filled:
        d.memset(fill)
    got = case.run(ctx)                     # (a chain is filled before the chain, never between its calls)
    after = ctx.scratch_regions()
    assert [(n, d.ptr, d.nbytes) for n, d in after] == [(n, d.ptr, d.nbytes) for n, d in filled], \
        f"{name}: the call moved its scratch, so the fill missed the memory it used"
    assert_same_run(got, first, f"{name} on scratch filled with {fill:#04x}")
    case.check(got, f"scratch filled with {fill:#04x}")
    if case.arena:                          # the call worked where the fill was
        arena = [d for n, d in after if n == "arena"]
        assert arena, name
        assert any((d.to_host() != fill).any() for d in arena), f"{name}: the arena still holds only {fill:#04x}"


# ================================================================================================ a. the region list
def test_scratch_regions(ctx):
    ctx.trim()
    assert "arena" not in [n for n, _, _ in regions_of(ctx)]
    bh = CF.CASES["bh vector radix"]
    bh.run(ctx)
    one = [r for r in regions_of(ctx) if r[0] == "arena"]
    assert len(one) == 1 and one[0][2] > 0
    bh.run(ctx)
    assert [r for r in regions_of(ctx) if r[0] == "arena"] == one
    with Context(ctx.device) as own:        # (the shared context's caches may have grown in earlier tests: sizes on a fresh one)
        assert regions_of(own) == []
        n = CF.CLUSTER_LARGE
        CF.CASES["cluster->ps"].run(own)
        got = {name: nbytes for name, _, nbytes in regions_of(own)}
        assert got["cluster.col"] == 4 * (16 * n + 1024)              # ensure_col(16 n + 1024), int32 entries
        assert got["cluster.reach"] == 4 * (-(-n // 16) + 1)          # ensure_reach: one word per 16 rows, plus one
        names = [name for name, _, _ in regions_of(own)]
        assert names == ["arena", "cluster.col", "cluster.reach"]
        name, p, nbytes = C.c_char_p(), C.c_void_p(), C.c_int64()
        args = (C.byref(name), C.byref(p), C.byref(nbytes))
        assert own.lib.sdice_scratch_region(own.h, len(names), *args) == SDICE_ERR_ARG
        assert own.lib.sdice_scratch_region(own.h, -1, *args) == SDICE_ERR_ARG
        assert own.lib.sdice_scratch_region(None, 0, *args) == SDICE_ERR_ARG
        assert own.lib.sdice_scratch_region(own.h, 0, None, None, None) == 0
        assert regions_of(own) == regions_of(own)                      # changes nothing
    for name, d in ctx.scratch_regions():
        assert d.dtype == np.uint8 and not d.owned and d.shape == (d.nbytes,), name


# ================================================================================================ d. state that is not scratch
def test_clusterings_of_three_sizes_share_the_grown_caches(ctx):
    """5 000, then 300, then 5 000 junctions, PS after each on the context's lists: the list and reach buffers have grown and
    stay, and each PS uses the reach of its own clustering"""
    large, small = CF.CASES["cluster->ps"], CF.CASES["cluster->ps one bucket"]
    first = large.run(ctx)
    large.check(first, "5 000")
    caches = [r for r in regions_of(ctx) if r[0] != "arena"]
    assert [r[0] for r in caches] == ["cluster.col", "cluster.reach"]
    small.check(small.run(ctx), "300 after 5 000")
    assert [r for r in regions_of(ctx) if r[0] != "arena"] == caches
    again = large.run(ctx)
    large.check(again, "5 000 after 300")
    assert_same_run(again, first, "5 000 after 300")
    assert [r for r in regions_of(ctx) if r[0] != "arena"] == caches


def _refused(kind):
    """a refusal case of test_gpu_cluster_sort_sweeps.py (test_invalid_in_a_late_tile, _expect_duplicate) on the 5 000 table"""
    a = [x.copy() for x in CF.CASES["cluster->ps"].inputs["junctions"]]
    n = a[0].size
    if kind == "right_below_left":
        a[2][n - 1] = a[1][n - 1] - 1
        return a, "invalid junction"
    for x in a:
        x[n - 1] = x[7]
    return a, "duplicate"


@pytest.mark.parametrize("kind", ["right_below_left", "duplicate"])
def test_valid_clustering_after_a_refused_one(ctx, kind):
    bad, message = _refused(kind)
    d_in, d_row_of, d_row_ptr = CF.cluster_device(ctx, bad)
    with pytest.raises(SdiceError, match=message):
        ctx.cluster_dev(*d_in, d_row_of, d_row_ptr)
    ctx.cluster_dev(*d_in, d_row_of, d_row_ptr, sync=False)            # and once more without waiting for its status
    with pytest.raises(SdiceError, match=message):
        ctx.sync()
    for d in (*d_in, d_row_of, d_row_ptr):
        d.free()
    case = CF.CASES["cluster->ps"]
    case.check(case.run(ctx), f"after a refused clustering ({kind})")
    nnz, reach = ctx.cluster_status()                                   # clean: nothing deferred, nothing sticky
    assert nnz == case.want["col"].size and reach > 0
    d_in, d_row_of, d_row_ptr = CF.cluster_device(ctx, case.inputs["junctions"])
    d_col, _ = ctx.cluster_dev(*d_in, d_row_of, d_row_ptr, sync=False)  # (the sticky word is read when a deferred status is)
    assert ctx.cluster_status() == (nnz, reach)
    ctx.sync()
    assert np.array_equal(d_col.offset(0, (nnz,)).to_host(), case.want["col"])
    for d in (*d_in, d_row_of, d_row_ptr):
        d.free()


def test_asynchronous_clustering_resolved_after_another_call(ctx):
    """cluster_dev(sync=False), then bh_dev, then cluster_status: the status block outlives the arena's next tenant"""
    case, bh = CF.CASES["cluster->ps"], CF.CASES["bh vector radix"]
    d_in, d_row_of, d_row_ptr = CF.cluster_device(ctx, case.inputs["junctions"])
    d_col, nnz = ctx.cluster_dev(*d_in, d_row_of, d_row_ptr, sync=False)
    assert nnz is None
    q = bh.run(ctx)
    nnz, reach = ctx.cluster_status()
    got = dict(row_of=d_row_of.to_host(), row_ptr=d_row_ptr.to_host(), col=d_col.offset(0, (nnz,)).to_host())
    got.update(CF.ps_on(ctx, case.inputs["counts"], d_row_ptr, d_col))
    for d in (*d_in, d_row_of, d_row_ptr):
        d.free()
    assert nnz == case.want["col"].size and reach > 0
    case.check(got, "resolved after bh_dev")
    bh.check(q, "between an asynchronous clustering and its status")


def _other_table():
    """a different clustering of the same n as the cluster->ps case"""
    x = CF.cluster_inputs(CF.CLUSTER_LARGE, 977)
    assert x["junctions"][0].size == CF.CLUSTER_LARGE
    assert not np.array_equal(x["junctions"][1], CF.CASES["cluster->ps"].inputs["junctions"][1])
    return x


def test_ps_on_a_copy_of_the_lists_ignores_the_reach_of_another_clustering(ctx):
    case = CF.CASES["cluster->ps"]
    d_in, d_row_of, d_row_ptr = CF.cluster_device(ctx, case.inputs["junctions"])
    d_col, nnz = ctx.cluster_dev(*d_in, d_row_of, d_row_ptr)
    d_copy = ctx.to_device(d_col.to_host())                              # caller-owned
    other = _other_table()
    o_in, o_row_of, o_row_ptr = CF.cluster_device(ctx, other["junctions"])
    ctx.cluster_dev(*o_in, o_row_of, o_row_ptr)                          # same n: its reach is what the context holds now
    got = CF.ps_on(ctx, case.inputs["counts"], d_row_ptr, d_copy)
    assert np.array_equal(got["excl"], case.want["excl"])
    assert np.array_equal(got["ps"], case.want["ps"], equal_nan=True)
    for d in (*d_in, d_row_of, d_row_ptr, d_copy, *o_in, o_row_of, o_row_ptr):
        d.free()


def test_ps_on_the_lists_of_a_generic_clustering_after_a_fast_one(ctx):
    """the generic chain leaves no reach (reach_n = 0): PS on the context's lists must not read the fast chain's"""
    CF.CASES["cluster->ps"].run(ctx)
    other = _other_table()
    with ctx.params({"cluster.generic": 1}):
        got = CF.run_cluster_ps(ctx, other)
    want = CF.want_cluster_ps(other)
    CF.check_cluster_ps(got, want, "generic after fast")


# ---- Fisher: the log-factorial table is rebuilt when fisher.table_max changes and reused otherwise
LF_SHORT = PF.TABLE_MAX_T          # 256: the "edge" palette has totals of T - 1 (the last entry) and T (beyond the table)


def _fisher_rows(palettes, seed):
    ref = PF.PaletteRef(palettes)
    incl, excl, _, _ = ref.rows(CF.PAIR_S, reps=4, seed=seed)
    return incl, excl


def _fisher_run(ctx, incl, excl):
    d_incl, d_excl = ctx.to_device(incl), ctx.to_device(excl)
    d_p = ctx.empty((incl.shape[0], CF.PAIR_S * (CF.PAIR_S - 1) // 2), np.float64).memset(CF.FILL)
    ctx.fisher_pairs_dev(d_incl, d_excl, d_p)
    p = d_p.to_host()
    for d in (d_incl, d_excl, d_p):
        d.free()
    return p


def _fisher_check(p, incl, excl, label):
    """against fisher_referee by the rule of test_gpu_pair_large_counts.py:54 (_check, _rtol; every total here is inside the
    default table): 1e-9 up to a total of 5e4, 1e-7 above, under 2e-280 where the referee is under 1e-280"""
    iu, ju = np.triu_indices(CF.PAIR_S, 1)
    for r in range(incl.shape[0]):
        for q, (i, j) in enumerate(zip(iu, ju)):
            t = (int(incl[r, i]), int(incl[r, j]), int(excl[r, i]), int(excl[r, j]))
            want = FR.two_sided(*t)[0]
            if want < 1e-280:
                assert 0.0 <= p[r, q] < 2e-280, (label, t)
            else:
                rtol = PF.P_RTOL_TIGHT if sum(t) <= PF.BIG_TOTAL else PF.P_RTOL_BIG
                assert abs(p[r, q] - want) <= rtol * want, (label, t, p[r, q], want)


def test_fisher_table_of_two_lengths_in_turn(ctx):
    small, large = _fisher_rows(("edge", "under", "zeros"), 5), _fisher_rows(("thousands", "big"), 6)
    assert (small[0] + small[1]).max() == LF_SHORT // 2 and (large[0] + large[1]).min() > LF_SHORT    # (a table: two samples)
    with ctx.params({"fisher.table_max": LF_SHORT}):
        first = _fisher_run(ctx, *small)
    _fisher_check(first, *small, "short table")
    long_run = _fisher_run(ctx, *large)                                  # the default table: longer, built anew
    _fisher_check(long_run, *large, "default table")
    with ctx.params({"fisher.table_max": LF_SHORT}):
        again = _fisher_run(ctx, *small)
    _fisher_check(again, *small, "short table again")
    assert np.array_equal(again.view(np.uint64), first.view(np.uint64))


@pytest.mark.parametrize("name", ["cluster->ps", "bh columns sample sort", "fisher_pairs", "sample_gram", "sort_unique_u64"])
def test_same_result_after_trim(ctx, name):
    case = CF.CASES[name]
    first = case.run(ctx)
    case.check(first, "before trim")
    ctx.trim()
    assert "arena" not in [n for n, _, _ in regions_of(ctx)]
    assert_same_run(case.run(ctx), first, f"{name} after trim")


def test_bh_columns_paths_in_turn(ctx):
    """the radix path, the default (sample sort at this size), the radix path again, on one table"""
    case = CF.CASES[CF.BH_COLUMNS_SAMPLESORT]
    first = case.run(ctx, {"bh.columns_path": 1})
    case.check(first, "columns_path 1")
    case.check(case.run(ctx, {}), "default path")
    again = case.run(ctx, {"bh.columns_path": 1})
    case.check(again, "columns_path 1 again")
    assert_same_run(again, first, "columns_path 1, default, 1")


def test_bh_vector_after_masked_vector(ctx):
    """the masked forms count their present entries in scratch (m_eff); the plain form that follows must not see it"""
    p = bh_values(CF.BH_RADIX_M, np.random.default_rng(5))
    CF.CASES["bh vector radix masked"].run(ctx)
    with ctx.params({"bh.vector_path": 1}):
        d_p, d_q = ctx.to_device(p), ctx.empty(p.size, np.float64).memset(CF.FILL)
        ctx.bh_dev(d_p, d_q)
        q = d_q.to_host()
    assert np.array_equal(q.view(np.uint64), O.bh_fdr(p).view(np.uint64))
    for d in (d_p, d_q):
        d.free()
