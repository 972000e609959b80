"""GPU: the Fisher and chi2 pair kernels on LARGE counts against an exact referee (tests/fisher_referee.py, mpmath at 60
digits): real tables on both sides of the log-factorial table's end (totals of 2^20 - 1, 2^20, 2^20 + 1 at the default
fisher.table_max), balanced tables at counts of 1e5, 3e5 and 1e6 (walks of 5e5 steps), small inclusion counts against
exclusion sums of 1e7, 1e9, 2^31 +- 1, 1e10, 2^40 and 2^52, the largest int32 inclusion count, and the refusal of
everything beyond the count range of include/sdice.h (a table's total, a d and b c at most 2^53).

Every set of pair_fixtures.LARGE_SETS goes through every entry point: sdice_fisher_tables, sdice_fisher_pairs,
sdice_fisher_pair_list (every pair reversed, then repeats) and the two _dev forms; the small-a sets again under
fisher.unroll 4, 8, 16 and 24; chi2 through its four.  A row mixes small and huge columns, so the lanes of a wave carry
walks of 8 to 5e5 steps, and flagged (beyond the table) and unflagged pairs share a row.

Tolerances: 1e-9 for totals up to 5e4 and 1e-7 up to the end of the table, the project's figures; beyond the table
BEYOND_RTOL (see there).  Referee p-values below 1e-280 are asked to come out below 2e-280.  tests/test_fisher_referee_cpu.py
holds what makes the fixtures fair (no near-ties, the step budget, the count range) and runs without a GPU.

Before log_pmf_beyond_table took the saddle-point form, pmf(a) beyond the table was a difference of nine lgamma values:
on that library, held to the project's 1e-6, test_fisher_large_counts_every_entry_point fails on the sets 1e9 (1.5e-5
relative), 2^31 (4.5e-5), 1e10 (1.5e-4), 2^40 (2.1e-2), 2^52 (a factor of 6.6e3) and int32 (7.5e-3) and passes on
boundary (2^20 +- 1), balanced and 1e7 (1.4e-7).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_referee as R  # noqa: E402
from pair_fixtures import (BIG_TOTAL, LARGE_SETS, LARGE_SMALL_A, LF_TABLE_DEFAULT, P_RTOL_BIG, P_RTOL_TIGHT, large_arrays,  # noqa: E402
                           large_pair_list, large_tables)
from splicedice_amd.engine import SdiceError, _ptr  # noqa: E402

gpu = pytest.mark.gpu
P_RTOL = 1e-6          # the project's stated tolerance (north_star)
# Beyond the log-factorial table p = exp(log pmf(a)) * (1 + sum): log pmf(a) in the saddle-point form is a dozen terms of at
# most |log p| <= 645 (an ulp of 1.1e-13), the sum is good to 6e-14 after 5e5 steps.  Worst seen over all fixtures: 1.7e-13
# in the float64 model on the host, MEASURED_WORST on an MI355X (the 2^31 set; DESIGN.md section 7 has the figure per
# magnitude); the bound is four times that, as margin for another device library's log and exp.
MEASURED_WORST = 2.7e-13
BEYOND_RTOL = min(4 * MEASURED_WORST, P_RTOL)
SDICE_ERR_ARG = -1


def _rtol(t):
    tot = sum(t)
    return P_RTOL_TIGHT if tot <= BIG_TOTAL else P_RTOL_BIG if tot < LF_TABLE_DEFAULT else BEYOND_RTOL


def _table(incl, excl, r, i, j):
    return int(incl[r, i]), int(incl[r, j]), int(excl[r, i]), int(excl[r, j])


def _check(got, tables, what, want_of=lambda t: R.two_sided(*t)[0], rtol_of=_rtol):
    """got[k] against the referee on tables[k]; returns the worst relative error beyond and inside the table"""
    worst = {True: 0.0, False: 0.0}
    bad = []
    for g, t in zip(np.asarray(got).reshape(-1), tables):
        want = want_of(t)
        if np.isnan(want):
            ok = np.isnan(g)
        elif want < 1e-280:
            ok = 0.0 <= g < 2e-280
        else:
            err = abs(g - want) / want
            worst[sum(t) >= LF_TABLE_DEFAULT] = max(worst[sum(t) >= LF_TABLE_DEFAULT], err)
            ok = err <= rtol_of(t)
        if not ok:
            bad.append((t, float(g), want))
    print(f"{what}: worst relative error {worst[True]:.2e} beyond the table, {worst[False]:.2e} inside, {len(tables)} values")
    assert not bad, (what, len(bad), bad[:4])
    return worst


def _pair_tables(incl, excl, pairs):
    return [_table(incl, excl, r, i, j) for r in range(incl.shape[0]) for i, j in pairs]


def _natural(s):
    iu, ju = np.triu_indices(s, 1)
    return np.stack([iu, ju], axis=1).astype(np.int32)


def _same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


# ------------------------------------------------------------------------------ Fisher
@gpu
@pytest.mark.parametrize("name", list(LARGE_SETS))
def test_fisher_large_counts_every_entry_point(ctx, name):
    incl, excl = large_arrays(name)
    n, s = incl.shape
    nat, lst = _natural(s), large_pair_list(s)
    tabs = large_tables(name)
    _check(ctx.fisher_tables(np.array(tabs, np.int64)), tabs, f"{name} tables")
    full = ctx.fisher_pairs(incl, excl)
    _check(full, _pair_tables(incl, excl, nat), f"{name} pairs")
    listed = ctx.fisher_pairs(incl, excl, pairs=lst)
    _check(listed, _pair_tables(incl, excl, lst), f"{name} pair list")
    # the _dev forms: the same kernels on the same data, bit for bit; NaN-filled outputs with a guard row
    d_incl, d_excl, d_tab = ctx.to_device(incl), ctx.to_device(excl), ctx.pair_table(s, lst)
    for pairs, host in ((None, full), (d_tab, listed)):
        d_p = ctx.empty((n + 1, host.shape[1]), np.float64).memset(0xFF)
        ctx.fisher_pairs_dev(d_incl, d_excl, d_p, pairs=pairs)
        out = d_p.to_host()
        assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
        assert _same_bits(out[:n], host), (name, "host and _dev forms differ")
    for d in (d_incl, d_excl, d_tab):
        d.free()


@gpu
def test_fisher_small_a_huge_d_under_every_unroll(ctx):
    """fisher.unroll 4, 8, 16, 24 on the small-a / huge-d rows: walks of 8 to 2000 steps end at the support's edge, so a
    lane runs up to unroll - 1 steps past its end on N = 0 (exact inside the count range).  (The pair kernel and
    fisher_two_sided agree to the tolerance, not bit for bit: a lane of the pair kernel steps once on a side without
    support, where fisher_two_sided skips it, and turns on a denominator scaled differently.)"""
    for name in LARGE_SMALL_A:
        incl, excl = large_arrays(name)
        nat = _natural(incl.shape[1])
        tabs = _pair_tables(incl, excl, nat)
        for unroll in (4, 8, 16, 24):
            with ctx.params({"fisher.unroll": unroll}):
                got = ctx.fisher_pairs(incl, excl)
            _check(got, tabs, f"{name} unroll={unroll}")


# ------------------------------------------------------------------------------ chi2
def _chi2_want(t):
    return R.chi2_yates(*t)[0]


@gpu
@pytest.mark.parametrize("name", list(LARGE_SETS))
def test_chi2_large_counts_every_entry_point(ctx, name):
    """1e-9 against the referee on every set; n_bad is the referee's count of tables with a zero expected frequency.
    Row x column products run to 2^71 here ((2^31 + b)(2^31 + 2^40) in the int32 set, beyond 2^53 from the 1e9 set on):
    the kernel forms them in float64, rounded once, and divides by the total -- an expected frequency of an accepted
    table is at least 1 / 2^53, so none underflows to 0 and the bad tables are exactly those with an empty row or column."""
    incl, excl = large_arrays(name)
    n, s = incl.shape
    nat, lst = _natural(s), large_pair_list(s)
    if name == "int32":
        assert max((t[0] + t[1]) * (t[0] + t[2]) for t in _pair_tables(incl, excl, nat)) > 1 << 63
    d_incl, d_excl, d_tab = ctx.to_device(incl), ctx.to_device(excl), ctx.pair_table(s, lst)
    for pairs, d_pairs in ((nat, None), (lst, d_tab)):
        tabs = _pair_tables(incl, excl, pairs)
        want_bad = sum(R.chi2_yates(*t)[1] for t in tabs)
        p, n_bad = ctx.chi2_pairs(incl, excl, pairs=None if d_pairs is None else pairs)
        assert n_bad == want_bad, (name, n_bad, want_bad)
        _check(p, tabs, f"{name} chi2 {'pairs' if d_pairs is None else 'pair list'}", _chi2_want, lambda t: P_RTOL_TIGHT)
        d_p = ctx.empty((n + 1, len(pairs)), np.float64).memset(0xFF)
        d_bad = ctx.empty(1, np.int64).memset(0xFF)
        ctx.chi2_pairs_dev(d_incl, d_excl, d_p, d_bad, pairs=d_pairs)
        out = d_p.to_host()
        assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
        assert _same_bits(out[:n], p) and int(d_bad.to_host()[0]) == want_bad, name
    for d in (d_incl, d_excl, d_tab):
        d.free()


# ------------------------------------------------------------------------------ beyond the count range: refused
BEYOND_RANGE = {
    # (incl, excl) of one junction; walk: only the Fisher entry points refuse it (a d or b c above 2^53)
    "excl 2^53 + 1": ([3, 5, 2], [(1 << 53) + 1, 40, 9], False),
    "excl 2^62": ([3, 5, 2], [1 << 62, 1 << 62, 9], False),
    "excl 2^63 - 1": ([0, 0, 2], [(1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1], False),
    "total 2^53 + 1": ([1, 0, 2], [(1 << 52) - 1, (1 << 52) + 1, 9], False),
    "a d = 60 * 2^52": ([60, 5, 2], [1 << 49, 1 << 52, 9], True),
    "a d = 2^53 + 2": ([2, 1, 0], [7, (1 << 52) + 1, 9], True),
    "int32 max * 2^23": ([(1 << 31) - 1, 4000, 2], [1 << 40, 1 << 23, 9], True),
}


@gpu
@pytest.mark.parametrize("case", list(BEYOND_RANGE))
def test_counts_beyond_the_range_are_refused_with_outputs_untouched(ctx, case):
    """2^53 .. 2^63: (double) of such a count is no longer the count, and a walk product above 2^53 no longer ends at 0
    (the float64 model turns p negative: tests/test_fisher_referee_cpu.py).  The host entry points return SDICE_ERR_ARG
    before any launch; chi2, which does not walk, accepts the tables whose only fault is a product and is held to 1e-9"""
    incl, excl, walk_only = BEYOND_RANGE[case]
    incl, excl = np.array([incl], np.int32), np.array([excl], np.int64)
    s = incl.shape[1]
    lst = large_pair_list(s)
    lib, sentinel = ctx.lib, np.float64(-7.25)

    def fresh(m):
        return np.full(m, sentinel)

    p = fresh(3)
    assert lib.sdice_fisher_pairs(ctx.h, 1, s, _ptr(incl), _ptr(excl), _ptr(p)) == SDICE_ERR_ARG and (p == sentinel).all()
    p = fresh(len(lst))
    assert lib.sdice_fisher_pair_list(ctx.h, 1, s, _ptr(incl), _ptr(excl), len(lst), _ptr(lst), _ptr(p)) == SDICE_ERR_ARG
    assert (p == sentinel).all()
    with pytest.raises(SdiceError, match="2\\^53"):
        ctx.fisher_pairs(incl, excl)
    tabs = np.array(_pair_tables(incl, excl, _natural(s)), np.int64)
    p = fresh(len(tabs))
    assert lib.sdice_fisher_tables(ctx.h, len(tabs), _ptr(tabs), _ptr(p)) == SDICE_ERR_ARG and (p == sentinel).all()
    bad = C.c_int64(-5)
    if walk_only:
        got, n_bad = ctx.chi2_pairs(incl, excl)
        assert n_bad == 0
        _check(got, [tuple(int(v) for v in t) for t in tabs], f"chi2 {case}", _chi2_want, lambda t: P_RTOL_TIGHT)
    else:
        p = fresh(3)
        assert lib.sdice_chi2_pairs(ctx.h, 1, s, _ptr(incl), _ptr(excl), _ptr(p), C.byref(bad)) == SDICE_ERR_ARG
        assert (p == sentinel).all()
        p = fresh(len(lst))
        assert lib.sdice_chi2_pair_list(ctx.h, 1, s, _ptr(incl), _ptr(excl), len(lst), _ptr(lst), _ptr(p),
                                        C.byref(bad)) == SDICE_ERR_ARG and (p == sentinel).all()
    # the context is still usable, and the largest accepted table is accepted
    edge = np.array([[2, 1, (1 << 52) - 2, (1 << 52) - 1]], np.int64)
    _check(ctx.fisher_tables(edge), [tuple(int(v) for v in edge[0])], "total 2^53")
