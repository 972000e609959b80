"""CPU: the referee of the large-count pair tests (tests/fisher_referee.py) against scipy, against exact rational
arithmetic and against the two pinned underflow tables; the float64 model of csrc/fisher.hip (tests/fisher_walk_model.py)
against the referee; and the conditions every fixture of tests/test_gpu_pair_large_counts.py must meet before it may go
to a GPU: no near-tie, the step budget, the count range of include/sdice.h."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fisher_referee as R  # noqa: E402
import fisher_walk_model as W  # noqa: E402
from exact_fisher import exact_two_sided as exact_tool  # noqa: E402
from pair_fixtures import (LARGE_MAX_LANE_STEPS, LARGE_MAX_STEPS, LARGE_SETS, LARGE_SMALL_A, LF_TABLE_DEFAULT, PALETTES,  # noqa: E402
                           PaletteRef, chi2_scipy, exact_two_sided, fisher_scipy, in_count_range, large_tables, large_test_tables)


def _small_tables():
    rng = np.random.default_rng(5)
    tabs = [tuple(int(v) for v in rng.integers(0, hi, 4)) for hi in (4, 12, 60, 300) for _ in range(25)]
    tabs += [(k, m - k, m - k, k) for m in (10, 101) for k in (0, 1, m // 3, m // 2, m)]
    return tabs


def test_referee_agrees_with_scipy_below_5e4():
    ref = PaletteRef(["zeros", "ties", "small", "thousands", "tiny"])
    tabs = [tuple(int(v) for v in t) for t in ref.tables if t.sum() < 50_000][::3] + _small_tables()
    assert len(tabs) > 150 and max(sum(t) for t in tabs) > 20_000
    for t in tabs:
        want, (p, nearest) = fisher_scipy(t), R.two_sided(*t)
        if nearest >= 1e-9:                                     # (scipy's 1e-14 slack and the referee's ties agree)
            assert abs(p - want) <= 1e-9 * want, (t, p, want)


def test_referee_is_the_exact_sum_on_small_tables():
    """tools/exact_fisher.py and the rational sum of pair_fixtures: both accept pmf(k) <= pmf(a) (1 + 1e-12), the referee
    ties only -- the same terms where nearest >= 1e-9; the referee's float is the exact sum's float to the last bits"""
    n = 0
    for t in _small_tables() + [(17, 45, 60, 12), (4, 9, 9, 4), (30, 30, 30, 30), (0, 140, 120, 0), (450, 3, 3, 450)]:
        p, nearest = R.two_sided(*t)
        if min(t[0] + t[1], t[2] + t[3], t[0] + t[2], t[1] + t[3]) == 0:
            assert p == 1.0
            continue
        assert nearest >= 1e-9
        for exact in (exact_tool(*t), exact_two_sided(*t)):
            assert abs(p - exact) <= 4e-16 * exact, (t, p, exact)
        n += 1
    assert n > 80


@pytest.mark.parametrize("table,want", [((41976, 5113, 372553, 78120), 6.575064524545e-310),
                                        ((58002, 90233, 44143, 91836), 3.450966061159082e-300)])
def test_referee_on_the_pinned_underflow_tables(table, want):
    """tests/test_gpu_parity.py test_fisher_p_near_underflow_is_the_exact_sum: values from rational arithmetic"""
    assert abs(R.two_sided(*table)[0] - want) <= 1e-12 * want


def test_chi2_referee_agrees_with_scipy():
    ref = PaletteRef(PALETTES)
    n_bad = 0
    for t in ref.tables[::2]:
        t = tuple(int(v) for v in t)
        want, (p, bad) = chi2_scipy(t), R.chi2_yates(*t)
        assert bad == math.isnan(want), t
        n_bad += bad
        if not bad and want >= 1e-300:
            assert abs(p - want) <= 1e-12 * want, (t, p, want)
    assert n_bad > 5


# ------------------------------------------------------------------------------ the fixtures and the model
_MODEL = {}


def _model(t):
    if t not in _MODEL:
        _MODEL[t] = W.fisher(*t, unroll=24)
    return _MODEL[t]


@pytest.mark.parametrize("name", list(LARGE_SETS))
def test_large_fixtures_meet_their_conditions(name):
    for t in large_tables(name):
        p, nearest = R.two_sided(*t)
        assert nearest >= 1e-9, (t, nearest)
        assert in_count_range(*t), t
        assert _model(t).steps <= LARGE_MAX_STEPS, (t, _model(t).steps)
    lane_steps = sum(_model(t).steps for t in large_test_tables(name))
    print(f"{name}: {lane_steps} lane-steps in one GPU test")
    assert lane_steps <= LARGE_MAX_LANE_STEPS, (name, lane_steps)
    assert len(LARGE_SETS[name][0]) >= 8


def test_large_fixtures_reach_what_they_claim():
    tot = lambda t: sum(t)                                                                     # noqa: E731
    b = large_tables("boundary")
    assert {LF_TABLE_DEFAULT - 1, LF_TABLE_DEFAULT, LF_TABLE_DEFAULT + 1} <= {tot(t) for t in b}
    row_max = [max(x[0] + x[1] for x in row) for row in LARGE_SETS["boundary"]]
    second = sorted(x[0] + x[1] for x in LARGE_SETS["boundary"][1])[-2:]
    assert sum(second) < LF_TABLE_DEFAULT and row_max[0] > LF_TABLE_DEFAULT // 2      # a row that is never flagged
    bal = large_tables("balanced")
    assert any(_model(t).steps > 500_000 for t in bal) and any(tot(t) < LF_TABLE_DEFAULT for t in bal)
    assert {10 ** 5, 3 * 10 ** 5, 10 ** 6} <= {t[0] for t in bal}
    for name in LARGE_SMALL_A:
        tabs = large_tables(name)
        huge = [t for t in tabs if tot(t) >= LF_TABLE_DEFAULT]
        assert huge and any(tot(t) < LF_TABLE_DEFAULT for t in tabs), name        # flagged and unflagged pairs in a row
        assert any(t[0] == 0 for t in huge) and any(t[1] == 0 and t[0] > 0 for t in huge), name    # a at either end
        if name != "int32":                                     # equal sample totals: pmf(b) == pmf(a), an exact tie
            assert any(t[0] != t[1] and t[0] + t[2] == t[1] + t[3] for t in huge), name
        assert sum(1e-280 <= R.two_sided(*t)[0] < 1 for t in huge) >= 10, name
        assert max(_model(t).steps for t in tabs) > 20 * min(_model(t).steps for t in huge), name     # uneven lanes
    assert max(tot(t) for t in large_tables("2^52")) == 1 << 53
    assert any(t[0] == (1 << 31) - 1 for t in large_tables("int32"))
    assert any(t[0] * t[3] > 1 << 52 for t in large_tables("int32") + large_tables("2^52"))


@pytest.mark.parametrize("name", list(LARGE_SETS))
def test_model_ratio_sum_is_the_referees(name):
    """the walk alone: 1 + sum of the accepted ratios within 1e-12 of the referee on every fixture table, so whatever
    error a p-value has beyond that is pmf(a)'s; and the model's whole p within the GPU tests' tolerances"""
    worst_sum = worst_p = 0.0
    for t in large_tables(name):
        m, rs, (p, _) = _model(t), R.ratio_sum(*t), R.two_sided(*t)
        worst_sum = max(worst_sum, float(abs(m.total - rs) / rs))
        if p >= 1e-280:
            worst_p = max(worst_p, abs(m.p - p) / p)
    print(f"{name}: ratio sum within {worst_sum:.2e}, p within {worst_p:.2e} of the referee")
    assert worst_sum <= 1e-12
    assert worst_p <= 1e-7


def test_nine_log_factorials_lose_digits_and_the_saddle_form_does_not():
    """pmf(a) alone at the magnitudes of the fixtures: the difference of log-factorials misses 1e-6 from ~1e9 on, the
    saddle-point form stays within 1e-12 everywhere (|log pmf| up to 645 for p >= 1e-280: an ulp of 1.1e-13, and the
    form adds about a dozen terms of that size or less)"""
    import mpmath as mp
    for name, lost in (("1e7", False), ("1e9", True), ("2^40", True), ("2^52", True), ("int32", True)):
        old = new = 0.0
        for t in large_tables(name):
            p, _ = R.two_sided(*t)
            if sum(t) >= LF_TABLE_DEFAULT and p >= 1e-280:
                ft = tuple(float(v) for v in t)
                lp = R.log_pmf(*t)
                old = max(old, float(abs(mp.expm1(W.log_pmf_table(*ft) - lp))))
                new = max(new, float(abs(mp.expm1(W.log_pmf_saddle(*ft) - lp))))
        print(f"{name}: pmf(a) off by {old:.2e} (nine log-factorials), {new:.2e} (saddle-point form)")
        assert new <= 1e-12 and (old > 1e-6) == lost, (name, old, new)


def test_inexact_walk_products_are_why_the_range_ends_at_2_53():
    """a d above 2^53: N no longer ends at exactly 0, the steps past the end of the support are added -- the model's sum
    is far from the referee's (negative, even), so the host entry points refuse such tables"""
    t = (60, 5, 1 << 49, 1 << 52)
    assert not in_count_range(*t)
    m, rs = W.fisher(*t), float(R.ratio_sum(*t))
    assert 1.0 < rs < 1.1 and not abs(m.total - rs) <= 1e-6 * rs
