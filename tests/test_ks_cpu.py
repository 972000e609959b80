"""The Kolmogorov-Smirnov test without a GPU: the referee (tests/ks_referee.py) against brute force over all subsets,
scipy's ks_2samp(method="exact") and scipy.special.kolmogorov, its symmetries, the hand case of a tie run; the command's
refusals; the ABI; and the conditions the fixtures of the GPU suites (tests/ks_fixtures.py) must meet for the referee
alone, before any GPU is involved."""
import argparse
import itertools
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_fixtures as KF  # noqa: E402
import ks_referee as KR  # noqa: E402
import rank_support as RS  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the referee
def brute_force_p(x, y):
    """P(M* >= M) over every way to deal the pooled values to groups of the two sizes -> Fraction"""
    pooled = np.concatenate([x, y]).astype(np.float32)
    n1, N = len(x), len(x) + len(y)
    M, _ = KR.statistic(x, y)
    hits = total = 0
    for pick in itertools.combinations(range(N), n1):
        mask = np.zeros(N, bool)
        mask[list(pick)] = True
        hits += KR.statistic(pooled[mask], pooled[~mask])[0] >= M
        total += 1
    return Fraction(hits, total)


def _draw(rng, n1, n2, tied):
    if tied:
        return (rng.integers(0, 4, size=k).astype(np.float32) / np.float32(4) for k in (n1, n2))
    perm = rng.permutation(n1 + n2).astype(np.float32)
    return perm[:n1], perm[n1:]


def test_recurrence_equals_brute_force_up_to_12():
    rng = np.random.default_rng(1)
    seen = 0
    for N in range(2, 13):
        for n1 in range(1, N):
            for tied in (False, True):
                x, y = _draw(rng, n1, N - n1, tied)
                M, T = KR.statistic(x, y)
                assert (M, T) == KR.statistic_plain(x, y)
                assert KR.exact_p(M, n1, N - n1, T) == brute_force_p(x, y), (n1, N - n1, tied, x, y)
                seen += 1
    assert seen == 2 * sum(N - 1 for N in range(2, 13))


@pytest.mark.parametrize("n1,n2", [(16, 16), (10, 22), (3, 29), (31, 1), (5, 7), (12, 20)])
def test_untied_rows_equal_scipy_exact(n1, n2):
    from scipy.stats import ks_2samp
    rng = np.random.default_rng(n1)
    checked, shifted = 0, 0
    for draw in range(6):
        # two pieces of one permutation of distinct integers cannot share a value; on odd draws group 1 is moved by
        # more than the range of the values, so the draws cover interleaved and separated samples
        perm = rng.permutation(4 * (n1 + n2)).astype(np.float32)
        x, y = perm[:n1].copy(), perm[n1: n1 + n2]
        if draw % 2:
            x += np.float32(rng.choice([-1, 1]) * 8 * (n1 + n2))
            shifted += 1
        assert np.intersect1d(x, y).size == 0 and np.unique(x).size == n1 and np.unique(y).size == n2
        M, T = KR.statistic(x, y)
        assert T == list(range(1, n1 + n2 + 1))
        want = ks_2samp(x, y, method="exact")
        assert float(Fraction(M, n1 * n2)) == want.statistic, (M, n1, n2, want.statistic)
        p = float(KR.exact_p(M, n1, n2, T))
        assert abs(p - want.pvalue) <= 1e-12 * want.pvalue, (p, want.pvalue)
        assert (M == n1 * n2) == bool(draw % 2)
        checked += 1
    assert checked == 6 and shifted == 3


def test_series_equal_scipy_kolmogorov_and_each_other():
    from scipy.special import kolmogorov
    import mpmath
    for lam in np.concatenate([np.linspace(0.05, 3.0, 60), np.linspace(3.0, 25.3, 40)]):
        lam2 = Fraction(float(lam)) ** 2
        p = KR.kolmogorov_mp(lam2)
        want = kolmogorov(float(lam))
        if want >= 1e-278:
            assert abs(float(p) - want) <= 1e-13 * want, (lam, float(p), want)
    # the two forms are one function: at the library's switch and on both sides of the referee's
    for lam2 in (Fraction(1, 4), Fraction(1, 2), Fraction(1), Fraction(2)):
        a, d = KR.kolmogorov_mp(lam2, "alternating"), KR.kolmogorov_mp(lam2, "dual")
        assert abs(a - d) <= mpmath.mpf(10) ** -KR.DIGITS * a, lam2
    assert KR.asymptotic_p(0, 5, 5) == 1.0 and KR.asymptotic_p(1, 4096, 4096) == 1.0
    assert KR.asymptotic_p(4096 * 4096, 4096, 4096) == 0.0           # 2 exp(-4096): past the float64 range
    assert abs(KR.asymptotic_p(50, 10, 10) - float(kolmogorov(np.sqrt(2500 / 2000)))) < 1e-15


def test_symmetries_of_the_referee():
    rng = np.random.default_rng(3)
    for n1, n2, tied in [(5, 9, True), (7, 7, False), (12, 20, True), (40, 33, True), (64, 65, False)]:
        x, y = _draw(rng, n1, n2, tied)
        s = n1 + n2
        row = np.concatenate([x, y])
        g1, g2 = np.arange(n1), np.arange(n1, s)
        a, b = KR.row_reference(row, g1, g2), KR.row_reference(row, g2, g1)
        assert (a["M"], a["d"], a["p"], a["exact"]) == (b["M"], b["d"], b["p"], b["exact"])
        up = KR.row_reference(np.exp(row.astype(np.float64) / 64.0).astype(np.float32) * np.float32(3) - np.float32(2), g1, g2)
        assert (a["M"], a["d"], a["p"], a["exact"]) == (up["M"], up["d"], up["p"], up["exact"])
        assert a["exact"] == (s <= 32) and a["p_asym"] == KR.asymptotic_p(a["M"], n1, n2)


def test_the_hand_case_of_a_tie_run():
    x, y = np.array([1, 1, 1], np.float32), np.array([1, 1, 1, 2], np.float32)
    M, T = KR.statistic(x, y)
    assert (M, T) == (3, [6, 7]) and Fraction(M, 12) == Fraction(1, 4)
    assert _mid_run_M(x, y) == 12                       # group 1's part of the run first: c1 = 3, c2 = 0
    # every deal of the pooled six 1s and one 2 reaches M: the 2 in the set of four gives M* = 3, in the set of three 4
    assert KR.exact_p(M, 3, 4, T) == brute_force_p(x, y) == Fraction(1)
    ref = KR.row_reference(np.concatenate([x, y]), [0, 1, 2], [3, 4, 5, 6])
    assert ref["d"] == 0.25 and ref["exact"] == 1 and ref["p"] == 1.0


def _mid_run_M(x, y):
    """what an evaluation at every position of the merged order would report, group 1 first inside a tie run"""
    vals = np.concatenate([x, y])
    grp = np.concatenate([np.zeros(len(x), int), np.ones(len(y), int)])
    order = np.lexsort((grp, vals))
    c1 = np.cumsum(grp[order] == 0)
    c2 = np.cumsum(grp[order] == 1)
    return int(np.abs(c1 * len(y) - c2 * len(x)).max())


# ---------------------------------------------------------------- the fixtures of the GPU suites
@pytest.mark.parametrize("total", KF.TOTALS)
def test_mixed_tables_are_what_they_claim(total):
    n1, n2 = KF.split(total)
    assert n1 >= 3 and n2 >= 3 and n1 + n2 == total
    ps, g1, g2, kind = KF.table(n1, n2)
    ref = KF.reference(n1, n2)
    assert np.unique(np.concatenate([g1, g2])).size == total and ps.shape == (2 * len(KF.KINDS), total + 3)
    assert sorted(set(kind.tolist())) == list(range(len(KF.KINDS)))          # each row kind occurs at every total
    t = ref["tested"].astype(bool)
    assert 2 * t.sum() >= t.size                                             # at least half of the rows are tested
    assert (ref["p"][t] >= RS.P_FLOOR).all() and (ref["p_asym"][t] >= RS.P_FLOOR).all()
    RS.check_floor_share(int(t.sum()), int((ref["p"][t] < RS.P_FLOOR).sum()), total)
    assert np.array_equal(ref["exact"], t & (ref["n1"] + ref["n2"] <= 32))
    for r in range(ps.shape[0]):
        name = KF.KINDS[kind[r]]
        x, y = KR.kept(ps[r, g1]), KR.kept(ps[r, g2])
        both = np.concatenate([x, y])
        assert ref["tested"][r] == (x.size >= 3 and y.size >= 3), (r, name)
        if name in ("no NaN", "6 % NaN", "heavy ties"):
            assert bool(np.all(RS.on_grid(both))) == (r < len(KF.KINDS)), (r, name)
        if name == "no NaN":
            assert x.size == n1 and y.size == n2
        if name == "NaNs leaving 3 v 3":
            assert (x.size, y.size) == (3, 3) and ref["exact"][r] == 1
        if name == "NaNs leaving 2 v 3":
            assert (x.size, y.size) == (2, 3) and not ref["tested"][r]
        if name in ("all values equal", "identical samples"):
            assert ref["tested"][r] and ref["M"][r] == 0 and ref["d"][r] == 0.0 and ref["p"][r] == 1.0
        if name == "identical samples":
            assert np.array_equal(np.sort(x), np.sort(y)) and (np.unique(x).size > 1)
        if name == "fully separated":
            assert ref["d"][r] == 1.0 and ref["M"][r] == n1 * n2
        if name == "tie run of both groups at the extreme":
            assert _mid_run_M(x, y) > ref["M"][r] > 0, (r, total)
        if name == "heavy ties":
            assert np.unique(both).size <= 8
        if name == "signed zeros":
            assert (np.signbit(both) & (both == 0)).any() and (~np.signbit(both) & (both == 0)).any()
            assert (x == 0).any() and (y == 0).any()
        if name == "subnormals and FLT_MAX":
            v = np.abs(both)
            assert (v == np.finfo(np.float32).max).sum() >= 2 and (v < np.finfo(np.float32).tiny).sum() >= total - 3
        if name == "+-inf":
            assert np.isinf(x).sum() == 1 and np.isinf(y).sum() == 1 and np.isfinite([ref["med1"][r], ref["med2"][r]]).all()


@pytest.mark.parametrize("n1,n2", [(1024, 1024), (4096, 4096), (4096, 3), (3, 4096)])
def test_large_tables_stay_above_the_floor(n1, n2):
    ref = KF.reference(n1, n2, 2, KF.LARGE_KINDS)
    t = ref["tested"].astype(bool)
    assert t.sum() >= 8 and (ref["p"][t] >= RS.P_FLOOR).all()
    if (n1, n2) == (4096, 4096):
        assert ref["d"][t].max() < 0.39


def test_pair_tables_hold_every_kept_pair():
    want = KF.kept_pairs()
    assert len(want) == sum(N - 5 for N in range(6, 34)) and all(a >= 3 and b >= 3 for a, b in want)
    for n1, n2 in ((30, 30), (40, 40)):
        ps, g1, g2, pairs = KF.pair_table(n1, n2)
        ref = KF.pair_reference(n1, n2)
        assert [tuple(p) for p in pairs[::2]] == want and ps.shape[0] == 2 * len(want)
        assert np.array_equal(ref["n1"], pairs[:, 0]) and np.array_equal(ref["n2"], pairs[:, 1]) and ref["tested"].all()
        assert np.array_equal(ref["exact"], (pairs.sum(axis=1) <= 32).astype(np.uint8)) and (ref["exact"] == 0).sum() == 2 * 28
        assert (ref["p"][ref["tested"] == 1] >= RS.P_FLOOR).all()
        tied = np.array([np.unique(KR.kept(ps[r, np.concatenate([g1, g2])])).size < pairs[r].sum() for r in range(ps.shape[0])])
        assert tied[::2].mean() > 0.8 and not tied[1::2].any()


@pytest.mark.parametrize("n1,n2", [(3, 3), (33, 33)])
def test_blocks_are_mixed(n1, n2):
    ref = KF.block_reference(n1, n2)
    t = ref["tested"].astype(bool)
    assert 0.6 * KF.BLOCK < t.sum() < 0.95 * KF.BLOCK and (ref["p"][t] >= RS.P_FLOOR).all()
    assert np.unique(ref["d"][t]).size > (3 if n1 == 3 else 200)


@pytest.mark.parametrize("n1,n2,steps", KF.LADDERS)
def test_ladders_reach_where_they_should(n1, n2, steps):
    ref = KF.ladder_reference(n1, n2, steps)
    ps, g1, g2 = KF.ladder(n1, n2, steps)
    assert ref["tested"].all() and not ref["exact"].any()
    assert np.all(RS.on_grid(ps[::2])) and not np.any(np.all(RS.on_grid(ps[1::2]), axis=1))
    d, p = ref["d"], ref["p"]
    assert d[0] == 0.0 and p[0] == 1.0 and d[-1] == 1.0 and np.all(np.diff(d) > 0)
    assert (p < RS.P_FLOOR).sum() >= 3 and ((p >= RS.P_FLOOR) & (p < 1e-100)).sum() >= 3 and (p == 0).any()
    assert ((p > 1e-100) & (p < 1e-3)).sum() >= 3 and ((p > 0) & (p < RS.P_FLOOR)).any()


# ---------------------------------------------------------------- the command's refusals
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the context was touched: {name}")


NAMES = [f"s{j}" for j in range(12)]


def _manifest(tmp_path, name, group):
    path = tmp_path / name
    path.write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    return str(path)


def _args(tmp_path, **extra):
    table = tmp_path / "t_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(NAMES) + "\n" + "chr1:1-2:+\t" + "\t".join(["0.500"] * len(NAMES)) + "\n")
    base = dict(psiSPLICEDICE=str(table), manifest1=_manifest(tmp_path, "m1.tsv", NAMES[:4]),
                manifest2=_manifest(tmp_path, "m2.tsv", NAMES[4:8]), moreManifests=None, paired=False, exact=False,
                strata=None, trend=False, ks=True, annotation="", outputFile=str(tmp_path / "out.tsv"))
    if extra.pop("mx", False):
        base["moreManifests"] = [_manifest(tmp_path, "m3.tsv", NAMES[8:12])]
    if extra.pop("with_strata", False):
        lab = tmp_path / "batches.tsv"
        lab.write_text("".join(f"{x}\tA\n" for x in NAMES))
        base["strata"] = str(lab)
    base.update(extra)
    return argparse.Namespace(**base)


REFUSALS = {
    "with --paired": (dict(paired=True), "cannot be combined with --paired"),
    "with -mx": (dict(mx=True), "cannot be combined with -mx"),
    "with --strata": (dict(with_strata=True), "cannot be combined with --strata"),
    "with --trend": (dict(trend=True), "cannot be combined with --trend"),
    "with --trend and -mx": (dict(trend=True, mx=True), "cannot be combined with --trend"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_1_before_any_engine_call(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(css, "Context", no_context)
    kw, words = REFUSALS[case]
    args = _args(tmp_path, **kw)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("compare_sample_sets --ks: ") and words in err, err
    assert not os.path.exists(args.outputFile)


def test_multi_rank_launcher_is_refused(tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css
    from splicedice_amd import mgpu

    class TwoRanks:
        world, rank, local_rank, root = 2, 0, 0, True
    monkeypatch.setattr(mgpu, "launcher", lambda: TwoRanks())
    args = _args(tmp_path)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err == css.KS_MULTI_RANK_REFUSAL + "\n" and "is not available under the multi-rank launcher" in err
    assert css.STRATA_MULTI_RANK_REFUSAL.split("(")[0].replace("--strata", "--ks") == err.split("(")[0]


def test_the_flag_parses_and_goes_with_exact():
    from splicedice_amd import compare_sample_sets as css
    p = argparse.ArgumentParser()
    css.add_parser(p)
    base = ["--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "o"]
    assert p.parse_args(base).ks is False
    a = p.parse_args(base + ["--ks", "--exact"])
    assert a.ks is True and a.exact is True


# ---------------------------------------------------------------- the ABI
def test_abi_of_the_two_calls():
    from splicedice_amd import _ffi
    from splicedice_amd.engine import KS_FIELDS, Context
    lib = _ffi.load()
    header = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_ks", "sdice_ks_dev"):
        assert len(_ffi.SIGNATURES[name]) == 18 and hasattr(lib, name)
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and proto.group(1).count(",") == 17, name
        assert "int32_t want_exact" in proto.group(1)
    assert [f[0] for f in KS_FIELDS] == ["tested", "p", "d", "med1", "med2", "mean1", "mean2", "delta", "exact"]
    assert [f[0] for f in KS_FIELDS] == [name for name, _ in KR.FIELDS] == list(KF.OUTS)
    assert [np.dtype(f[1]) for f in KS_FIELDS] == [np.dtype(dt) for _, dt in KR.FIELDS]
    assert callable(Context.ks) and callable(Context.ks_dev)
