"""CPU: the host side of the Jonckheere-Terpstra path of compare_sample_sets (-mx --trend): the exact referee the GPU tests
lean on (against pair counting, full permutation enumeration and scipy's tie-corrected Mann-Whitney test at k = 2), the ABI
symbols, the flag and every refusal.  No device is touched."""
import argparse
import itertools
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jonckheere_referee as JR  # noqa: E402


def _random_sets(rng, k, lo, hi, levels):
    return [rng.integers(0, levels, size=int(m)) for m in rng.integers(lo, hi + 1, size=k)]


def test_referee_j2_against_pair_counting():
    rng = np.random.default_rng(1801)
    for case in range(200):
        sets = _random_sets(rng, int(rng.integers(2, 9)), 1, 30, (3, 20, 1001)[case % 3])
        pc = JR.exact_pieces(sets)
        assert pc["J2"] == JR.brute_j2(sets), case
        sizes = [g.size for g in sets]
        assert pc["M2"] == sum(sizes[i] * sizes[j] for i in range(len(sets)) for j in range(i + 1, len(sets)))
        assert pc["N"] == sum(sizes) and pc["num"] >= 0


@pytest.mark.parametrize("sizes", [(3, 4), (4, 4), (2, 3, 3), (3, 2, 2), (1, 3, 3), (3, 3, 2)])
def test_referee_mean_and_variance_against_full_enumeration(sizes):
    """every permutation of a tied sample over the sets: the mean of J2 is M2 and the variance of J is the formula's
    rational value, so the formula is the exact conditional variance given the ties"""
    rng = np.random.default_rng(sum(sizes) * 100 + len(sizes))
    N = sum(sizes)
    perms = np.array(list(itertools.permutations(range(N))))
    cuts = np.cumsum((0,) + sizes)
    for levels in (2, 3, 5, 50):
        vals = rng.integers(0, levels, size=N)
        arranged = vals[perms]
        j2 = np.zeros(perms.shape[0], np.int64)
        for i in range(len(sizes)):
            for j in range(i + 1, len(sizes)):
                x = arranged[:, cuts[i]: cuts[i + 1], None]
                y = arranged[:, None, cuts[j]: cuts[j + 1]]
                j2 += 2 * (x < y).sum(axis=(1, 2)) + (x == y).sum(axis=(1, 2))
        pc = JR.exact_pieces(np.split(vals, cuts[1:-1]))
        assert int(j2.sum()) == pc["M2"] * perms.shape[0]
        var_j = Fraction(int(((j2 - pc["M2"]) ** 2).sum()), 4 * perms.shape[0])
        assert var_j == JR.variance(pc), (sizes, levels, vals.tolist())
        assert (pc["num"] == 0) == (np.unique(vals).size == 1)


def test_referee_two_sets_equal_scipy_mannwhitneyu():
    """k = 2: p is scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic") on tied and untied samples"""
    from scipy.stats import mannwhitneyu
    rng = np.random.default_rng(1802)
    worst = 0.0
    for case in range(200):
        a, b = _random_sets(rng, 2, 3, 40, (4, 1001, 10 ** 6)[case % 3])
        b = b + int(rng.integers(0, 3))
        if np.unique(np.concatenate([a, b])).size == 1:
            continue
        z, p = JR.z_and_p(JR.exact_pieces([a, b]))
        want = mannwhitneyu(a.astype(np.float64), b.astype(np.float64), use_continuity=False, method="asymptotic")
        worst = max(worst, abs(float(p) - want.pvalue) / want.pvalue)
        assert (float(z) > 0) == (want.statistic < a.size * b.size / 2) or float(z) == 0     # U of the first sample
    print("worst relative p difference to scipy mannwhitneyu:", worst)
    assert worst <= 1e-12


def test_referee_reversal_symmetry():
    """the sets in reversed order: -z, the same p, and J -> sum n_i n_j - J"""
    rng = np.random.default_rng(1803)
    for case in range(100):
        sets = _random_sets(rng, int(rng.integers(2, 7)), 3, 20, (5, 1001)[case % 2])
        a, b = JR.exact_pieces(sets), JR.exact_pieces(sets[::-1])
        assert a["num"] == b["num"] and a["M2"] == b["M2"] and a["J2"] + b["J2"] == 2 * a["M2"]
        (za, pa), (zb, pb) = JR.z_and_p(a), JR.z_and_p(b)
        assert float(za) == -float(zb) and float(pa) == float(pb)


def test_referee_all_equal_row_and_row_rules():
    pc = JR.exact_pieces([np.full(4, 7), np.full(3, 7), np.full(5, 7)])
    assert pc["num"] == 0 and pc["J2"] == pc["M2"]
    assert [float(x) for x in JR.z_and_p(pc)] == [0.0, 1.0]
    row = np.array([0.5, 0.5, 0.5, np.nan, 0.5, 0.5, 0.5, 0.25, 0.5], dtype=np.float32)
    ref = JR.row_reference(row, [[0, 1, 2, 3], [4, 5, 6]], grid=True)
    assert ref["tested"] == 1 and ref["z"] == 0.0 and ref["p"] == 1.0 and ref["num"] == 0 and ref["j"] == 4.5
    ref = JR.row_reference(row, [[0, 1, 3], [4, 5, 6]], grid=True)          # the first set keeps two values
    assert ref["tested"] == 0 and ref["z"] == 0.0 and ref["p"] == 0.0 and ref["j"] == 0.0


def test_referee_three_sets_of_three_in_perfect_order():
    """z = 3 exactly, p = 0.0027 (the permutation value is 2 / 1680: the test is asymptotic)"""
    row = np.arange(9, dtype=np.float32) / np.float32(10)
    sets = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    ref = JR.row_reference(row, sets, grid=True)
    assert ref["z"] == 3.0 and ref["j"] == 27.0 and abs(ref["p"] - 0.0026997960632601866) < 1e-17
    assert JR.variance(JR.exact_pieces([np.arange(3), np.arange(3, 6), np.arange(6, 9)])) == Fraction(81, 4)
    assert JR.row_reference(row, sets[::-1], grid=True)["z"] == -3.0


def test_abi_symbols_present():
    from splicedice_amd import _ffi
    lib = _ffi.load()
    for name in ("sdice_jonckheere", "sdice_jonckheere_dev"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert len(_ffi.SIGNATURES[name]) == 14
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdice.h")).read()
    assert "int sdice_jonckheere(" in text and "int sdice_jonckheere_dev(" in text


def test_engine_field_table():
    from splicedice_amd import engine
    assert [f[0] for f in engine.JONCKHEERE_FIELDS] == ["tested", "p", "z", "j", "med", "mean", "delta"]
    shapes = engine.field_shapes(engine.JONCKHEERE_FIELDS, 5, 3)
    assert shapes["med"] == ((3, 5), np.float32) and shapes["j"] == (5, np.float64)
    assert hasattr(engine.Context, "jonckheere") and hasattr(engine.Context, "jonckheere_dev")


def test_trend_flag_default_and_parse():
    from splicedice_amd.__main__ import build_parser
    p = build_parser()
    base = ["compare_sample_sets", "--psiSPLICEDICE", "p", "-m1", "a", "-m2", "b", "-o", "x"]
    assert p.parse_args(base).trend is False
    got = p.parse_args(base + ["-mx", "c", "d", "--trend"])
    assert got.trend is True and got.moreManifests == ["c", "d"]
    help_text = " ".join(p.format_help().split()) + " ".join(
        a.help for sp in p._subparsers._group_actions for a in sp.choices["compare_sample_sets"]._actions if a.dest == "trend")
    for word in ("ORDERED", "in the order given", "z > 0", "asymptotic only", "not part of the reference"):
        assert word in " ".join(help_text.split()), word


def _manifest(path, names):
    path.write_text("".join(f"{x}\tp\tm\tA\n" for x in names))
    return str(path)


def _args(tmp_path, n_sets, **flags):
    ms = [_manifest(tmp_path / f"m{i}.tsv", [f"s{i}_{j}" for j in range(3)]) for i in range(n_sets)]
    return argparse.Namespace(psiSPLICEDICE=str(tmp_path / "absent_allPS.tsv"), manifest1=ms[0], manifest2=ms[1],
                              moreManifests=ms[2:] or None, annotation="", outputFile=str(tmp_path / "x.tsv"), trend=True,
                              **flags)


def _refused(args, capsys, monkeypatch):
    """runs the command with every way to a device closed -> the single stderr line"""
    from splicedice_amd import compare_sample_sets as css

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(css, "Context", no_device)
    monkeypatch.setattr(css, "read_ps_table", no_device)
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.endswith("\n") and "\n" not in err.strip() and err.strip()
    return err.strip()


def test_trend_without_more_manifests_is_refused(tmp_path, capsys, monkeypatch):
    err = _refused(_args(tmp_path, 2), capsys, monkeypatch)
    assert err.startswith("compare_sample_sets --trend: needs -mx/--moreManifests") and "rank-sum" in err


@pytest.mark.parametrize("flag, value, word", [("paired", True, "--paired"), ("exact", True, "--exact"),
                                               ("strata", "labels.tsv", "--strata")])
def test_trend_with_another_test_is_refused(tmp_path, capsys, monkeypatch, flag, value, word):
    err = _refused(_args(tmp_path, 3, **{flag: value}), capsys, monkeypatch)
    assert err.startswith("compare_sample_sets --trend: cannot be combined with " + word), err


def test_trend_under_the_launcher_is_refused(tmp_path, capsys, monkeypatch):
    from splicedice_amd import compare_sample_sets as css, mgpu
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))
    err = _refused(_args(tmp_path, 3), capsys, monkeypatch)
    assert err == css.TREND_MULTI_RANK_REFUSAL and "--trend" in err and css.TREND_MULTI_RANK_REFUSAL != css.MULTI_RANK_REFUSAL


def test_trend_too_few_samples_exit(tmp_path, capsys):
    """the `<3 samples` exit stays as it is"""
    from splicedice_amd import compare_sample_sets as css
    args = _args(tmp_path, 3)
    _manifest(tmp_path / "m2.tsv", ["a", "b"])
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    assert "Cannot conduct wilcoxon with less than 3 samples in either group. Exit." in capsys.readouterr().err
