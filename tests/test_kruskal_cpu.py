"""CPU: the host side of the Kruskal-Wallis path of compare_sample_sets (-mx): the exact referee the GPU tests lean on,
the ABI symbols, the flag, the one-set-per-column rule and the multi-rank refusal.  No device is touched."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kruskal_referee as KR  # noqa: E402


def test_referee_agrees_with_scipy_kruskal():
    """exact rational H + chi2.sf against scipy.stats.kruskal on tied (3-decimal) and untied data: p to 1e-9 relative
    (scipy's own H carries the cancellation of the textbook formula, about 3e-9 relative at worst)"""
    from scipy.stats import kruskal
    rng = np.random.default_rng(20240611)
    worst = 0.0
    for case in range(300):
        k = int(rng.integers(2, 9))
        sizes = rng.integers(3, 40, size=k)
        if case % 2:
            groups = [(rng.integers(0, 1001, size=m) / 1000.0).astype(np.float32) for m in sizes]
            keys = [KR.grid_keys(g) for g in groups]
        else:
            groups = [rng.random(m, dtype=np.float32) + np.float32(0.05 * i) for i, m in enumerate(sizes)]
            keys = np.split(KR.dense_keys(np.concatenate(groups)), np.cumsum(sizes)[:-1])
        h = KR.exact_h(keys)
        from scipy.stats import chi2
        p = float(chi2.sf(float(h), k - 1))
        want = kruskal(*[g.astype(np.float64) for g in groups])
        assert abs(p - want.pvalue) <= 1e-9 * want.pvalue, (case, p, want.pvalue)
        assert abs(float(h) - want.statistic) <= 1e-7 * max(want.statistic, 1e-300)
        worst = max(worst, abs(p - want.pvalue) / want.pvalue)
    print("worst relative p difference to scipy.stats.kruskal:", worst)


def test_referee_all_equal_is_none_and_row_rules():
    assert KR.exact_h([np.full(4, 7), np.full(3, 7), np.full(5, 7)]) is None
    row = np.array([0.5, 0.5, 0.5, np.nan, 0.5, 0.5, 0.5, 0.25, 0.5], dtype=np.float32)
    ref = KR.row_reference(row, [[0, 1, 2, 3], [4, 5, 6]], grid=True)
    assert ref["tested"] == 1 and ref["hf"] == 0.0 and ref["p"] == 1.0 and ref["delta"] == 0
    ref = KR.row_reference(row, [[0, 1, 3], [4, 5, 6]], grid=True)          # the first set keeps two values
    assert ref["tested"] == 0


def test_abi_symbols_present():
    from splicedice_amd import _ffi
    lib = _ffi.load()
    for name in ("sdice_kruskal", "sdice_kruskal_dev"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert len(_ffi.SIGNATURES[name]) == 13
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdice.h")).read()
    assert "int sdice_kruskal(" in text and "int sdice_kruskal_dev(" in text


def test_more_manifests_flag_default_and_parse():
    from splicedice_amd.__main__ import build_parser
    p = build_parser()
    base = ["compare_sample_sets", "--psiSPLICEDICE", "p", "-m1", "a", "-m2", "b", "-o", "x"]
    assert p.parse_args(base).moreManifests is None
    assert p.parse_args(base + ["-mx", "c"]).moreManifests == ["c"]
    assert p.parse_args(base + ["--moreManifests", "c", "d", "e"]).moreManifests == ["c", "d", "e"]


def test_duplicate_column_across_sets_raises():
    from splicedice_amd.engine import kruskal_sets
    cols, ptr = kruskal_sets([[0, 1, 2], [5, 4, 3], [6, 7, 8, 9]], s=10)
    assert cols.dtype == np.int32 and cols.tolist() == [0, 1, 2, 5, 4, 3, 6, 7, 8, 9] and ptr.tolist() == [0, 3, 6, 10]
    with pytest.raises(ValueError, match="one set only"):
        kruskal_sets([[0, 1, 2], [3, 4, 5], [6, 7, 2]], s=10)
    with pytest.raises(ValueError, match="one set only"):
        kruskal_sets([[0, 1, 1], [3, 4, 5]])
    with pytest.raises(ValueError, match="outside"):
        kruskal_sets([[0, 1, 2], [3, 4, 10]], s=10)


def _manifest(path, names):
    path.write_text("".join(f"{x}\tp\tm\tA\n" for x in names))
    return str(path)


def test_more_manifests_under_the_launcher_is_refused(tmp_path, monkeypatch, capsys):
    """world > 1: one clear line and exit status 1, before the table is read or a device is opened"""
    import types
    from splicedice_amd import compare_sample_sets as css, mgpu
    # (what mgpu.launcher() hands out under a two-rank launch, without starting a process group here)
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))
    ms = [_manifest(tmp_path / f"m{i}.tsv", [f"s{i}_{j}" for j in range(3)]) for i in range(3)]
    args = argparse.Namespace(psiSPLICEDICE=str(tmp_path / "absent_allPS.tsv"), manifest1=ms[0], manifest2=ms[1],
                              moreManifests=[ms[2]], annotation="", outputFile=str(tmp_path / "x.tsv"))
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.strip() == css.MULTI_RANK_REFUSAL and "\n" not in err.strip() and "moreManifests" in err


def test_more_manifests_too_few_samples_exit(tmp_path, capsys):
    """the `<3 samples` exit covers every manifest, same message and status as the two-set command"""
    from splicedice_amd import compare_sample_sets as css
    ms = [_manifest(tmp_path / f"m{i}.tsv", [f"s{i}_{j}" for j in range(3 if i < 3 else 2)]) for i in range(4)]
    args = argparse.Namespace(psiSPLICEDICE=str(tmp_path / "absent_allPS.tsv"), manifest1=ms[0], manifest2=ms[1],
                              moreManifests=ms[2:], annotation="", outputFile=str(tmp_path / "x.tsv"))
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    assert "Cannot conduct wilcoxon with less than 3 samples in either group. Exit." in capsys.readouterr().err
