"""compare_sample_sets --strata on the CPU: the referee (tests/strata_referee.py) against scipy and a float64 restatement,
its symmetries, the parser, every refusal on a context that must not be touched, the label helpers, the ABI table.  No GPU."""
import argparse
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strata_referee as VR  # noqa: E402


def _cohort(rng, n1, n2, H, ties=False, nan=0.0):
    """one row over n1 + n2 columns in H random strata, a batch shift per stratum -> (row, g1, g2, strat1, strat2)"""
    s = n1 + n2
    perm = rng.permutation(s)
    g1, g2 = perm[:n1].astype(np.int32), perm[n1:].astype(np.int32)
    strat = rng.integers(0, H, size=s).astype(np.int32)
    v = rng.random(s) * 0.5 + 0.2 * rng.random(H)[strat]
    v[g1] += 0.05
    v = np.rint(v * (20 if ties else 1000)) / (20 if ties else 1000)
    row = v.astype(np.float32)
    row[rng.random(s) < nan] = np.nan
    return row, g1, g2, strat[g1], strat[g2]


def _float64_restatement(row, g1, g2, strat1, strat2):
    """the statistic once more, in plain float64 through scipy.stats.rankdata -> z (None when the row is not tested)"""
    from scipy.stats import rankdata
    x, y = row[g1].astype(np.float64), row[g2].astype(np.float64)
    sd = sv = 0.0
    n1 = n2 = 0
    for h in np.union1d(strat1, strat2):
        a, b = x[strat1 == h], y[strat2 == h]
        a, b = a[~np.isnan(a)], b[~np.isnan(b)]
        if a.size == 0 or b.size == 0:
            continue
        N = a.size + b.size
        r = rankdata(np.concatenate([a, b]))
        _, cnt = np.unique(np.concatenate([a, b]), return_counts=True)
        T = float(((cnt.astype(np.float64)) ** 3 - cnt).sum())
        sd += (r[:a.size].sum() - a.size * (N + 1) / 2.0) / (N + 1)
        sv += a.size * b.size * (N ** 3 - N - T) / (12.0 * N * (N - 1) * (N + 1) ** 2)
        n1 += a.size
        n2 += b.size
    if n1 < 3 or n2 < 3:
        return None
    return sd / np.sqrt(sv) if sv > 0 else 0.0


def test_one_stratum_without_ties_is_scipy_ranksums():
    from scipy.stats import ranksums
    rng = np.random.default_rng(1)
    for n1, n2 in ((3, 3), (7, 12), (40, 33), (200, 150)):
        v = (rng.permutation(1001)[: n1 + n2] / 1000.0).astype(np.float32)
        g1, g2 = np.arange(n1), np.arange(n1, n1 + n2)
        ref = VR.row_reference(v, g1, g2, np.zeros(n1, np.int32), np.zeros(n2, np.int32))
        want = ranksums(v[g1].astype(np.float64), v[g2].astype(np.float64))
        assert ref["tested"] == 1 and ref["grid"]
        assert abs(ref["z"] - want.statistic) <= 1e-13 * abs(want.statistic), (n1, n2, ref["z"], want.statistic)


def test_one_stratum_with_ties_is_mannwhitneyu_without_continuity():
    from scipy.stats import mannwhitneyu, ranksums
    rng = np.random.default_rng(2)
    differs = 0
    for n1, n2 in ((4, 5), (9, 9), (30, 45), (120, 80)):
        v = (rng.integers(0, 12, size=n1 + n2) / 16.0).astype(np.float32)
        g1, g2 = np.arange(n1), np.arange(n1, n1 + n2)
        ref = VR.row_reference(v, g1, g2, np.zeros(n1, np.int32), np.zeros(n2, np.int32))
        x, y = v[g1].astype(np.float64), v[g2].astype(np.float64)
        want = mannwhitneyu(x, y, use_continuity=False, method="asymptotic").pvalue
        assert abs(ref["p"] - want) <= 1e-13 * want, (n1, n2, ref["p"], want)
        differs += abs(ref["p"] - ranksums(x, y).pvalue) > 1e-6 * want        # (ranksums has no tie correction)
    assert differs >= 3


@pytest.mark.parametrize("ties", [False, True])
def test_several_strata_agree_with_the_float64_restatement(ties):
    rng = np.random.default_rng(3 + ties)
    tested = 0
    for _ in range(60):
        n1, n2, H = int(rng.integers(3, 60)), int(rng.integers(3, 60)), int(rng.integers(1, 9))
        row, g1, g2, s1, s2 = _cohort(rng, n1, n2, H, ties=ties, nan=0.05)
        ref = VR.row_reference(row, g1, g2, s1, s2)
        z = _float64_restatement(row, g1, g2, s1, s2)
        assert (z is not None) == bool(ref["tested"])
        if z is not None:
            tested += 1
            assert abs(ref["z"] - z) <= 1e-12 * max(1.0, abs(z)), (ref["z"], z)
    assert tested >= 50


def test_symmetries_of_the_exact_statistic():
    """renumbering the strata leaves the exact z^2 (a Fraction) unchanged; swapping the groups flips the sign of z and
    keeps p; a stratum with samples of one group only changes nothing"""
    rng = np.random.default_rng(5)
    for _ in range(25):
        n1, n2, H = int(rng.integers(4, 40)), int(rng.integers(4, 40)), int(rng.integers(2, 7))
        row, g1, g2, s1, s2 = _cohort(rng, n1, n2, H, ties=bool(rng.integers(0, 2)), nan=0.04)
        ref = VR.row_reference(row, g1, g2, s1, s2)
        perm = rng.permutation(H).astype(np.int32)
        again = VR.row_reference(row, g1, g2, perm[s1], perm[s2])
        assert again["z2"] == ref["z2"] and again["z"] == ref["z"] and again["p"] == ref["p"] and again["tested"] == ref["tested"]
        swapped = VR.row_reference(row, g2, g1, s2, s1)
        assert swapped["z"] == -ref["z"] and swapped["p"] == ref["p"] and swapped["z2"] == ref["z2"]
        # five more columns of group 1 in a stratum of their own: not informative
        wide = np.concatenate([row, rng.random(5).astype(np.float32)])
        g1w = np.concatenate([g1, np.arange(row.size, row.size + 5, dtype=np.int32)])
        s1w = np.concatenate([s1, np.full(5, H, np.int32)])
        more = VR.row_reference(wide, g1w, g2, s1w, s2)
        assert more["z2"] == ref["z2"] and more["z"] == ref["z"] and more["p"] == ref["p"] and more["tested"] == ref["tested"]
        if ref["tested"]:
            assert more["mean1"] != ref["mean1"] or more["med1"] != ref["med1"]      # the descriptive columns do see them


def test_row_rules_of_the_referee():
    f = np.float32
    g1, g2 = np.arange(4), np.arange(4, 8)
    s1, s2 = np.array([0, 0, 1, 1], np.int32), np.array([0, 0, 1, 1], np.int32)
    tied = VR.row_reference(np.array([.5, .5, .25, .25, .5, .5, .25, .25], f), g1, g2, s1, s2)
    assert tied["tested"] == 1 and tied["z"] == 0.0 and tied["p"] == 1.0 and tied["z2"] == Fraction(0)
    # 2 v 3 in the informative strata, plenty kept elsewhere: not tested
    few = VR.row_reference(np.array([.1, .2, .3, .4, .5, .6, .7, .8, .9], f), np.arange(4), np.arange(4, 9),
                           np.array([0, 0, 1, 1], np.int32), np.array([0, 0, 0, 2, 2], np.int32))
    assert few["tested"] == 0 and few["p"] == 0.0
    # the textbook case by hand: strata of 2 v 2 without ties, group 1 on top in both: D_h = 4, d_h = 0.4, V_h = 1/15
    row = np.array([.8, .9, .6, .7, .1, .2, .3, .4], f)
    top = VR.row_reference(row, g1, g2, s1, s2)
    sd, sv, sa, n1, n2 = VR.exact_sums(VR.row_keys(row, g1, g2, s1, s2)[2])
    assert (n1, n2) == (4, 4) and sd == Fraction(4, 5) and sv == Fraction(2, 15) and sa == sd and top["tested"] == 1
    assert top["z2"] == Fraction(24, 5) and top["z"] > 0 and top["cond"] == pytest.approx(top["z"])
    # group 1 on top in one stratum and at the bottom in the other: the deviations cancel, cond stays
    mixed = VR.row_reference(np.array([.8, .9, .3, .4, .1, .2, .6, .7], f), g1, g2, s1, s2)
    assert mixed["z"] == 0.0 and mixed["p"] == 1.0 and mixed["cond"] == pytest.approx(top["cond"])


# ---------------------------------------------------------------- the command
BASE = ["compare_sample_sets", "--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "out"]


def test_strata_flag_default_and_help():
    from splicedice_amd.__main__ import build_parser
    from splicedice_amd import compare_sample_sets as css
    p = build_parser()
    assert p.parse_args(BASE).strata is None and p.parse_args(BASE + ["--strata", "batches.tsv"]).strata == "batches.tsv"
    sub = argparse.ArgumentParser()
    css.add_parser(sub)
    text = " ".join(sub.format_help().split())
    assert "--strata FILE" in text and "tie correction" in text and "mannwhitneyu" in text


def test_abi_table_carries_both_symbols():
    from splicedice_amd import _ffi
    host, dev = _ffi.SIGNATURES["sdice_ranksum_strata"], _ffi.SIGNATURES["sdice_ranksum_strata_dev"]
    assert len(host) == len(dev) == 19 and len(host) == len(_ffi.SIGNATURES["sdice_ranksum"]) + 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdice.h")).read()
    assert "int sdice_ranksum_strata(" in header and "int sdice_ranksum_strata_dev(" in header


def test_strata_ids_number_labels_by_first_appearance():
    from splicedice_amd.engine import strata_ids
    ids, names = strata_ids(["b", "a", "b", "", "a", "centre 3"])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 0, 2, 1, 3] and names == ["b", "a", "", "centre 3"]
    ids, names = strata_ids([])
    assert ids.shape == (0,) and names == []


def test_label_reader_keeps_duplicates_apart(tmp_path, capsys):
    from splicedice_amd import _cli
    path = tmp_path / "batches.tsv"
    path.write_text("s1\tA\ns2\tcentre 3\n\ns1\tB\ns3\tA\textra\n")
    got = _cli.read_labels(str(path), _cli.refusal("x"))
    assert got == {"s1": ["A", "B"], "s2": ["centre 3"], "s3": ["A\textra"]}
    path.write_text("s1\tA\ns2 B\n")
    with pytest.raises(SystemExit) as e:
        _cli.read_labels(str(path), _cli.refusal("compare_sample_sets --strata"))
    assert e.value.code == 1 and "line 2" in capsys.readouterr().err


class Untouchable:
    """a context that fails the test when anything is asked of it"""
    def __getattr__(self, name):
        raise AssertionError(f"the context was touched: {name}")


def _manifest(tmp_path, name, group):
    path = tmp_path / name
    path.write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    return str(path)


NAMES = [f"s{j}" for j in range(140)]


def _args(tmp_path, labels, g1=NAMES[:4], g2=NAMES[4:8], **extra):
    table = tmp_path / "t_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(NAMES) + "\n" + "chr1:1-2:+\t" + "\t".join(["0.500"] * len(NAMES)) + "\n")
    strata = tmp_path / "batches.tsv"
    strata.write_text("".join(f"{a}\t{b}\n" for a, b in labels))
    base = dict(psiSPLICEDICE=str(table), manifest1=_manifest(tmp_path, "m1.tsv", g1), manifest2=_manifest(tmp_path, "m2.tsv", g2),
                moreManifests=None, paired=False, exact=False, strata=str(strata), annotation="",
                outputFile=str(tmp_path / "out.tsv"))
    base.update(extra)
    return argparse.Namespace(**base)


GOOD = [(x, "AB"[j % 2]) for j, x in enumerate(NAMES[:8])]
REFUSALS = {
    "missing sample": (dict(labels=GOOD[:5] + GOOD[6:]), "'s5' has no label"),
    "duplicated sample": (dict(labels=GOOD + [("s2", "A")]), "'s2' has 2 lines"),
    "more than 64 labels": (dict(labels=[(x, f"batch{j}") for j, x in enumerate(NAMES[:130])], g1=NAMES[:65], g2=NAMES[65:130]),
                            "130 distinct labels"),
    "with --paired": (dict(labels=GOOD, paired=True), "cannot be combined with --paired"),
    "with -mx": (dict(labels=GOOD, mx=True), "cannot be combined with -mx"),
    "with --exact": (dict(labels=GOOD, exact=True), "cannot be combined with --exact"),
    "sample in both manifests": (dict(labels=GOOD, g2=NAMES[3:8]), "'s3' is in both manifests"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_1_before_any_engine_call(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(css, "Context", no_context)
    kw, words = REFUSALS[case]
    kw = dict(kw)
    if kw.pop("mx", False):
        kw["moreManifests"] = [_manifest(tmp_path, "m3.tsv", NAMES[8:12])]
    args = _args(tmp_path, **kw)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("compare_sample_sets --strata: ") and words in err, err
    assert not os.path.exists(args.outputFile)


def test_multi_rank_launcher_is_refused(tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css
    from splicedice_amd import mgpu

    class TwoRanks:
        world, rank, local_rank, root = 2, 0, 0, True
    monkeypatch.setattr(mgpu, "launcher", lambda: TwoRanks())
    args = _args(tmp_path, GOOD)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err == css.STRATA_MULTI_RANK_REFUSAL + "\n" and "is not available under the multi-rank launcher" in err
    assert css.MULTI_RANK_REFUSAL.split("(")[0].replace("-mx/--moreManifests", "--strata") == err.split("(")[0]


def test_a_stratum_of_one_set_only_is_accepted(tmp_path):
    """labels that leave a batch with samples of one set only, and samples outside the manifests without a label: the
    column lists and dense ids come out, in table order, numbered by first appearance"""
    from splicedice_amd import _cli
    from splicedice_amd import compare_sample_sets as css
    labels = {"s0": ["x"], "s1": ["y"], "s2": ["x"], "s3": ["only one"], "s4": ["y"], "s5": ["x"], "s6": ["y"], "s7": ["x"]}
    g1_idx, g2_idx, s1, s2, H = css.strata_columns(["s3", "s0", "s1", "s2"], NAMES[4:8], NAMES[:10], labels)
    assert g1_idx.tolist() == [0, 1, 2, 3] and g2_idx.tolist() == [4, 5, 6, 7] and H == 3
    assert s1.tolist() == [0, 1, 0, 2] and s2.tolist() == [1, 0, 1, 0] and s1.dtype == np.int32
    assert _cli.refusal("compare_sample_sets --strata") is not None
