"""CPU: the host side of `correlate` (Spearman rank correlation of PS with a sample covariate): the referee the GPU tests
lean on against scipy.stats.spearmanr, engine.spearman_order, the covariate file and every refusal of the command (none of
which opens a device), the ABI declarations and the sub-command's registration."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spearman_referee as SP  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_row(rng, k):
    """k kept (covariate, PS) values with ties on both sides and a trend of random strength and sign"""
    x = rng.integers(0, int(rng.integers(2, k + 2)), size=k).astype(np.float64)
    if rng.random() < 0.3:
        x = x + rng.random(k)                                   # an untied covariate
    slope = rng.choice([-1.0, 1.0]) * rng.choice([0.0, 0.3, 1.0, 3.0]) / np.sqrt(k)
    y = np.clip(0.5 + slope * (x - x.mean()) / (x.std() + 1e-9) + 0.25 * rng.standard_normal(k), 0, 1)
    return x, (np.rint(y * 1000) / 1000).astype(np.float32)


def test_referee_agrees_with_scipy_spearmanr():
    """exact integer sums + mpmath against scipy.stats.spearmanr on random tied rows, n' = 3..4096: rho within 1e-13
    absolute, p within 1e-11 relative wherever scipy's p >= 1e-280"""
    from scipy.stats import spearmanr
    rng = np.random.default_rng(99)
    ks = list(range(3, 40)) + [63, 64, 65, 100, 255, 256, 257, 1000, 1023, 1024, 1025, 2500, 4095, 4096]
    worst_rho = worst_p = 0.0
    compared = 0
    for k in ks:
        for _ in range(3):
            x, y = _tied_row(rng, k)
            num, dx, dy = SP.integer_pieces(x, y)
            if dx == 0 or dy == 0:
                continue                                        # scipy: NaN (ConstantInputWarning); the edge rule is tested below
            rho, p, _ = SP.rho_and_p(k, num, dx, dy)
            want = spearmanr(x, y.astype(np.float64))
            worst_rho = max(worst_rho, abs(rho - want.statistic))
            assert abs(rho - want.statistic) <= 1e-13, (k, rho, want.statistic)
            if want.pvalue >= 1e-280:
                err = abs(p - want.pvalue) / want.pvalue
                worst_p = max(worst_p, err)
                assert err <= 1e-11, (k, p, want.pvalue)
                compared += 1
    print(f"worst |rho - scipy| {worst_rho:.3g}, worst relative p difference {worst_p:.3g} over {compared} rows")
    assert compared > 100


def test_referee_rules():
    """the row rules: NaN drop, fewer than 3 kept, the covariate ranked again among the kept, the edge rules, numpy's mean
    and median in list order, -0.0 == +0.0"""
    cols = [4, 0, 2, 1, 3]
    x = [1.0, 2.0, 2.0, 3.0, 5.0]
    row = np.array([0.2, 0.9, 0.3, 0.4, 0.1, 7.0], dtype=np.float32)         # listed values: 0.1 0.2 0.3 0.9 0.4
    ref = SP.row_reference(row, cols, x)
    from scipy.stats import spearmanr
    want = spearmanr(x, row[cols].astype(np.float64))
    assert ref["tested"] == 1 and ref["n_kept"] == 5 and abs(ref["rho"] - want.statistic) < 1e-15
    assert abs(ref["p"] - want.pvalue) < 1e-14 and ref["med"] == np.float32(0.3) and ref["mean"] == np.mean(row[cols])
    row[1] = np.nan                                                          # the largest value goes: 0.1 0.2 0.3 0.4, monotone
    ref = SP.row_reference(row, cols, x)
    assert ref["n_kept"] == 4 and ref["med"] == np.float32(0.25)
    assert 0 < ref["rho"] < 1                                                 # x ties at 2.0, the PS values do not: not +1
    ref = SP.row_reference(row, cols, [1.0, 2.0, 2.5, 3.0, 5.0])
    assert ref["rho"] == 1.0 and ref["p"] == 0.0                              # |rho| = 1: p = 0, here at 4 kept
    row3 = np.array([0.2, np.nan, 0.3, np.nan, 0.1, 0.0], dtype=np.float32)
    ref = SP.row_reference(row3, cols, [1.0, 2.0, 2.5, 3.0, 5.0])
    assert ref["tested"] == 1 and ref["n_kept"] == 3 and ref["rho"] == 1.0 and ref["p"] == 0.0       # ... and at 3
    assert SP.row_reference(row3, cols, [5.0, 3.0, 2.5, 2.0, 1.0])["rho"] == -1.0
    row3[0] = np.nan
    ref = SP.row_reference(row3, cols, x)
    assert ref == dict(tested=0, rho=0.0, p=0.0, n_kept=0, med=np.float32(0), mean=np.float32(0))     # two kept
    const = np.full(6, 0.5, np.float32)
    ref = SP.row_reference(const, cols, x)
    assert (ref["tested"], ref["rho"], ref["p"], ref["n_kept"]) == (1, 0.0, 1.0, 5)                  # constant PS (scipy: NaN)
    ref = SP.row_reference(row, cols, [2.0] * 5)
    assert (ref["tested"], ref["rho"], ref["p"]) == (1, 0.0, 1.0)                                    # constant covariate
    # the covariate is constant among the KEPT only: columns 0 and 2 are NaN, the others share x = 2
    row = np.array([np.nan, 0.3, np.nan, 0.1, 0.2, 0.0], dtype=np.float32)
    ref = SP.row_reference(row, [0, 1, 2, 3, 4], [1.0, 2.0, 3.0, 2.0, 2.0])
    assert (ref["tested"], ref["rho"], ref["p"], ref["n_kept"]) == (1, 0.0, 1.0, 3)
    # signed zeros tie, and their mean and median are +0.0 as numpy's
    z = np.array([-0.0, 0.0, -0.0, 0.5, -0.0], dtype=np.float32)
    ref = SP.row_reference(z, [0, 1, 2, 3, 4], [1.0, 2.0, 3.0, 4.0, 5.0])
    assert SP.integer_pieces([1.0, 2.0, 3.0, 4.0], z[:4])[2] == 4 * (4 * 4 * 3 + 64) - 20 * 20      # ranks 2 2 2 4, doubled: 4 4 4 8
    assert not np.signbit(ref["med"]) and ref["med"] == 0
    ref = SP.row_reference(np.array([-0.0] * 4, np.float32), [0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0])
    assert not np.signbit(ref["mean"]) and not np.signbit(ref["med"]) and ref["p"] == 1.0


def test_spearman_order():
    from splicedice_amd.engine import spearman_order
    cols, xg = spearman_order([7, 3, 9, 1, 4, 0], [2.5, -1.0, 2.5, 0.0, -1.0, 2.5])
    assert cols.dtype == np.int32 and xg.dtype == np.int32
    assert cols.tolist() == [3, 4, 1, 7, 9, 0]                  # by x, ties in the order given
    assert xg.tolist() == [0, 0, 1, 2, 2, 2]
    cols, xg = spearman_order([2, 1, 0], [0.0, -0.0, 1e-300])
    assert cols.tolist() == [2, 1, 0] and xg.tolist() == [0, 0, 1]          # -0.0 == 0.0
    cols, xg = spearman_order([5, 6, 7], [3.0, 3.0, 3.0])
    assert cols.tolist() == [5, 6, 7] and xg.tolist() == [0, 0, 0]
    rng = np.random.default_rng(3)
    x = rng.integers(0, 50, size=400).astype(np.float64)
    c = rng.permutation(400)
    cols, xg = spearman_order(c, x)
    order = np.argsort(x, kind="stable")
    assert np.array_equal(cols, c[order]) and xg[0] == 0 and set(np.diff(xg).tolist()) <= {0, 1}
    assert np.array_equal(np.diff(xg) == 0, np.diff(x[order]) == 0) and xg[-1] == np.unique(x).size - 1
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            spearman_order([0, 1, 2], [1.0, bad, 2.0])
    with pytest.raises(ValueError, match="3 columns but 2"):
        spearman_order([0, 1, 2], [1.0, 2.0])
    with pytest.raises(TypeError):
        spearman_order([0.5, 1, 2], [1.0, 2.0, 3.0])


def test_abi_symbols_present():
    from splicedice_amd import _ffi
    lib = _ffi.load()
    text = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_spearman", "sdice_spearman_dev"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert len(_ffi.SIGNATURES[name]) == 13
        assert f"int {name}(" in text
    assert "spearman.hip" in open(os.path.join(REPO, "splicedice_amd", "csrc", "Makefile")).read()


def test_subcommand_is_registered():
    from splicedice_amd.__main__ import ACCELERATED, build_parser
    assert ACCELERATED["correlate"] == "splicedice_amd.correlate"
    args = build_parser().parse_args(["correlate", "--psiSPLICEDICE", "t", "--covariate", "c", "-o", "out"])
    assert (args.psiSPLICEDICE, args.covariate, args.annotation, args.outputFile) == ("t", "c", "", "out")
    from splicedice_amd import correlate
    assert args.main is correlate.run_with
    args = build_parser().parse_args(["correlate", "--psiSPLICEDICE", "t", "--covariate", "c", "-a", "g.gtf", "--outputFile", "o"])
    assert args.annotation == "g.gtf" and args.outputFile == "o"


# ---------------------------------------------------------------- the covariate file and the refusals
def test_read_covariate(tmp_path):
    from splicedice_amd import correlate
    path = tmp_path / "cov.tsv"
    path.write_text("s1\t3.5\n\ns2 NA\ns3   -2e1  trailing words\n   \ns4\tNaN\ns5\tna\ns6\t0\ns7\tnAn\n")
    names, values = correlate.read_covariate(str(path))
    assert names == ["s1", "s3", "s6"] and values.dtype == np.float64 and values.tolist() == [3.5, -20.0, 0.0]


def _write_table(tmp_path, samples, n=12):
    rng = np.random.default_rng(8)
    table = tmp_path / "in_allPS.tsv"
    with open(table, "w") as f:
        f.write("cluster\t" + "\t".join(samples) + "\n")
        for i in range(n):
            f.write(f"chr3:{100 + 7 * i}-{900 + 7 * i}:+\t" + "\t".join("%.3f" % v for v in rng.random(len(samples))) + "\n")
    return str(table)


@pytest.mark.parametrize("case", ["unparsable value", "infinite value", "negative infinity", "no value", "listed twice",
                                  "listed twice, once as NA", "missing from the header", "twice in the header",
                                  "fewer than 3 usable", "more than 4096"])
def test_refusals_exit_1_before_any_context(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import correlate

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(correlate, "Context", no_context)
    samples = [f"s{j}" for j in range(8)]
    header = list(samples)
    lines = [f"{x}\t{0.5 * j}" for j, x in enumerate(samples[:6])]
    if case == "unparsable value":
        lines[2] = "s2\ttwelve"
        word = "cannot read 'twelve' as a number"
    elif case == "infinite value":
        lines[3] = "s3\tinf"
        word = "'s3' is not finite"
    elif case == "negative infinity":
        lines[3] = "s3\t-Infinity"
        word = "'s3' is not finite"
    elif case == "no value":
        lines[1] = "s1"
        word = "'s1' has no value"
    elif case == "listed twice":
        lines.append("s4\t9")
        word = "'s4' is listed twice"
    elif case == "listed twice, once as NA":
        lines.append("s0\tNA")
        word = "'s0' is listed twice"
    elif case == "missing from the header":
        lines[0] = "nobody\t1"
        word = "'nobody' is missing from the table header"
    elif case == "twice in the header":
        header[7] = "s2"
        word = "'s2' appears 2 times in the table header"
    elif case == "fewer than 3 usable":
        lines = ["s0\t1", "s1\t2", "s2\tNA", "s3\tnan"]
        word = "fewer than 3 samples that have a value (got 2)"
    else:
        header = [f"s{j}" for j in range(4097)]
        lines = [f"{x}\t{j % 97}" for j, x in enumerate(header)]
        word = "4097 samples have a value, at most 4096"
    table = _write_table(tmp_path, header, n=2)
    cov = tmp_path / "cov.tsv"
    cov.write_text("\n".join(lines) + "\n")
    out = tmp_path / "out.tsv"
    args = argparse.Namespace(psiSPLICEDICE=table, covariate=str(cov), annotation="", outputFile=str(out))
    with pytest.raises(SystemExit) as e:
        correlate.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("correlate: ") and word in err and err.count("\n") == 1, err
    assert not out.exists()
