"""CPU: the host side of `sample_matrix` (sample-by-sample PS correlation over shared junctions): the ABI declarations,
the sub-command's registration, sdice_sample_matrix_finish against the 50-digit referee and its exact rules, and every
refusal of the command (none of which opens a device)."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_matrix_referee as SM  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# corr and rmsd against the 50-digit value: three int -> double roundings, a product, a square root and a division are at
# most 7 roundings of 2^-53 = 7.8e-16 relative
FINISH_BAR = 1e-15


def test_abi_symbols_present():
    from splicedice_amd import _ffi
    lib = _ffi.load()
    text = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name, nargs in (("sdice_sample_gram", 10), ("sdice_sample_gram_dev", 10), ("sdice_sample_matrix_finish", 8)):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert len(_ffi.SIGNATURES[name]) == nargs
        assert f"int {name}(" in text
    make = open(os.path.join(REPO, "splicedice_amd", "csrc", "Makefile")).read()
    assert "gram.hip" in make.split("HOSTSRC")[0] and "gramfinish.cpp" in make.split("HOSTSRC")[1].splitlines()[0]


def test_subcommand_is_registered():
    from splicedice_amd.__main__ import ACCELERATED, build_parser
    assert ACCELERATED["sample_matrix"] == "splicedice_amd.sample_matrix"
    args = build_parser().parse_args(["sample_matrix", "--psiSPLICEDICE", "t", "-o", "pre"])
    assert (args.psiSPLICEDICE, args.samples, args.minShared, args.outputPrefix) == ("t", "", 3, "pre")
    from splicedice_amd import sample_matrix
    assert args.main is sample_matrix.run_with
    args = build_parser().parse_args(["sample_matrix", "--psiSPLICEDICE", "t", "-s", "x.txt", "--minShared", "7", "-o", "p"])
    assert args.samples == "x.txt" and args.minShared == 7
    args = build_parser().parse_args(["sample_matrix", "--psiSPLICEDICE", "t", "--samples", "y", "-o", "p"])
    assert args.samples == "y"


def test_referee_blas_equals_int64_matmul():
    """the float64 BLAS products are the integer sums: against numpy's int64 matmul on a 10 000 x 64 table"""
    rng = np.random.default_rng(5)
    ps = SM.random_table(rng, 10_000, 64)
    got = SM.gram(ps, np.arange(64))
    k, present = SM.keys_of(ps)
    v = present.astype(np.int64)
    assert np.array_equal(got["shared"], v.T @ v) and np.array_equal(got["sum1"], k.T @ v)
    assert np.array_equal(got["sum2"], (k * k).T @ v) and np.array_equal(got["prod"], k.T @ k)
    for bad in (0.0005, 1.001, -0.001, np.inf, np.nextafter(np.float32(0.1), np.float32(1))):
        t = ps[:4].copy()
        t[1, 2] = bad
        with pytest.raises(AssertionError):
            SM.keys_of(t)


def _tables():
    """(name, float32 table): random keys, and near-constant keys around 500 (the worst cancellation in the variances)"""
    rng = np.random.default_rng(17)
    for n, s in ((7, 5), (300, 12), (20_000, 8)):
        yield f"random {n}x{s}", SM.random_table(rng, n, s)
        near = SM.GRID[500 + rng.integers(-1, 2, size=(n, s))].copy()
        near[rng.random((n, s)) < 0.3] = np.nan
        yield f"near-constant {n}x{s}", near


def _rel(got, want):
    both = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got[both] - want[both]) / np.abs(want[both])
    err[got[both] == want[both]] = 0.0
    return float(err.max(initial=0.0))


@pytest.mark.parametrize("name,table", list(_tables()), ids=[t[0] for t in _tables()])
def test_finish_against_the_50_digit_referee(name, table):
    from splicedice_amd.engine import sample_matrix_finish
    g = SM.gram(table, np.arange(table.shape[1]))
    for min_shared in (1, 3):
        corr, rmsd = sample_matrix_finish(g["shared"], g["sum1"], g["sum2"], g["prod"], min_shared)
        want_corr, want_rmsd = SM.finish(g["shared"], g["sum1"], g["sum2"], g["prod"], min_shared)
        e1, e2 = _rel(corr, want_corr), _rel(rmsd, want_rmsd)
        print(f"{name} min_shared {min_shared}: worst relative error corr {e1:.3g}, rmsd {e2:.3g}")
        assert e1 <= FINISH_BAR and e2 <= FINISH_BAR


def test_finish_exact_rules():
    """the diagonal, NaN exactly where the rules say, |corr| <= 1, bit-for-bit symmetry, min_shared 1, 3 and N + 1"""
    from splicedice_amd.engine import sample_matrix_finish
    rng = np.random.default_rng(23)
    ps = SM.random_table(rng, 60, 9, nan_frac=0.5)
    ps[:, 6] = np.float32(0.25)                     # a constant sample: variance 0, rmsd defined
    ps[:, 7] = np.nan
    ps[:2, 7] = SM.GRID[[100, 900]]                 # shares at most 2 rows with anyone
    ps[:, 8] = np.nan                               # shares nothing
    ps[:, 5] = ps[:, 4]                             # a duplicated sample: corr exactly 1, rmsd exactly 0
    g = SM.gram(ps, np.arange(9))
    S = g["shared"]
    va = S * g["sum2"] - g["sum1"] ** 2             # (small table: int64 holds it)
    for min_shared in (1, 3, int(S.max()) + 1):
        corr, rmsd = sample_matrix_finish(S, g["sum1"], g["sum2"], g["prod"], min_shared)
        enough = (S >= min_shared) & (S > 0)
        assert np.array_equal(np.isnan(rmsd), ~enough)
        assert np.array_equal(np.isnan(corr), ~(enough & (va > 0) & (va.T > 0)))
        assert np.array_equal(corr.view(np.int64), corr.T.copy().view(np.int64))
        assert np.array_equal(rmsd.view(np.int64), rmsd.T.copy().view(np.int64))
        ok = ~np.isnan(corr)
        assert np.all(np.abs(corr[ok]) <= 1.0)
        d = np.arange(9)
        assert np.all(corr[d, d][ok[d, d]] == 1.0) and np.all(rmsd[d, d][enough[d, d]] == 0.0)
        if min_shared <= 3:
            assert ok[0, 0] and ok[4, 5] and corr[4, 5] == 1.0 and rmsd[4, 5] == 0.0
            assert np.isnan(corr[6, 6]) and np.isnan(corr[0, 6]) and rmsd[6, 6] == 0.0 and rmsd[0, 6] > 0
            assert np.isnan(rmsd[8, 8]) and np.isnan(rmsd[0, 8])
        if min_shared == 1:
            assert not np.isnan(rmsd[7, 7])
        if min_shared == 3:
            assert np.all(np.isnan(rmsd[7])) and np.all(np.isnan(corr[7]))
        if min_shared > 3:
            assert np.all(np.isnan(corr)) and np.all(np.isnan(rmsd))
    for bad in (0, -1):
        with pytest.raises(Exception, match="min_shared"):
            sample_matrix_finish(S, g["sum1"], g["sum2"], g["prod"], bad)


def test_finish_beyond_int64():
    """N * prod past 2^63: N = 3 * 10^7 rows, keys of about 900 -- the integers supplied directly.  Sample a holds 900 on
    every row but ten at 0, sample b 900 on every row but twenty (ten of them a's) at 1000."""
    from splicedice_amd.engine import sample_matrix_finish
    N = 30_000_000
    kinds = ((N - 20, 900, 900), (10, 0, 1000), (10, 900, 1000))                  # (rows, a's key, b's key)
    assert sum(c for c, _, _ in kinds) == N
    s1a, s2a = sum(c * ka for c, ka, _ in kinds), sum(c * ka * ka for c, ka, _ in kinds)
    s1b, s2b = sum(c * kb for c, _, kb in kinds), sum(c * kb * kb for c, _, kb in kinds)
    pab = sum(c * ka * kb for c, ka, kb in kinds)
    assert N * pab > 2 ** 63 and N * s2a > 2 ** 63
    shared = [[N, N], [N, N]]
    sum1 = [[s1a, s1a], [s1b, s1b]]
    sum2 = [[s2a, s2a], [s2b, s2b]]
    prod = [[s2a, pab], [pab, s2b]]
    corr, rmsd = sample_matrix_finish(shared, sum1, sum2, prod, 3)
    want_corr, want_rmsd = SM.finish(shared, sum1, sum2, prod, 3)
    assert _rel(corr, want_corr) <= FINISH_BAR and _rel(rmsd, want_rmsd) <= FINISH_BAR
    assert corr[0, 0] == 1.0 and corr[1, 1] == 1.0 and corr[0, 1] == corr[1, 0] and -1 < corr[0, 1] < 0


# ---------------------------------------------------------------- the samples file and the refusals
def test_read_samples(tmp_path):
    from splicedice_amd import sample_matrix
    path = tmp_path / "samples.txt"
    path.write_text("s3\tgroupA\n\ns1   trailing words\n   \ns2\n")
    assert sample_matrix.read_samples(str(path)) == ["s3", "s1", "s2"]


def _write_table(tmp_path, samples, n=4):
    rng = np.random.default_rng(8)
    table = tmp_path / "in_allPS.tsv"
    with open(table, "w") as f:
        f.write("cluster\t" + "\t".join(samples) + "\n")
        for i in range(n):
            f.write(f"chr3:{100 + 7 * i}-{900 + 7 * i}:+\t" + "\t".join("%.3f" % v for v in rng.random(len(samples))) + "\n")
    return str(table)


@pytest.mark.parametrize("case", ["missing from the header", "twice in the header", "twice in the header, no -s",
                                  "listed twice", "fewer than 2", "one column, no -s", "more than 4096",
                                  "more than 4096, no -s", "minShared 0", "minShared negative"])
def test_refusals_exit_1_before_any_context(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import sample_matrix

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(sample_matrix, "Context", no_context)
    header = [f"s{j}" for j in range(8)]
    lines = ["s5", "s0", "s2"]
    min_shared = 3
    if case == "missing from the header":
        lines[1] = "nobody"
        word = "'nobody' is missing from the table header"
    elif case == "twice in the header":
        header[7] = "s2"
        word = "'s2' appears 2 times in the table header"
    elif case == "twice in the header, no -s":
        header[7] = "s2"
        lines = None
        word = "'s2' appears 2 times in the table header"
    elif case == "listed twice":
        lines.append("s5\tagain")
        word = "'s5' is listed twice"
    elif case == "fewer than 2":
        lines = ["s4", ""]
        word = "fewer than 2 samples (got 1)"
    elif case == "one column, no -s":
        header, lines = ["only"], None
        word = "fewer than 2 samples (got 1)"
    elif case == "more than 4096":
        header = [f"s{j}" for j in range(4100)]
        lines = header[:4097]
        word = "4097 samples, at most 4096"
    elif case == "more than 4096, no -s":
        header, lines = [f"s{j}" for j in range(4097)], None
        word = "4097 samples, at most 4096"
    elif case == "minShared 0":
        min_shared, word = 0, "--minShared must be at least 1 (got 0)"
    else:
        min_shared, word = -4, "--minShared must be at least 1 (got -4)"
    table = _write_table(tmp_path, header, n=2)
    chosen = ""
    if lines is not None:
        chosen = str(tmp_path / "samples.txt")
        with open(chosen, "w") as f:
            f.write("\n".join(lines) + "\n")
    prefix = str(tmp_path / "out")
    args = argparse.Namespace(psiSPLICEDICE=table, samples=chosen, minShared=min_shared, outputPrefix=prefix)
    with pytest.raises(SystemExit) as e:
        sample_matrix.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("sample_matrix: ") and word in err and err.count("\n") == 1, err
    assert not [x for x in os.listdir(tmp_path) if x.startswith("out")]


def test_multi_rank_launcher_is_refused(tmp_path, monkeypatch, capsys):
    from splicedice_amd import sample_matrix
    monkeypatch.setattr(sample_matrix, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a Context")))
    import types
    from splicedice_amd import mgpu
    # (what mgpu.launcher() hands out under a two-rank launch, without starting a process group here)
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))
    args = argparse.Namespace(psiSPLICEDICE=_write_table(tmp_path, ["a", "b"]), samples="", minShared=3,
                              outputPrefix=str(tmp_path / "out"))
    with pytest.raises(SystemExit) as e:
        sample_matrix.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("sample_matrix: not available under the multi-rank launcher") and err.count("\n") == 1
