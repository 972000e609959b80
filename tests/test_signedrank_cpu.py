"""CPU: the host side of compare_sample_sets --paired (Wilcoxon signed-rank test): the referee the GPU tests lean on
against scipy.stats.wilcoxon, the reason for the 3-decimal difference rule, the ABI symbols, the flag and its five
refusals, and the two-rank launcher against the single process.  No device is touched."""
import argparse
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signedrank_referee as SR  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy(d):
    from scipy.stats import wilcoxon
    return wilcoxon(d, zero_method="wilcox", correction=False, alternative="two-sided", method="asymptotic")


def test_referee_agrees_with_scipy_wilcoxon():
    """both kinds of row: 3-decimal values (the differences handed to scipy are the integer thousandths, which is what
    the rule makes of them) and float32 values off the grid (float32 differences); p to 1e-13 relative, |z| to 1e-14,
    and the sign: scipy reports -|z|, the referee is positive when side 1 is larger"""
    rng = np.random.default_rng(20251018)
    worst_p = worst_z = 0.0
    kinds = [0, 0]
    for case in range(400):
        m = int(rng.integers(3, 200))
        if case % 2:
            x, y = ((rng.integers(0, 1001, size=m) / 1000.0).astype(np.float32) for _ in range(2))
            if case % 4 == 1:
                x[: m // 3] = y[: m // 3]                       # zero differences
        else:
            x = (rng.random(m) * 1.7 - 0.3).astype(np.float32)
            y = x + (rng.integers(-6, 7, size=m) * np.float32(0.0625) + np.float32(0.03 * (case % 5))).astype(np.float32)
        d, grid = SR.differences(x, y)
        assert grid == bool(case % 2)
        kinds[grid] += 1
        npairs, w2, tie = SR.integer_pieces(d)
        if npairs == 0:
            continue
        z, p, _ = SR.z_and_p(npairs, w2, tie)
        want = _scipy(d[d != 0].astype(np.float64))
        assert want.statistic == min(w2, npairs * (npairs + 1) - w2) / 2
        assert abs(p - want.pvalue) <= 1e-13 * want.pvalue, (case, p, want.pvalue)
        assert abs(abs(z) + want.zstatistic) <= 1e-14 * max(abs(z), 1.0), (case, z, want.zstatistic)
        assert (z > 0) == (2 * w2 > npairs * (npairs + 1)) or z == 0
        worst_p = max(worst_p, abs(p - want.pvalue) / want.pvalue)
        worst_z = max(worst_z, abs(abs(z) + want.zstatistic))
    assert min(kinds) >= 150
    print("worst difference to scipy.stats.wilcoxon: p relative", worst_p, "|z| absolute", worst_z)


def test_referee_row_rules():
    a, b = [0, 1, 2, 3], [4, 5, 6, 7]
    row = np.array([0.5, 0.25, 0.75, np.nan, 0.5, 0.25, 0.75, 0.1], dtype=np.float32)
    ref = SR.row_reference(row, a, b)               # every kept pair equal: scipy has no answer, the rule is z = 0, p = 1
    assert ref["tested"] == 1 and ref["npairs"] == 0 and ref["z"] == 0.0 and ref["p"] == 1.0 and ref["delta"] == 0
    assert ref["mean1"] == np.mean(row[:3]) and ref["med2"] == np.float32(0.5)
    row[5] = np.nan                                 # two kept pairs
    ref = SR.row_reference(row, a, b)
    assert ref["tested"] == 0 and ref["p"] == 0.0 and ref["mean1"] == 0
    # pair order, not table order, decides which values meet: (0.9, 0.1) (0.2, 0.8) (0.6, 0.5) against (0.9, 0.1) (0.2, 0.5) (0.6, 0.8)
    row = np.array([0.9, 0.2, 0.6, 0.1, 0.8, 0.5], dtype=np.float32)
    r1 = SR.row_reference(row, [0, 1, 2], [3, 4, 5])
    r2 = SR.row_reference(row, [0, 1, 2], [3, 5, 4])
    assert r1["z"] != r2["z"] and r1["med1"] == r2["med1"] and r1["med2"] == r2["med2"]
    # -0.0 against +0.0 is a zero difference on either kind of row
    for extra in (0.25, 0.2500001):
        row = np.array([-0.0, 0.5, 0.7, extra, 0.0, 0.4, 0.9, 0.5], dtype=np.float32)
        ref = SR.row_reference(row, a, b)
        assert ref["npairs"] == 3 and ref["grid"] == (extra == 0.25)


def test_float_differences_of_3_decimal_values_break_ties_by_noise():
    """the documented reason for the grid rule: the pairs of 3-decimal values whose printed difference is 0.001 have many
    distinct float32 (and float64) differences, and 0.3 - 0.2 != 0.2 - 0.1 in float32; the referee ties them"""
    f = np.float32
    assert f(0.3) - f(0.2) != f(0.2) - f(0.1)
    assert 0.3 - 0.2 != 0.2 - 0.1
    k = np.arange(1, 1001)
    hi, lo = (k / 1000.0).astype(np.float32), ((k - 1) / 1000.0).astype(np.float32)
    d32 = np.unique(hi - lo)
    assert d32.size == 12, d32.size                           # 12 distinct float32 values for one printed difference
    assert np.unique(k / 1000.0 - (k - 1) / 1000.0).size > 1  # (float64 is no better)
    d, grid = SR.differences(hi, lo)
    assert grid and (d == 1).all()
    # three pairs, printed differences 0.1, 0.1, -0.4: tied ranks 1.5, 1.5, 3 -> R+ = 3; float32 ranks 2, 1, 3 or 1, 2, 3
    x, y = np.array([0.3, 0.2, 0.5], f), np.array([0.2, 0.1, 0.9], f)
    assert SR.integer_pieces(SR.differences(x, y)[0]) == (3, 6, 6)
    assert SR.integer_pieces((x - y).astype(f)) == (3, 6, 0)
    # a case where the noise changes R+ itself: 0.2 - 0.1 < 0.3 - 0.2 in float32, so with signs - and + the tie matters
    x, y = np.array([0.1, 0.3, 0.5], f), np.array([0.2, 0.2, 0.9], f)
    assert SR.integer_pieces(SR.differences(x, y)[0])[1] == 3 and SR.integer_pieces((x - y).astype(f))[1] == 4


def test_abi_symbols_present():
    from splicedice_amd import _ffi
    lib = _ffi.load()
    text = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_signedrank", "sdice_signedrank_dev"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert len(_ffi.SIGNATURES[name]) == 15
        assert f"int {name}(" in text


# ---------------------------------------------------------------- the flag and its refusals
def _write_inputs(tmp_path, n=60, pairs=5):
    rng = np.random.default_rng(31)
    s = 2 * pairs + 2
    samples = [f"s{j}" for j in range(s)]
    v = rng.integers(0, 1001, size=(n, s)) / 1000.0
    text = np.where(rng.random((n, s)) < 0.1, "nan", np.char.mod("%.3f", v))
    table = tmp_path / "in_allPS.tsv"
    with open(table, "w") as f:
        f.write("cluster\t" + "\t".join(samples) + "\n")
        for i in range(n):
            f.write(f"chr2:{100 + 7 * i}-{900 + 7 * i}:-\t" + "\t".join(text[i]) + "\n")
    order = rng.permutation(pairs)
    g1, g2 = [samples[2 * j + 1] for j in order], [samples[2 * j] for j in order]
    return str(table), samples, g1, g2


def _manifest(tmp_path, name, group):
    p = tmp_path / name
    p.write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    return str(p)


def test_paired_flag_default_and_help():
    from splicedice_amd.__main__ import build_parser
    p = build_parser()
    base = ["compare_sample_sets", "--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "out"]
    assert p.parse_args(base).paired is False and p.parse_args(base + ["--paired"]).paired is True
    from splicedice_amd import compare_sample_sets as css
    sub = argparse.ArgumentParser()
    css.add_parser(sub)
    text = " ".join(sub.format_help().split())
    assert "--paired" in text and "line i of -m1 is paired with line i of -m2" in text and "MANIFEST order" in text


@pytest.mark.parametrize("case", ["lengths differ", "fewer than 3 pairs", "missing from the header", "twice in the header",
                                  "twice in one manifest", "in both manifests", "with -mx"])
def test_paired_refusals_exit_1_before_any_context(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(css, "Context", no_context)
    table, samples, g1, g2 = _write_inputs(tmp_path)
    more, word = None, case
    if case == "lengths differ":
        g2 = g2[:-1]
        word = "differ in length"
    elif case == "fewer than 3 pairs":
        g1, g2 = g1[:2], g2[:2]
        word = "fewer than 3 pairs"
    elif case == "missing from the header":
        g1[1] = "nobody"
        word = "'nobody' is missing from the table header"
    elif case == "twice in the header":
        lines = open(table).read().split("\n")
        lines[0] = lines[0].replace(samples[-1], g2[0])
        open(table, "w").write("\n".join(lines))
        word = f"'{g2[0]}' appears 2 times in the table header"
    elif case == "twice in one manifest":
        g1[3] = g1[0]
        word = f"'{g1[0]}' appears twice in the manifests"
    elif case == "in both manifests":
        g2[2] = g1[4]
        word = f"'{g1[4]}' appears twice in the manifests"
    else:
        more = [_manifest(tmp_path, "m3.tsv", samples[-2:] + samples[:1])]
        word = "cannot be combined with -mx"
    out = tmp_path / "out.tsv"
    args = argparse.Namespace(psiSPLICEDICE=table, manifest1=_manifest(tmp_path, "m1.tsv", g1),
                              manifest2=_manifest(tmp_path, "m2.tsv", g2), moreManifests=more, paired=True, annotation="",
                              outputFile=str(out))
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert "--paired" in err and word in err, err
    assert not out.exists()


# ---------------------------------------------------------------- two ranks against one process
class RefereeEngine:
    """engine double: signedrank is the referee, bh the oracle's (the surface compare() and compare_sharded() use of a
    host engine, as OracleEngine of tests/test_distributed_cpu.py for the rank-sum test)"""

    def __init__(self):
        self.calls = []

    def signedrank(self, ps, a, b):
        self.calls.append(("signedrank", ps.shape[0], tuple(a), tuple(b)))
        ref = SR.table_reference(ps, a, b)
        return {name: ref[name] for name, _ in SR.FIELDS}

    def ranksum(self, ps, g1, g2):
        raise AssertionError("--paired ran the rank-sum test")

    def bh(self, p):
        return O.bh_fdr(p)


def _args(table, m1, m2, out):
    return argparse.Namespace(psiSPLICEDICE=table, manifest1=m1, manifest2=m2, moreManifests=None, paired=True,
                              annotation="", outputFile=out)


def _rank_worker(rank, world, port, table, m1, m2, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from splicedice_amd import compare_sample_sets
    eng = RefereeEngine()
    compare_sample_sets.run_with(_args(table, m1, m2, out), ctx=eng)
    assert [c[1] for c in eng.calls] == [30]                     # this rank tested its half of the 60 rows, once
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_paired_under_two_rank_launcher_equals_single_process(tmp_path):
    """both ranks run --paired on their rows, the packed all-gather carries the eight fields, ONE file appears and it is
    the single process's byte for byte; the pairs reach the engine in MANIFEST order"""
    import torch.multiprocessing as mp
    from splicedice_amd import compare_sample_sets as css
    table, samples, g1, g2 = _write_inputs(tmp_path)
    m1, m2 = _manifest(tmp_path, "m1.tsv", g1), _manifest(tmp_path, "m2.tsv", g2)
    single = str(tmp_path / "single.tsv")
    eng = RefereeEngine()
    css.run_with(_args(table, m1, m2, single), ctx=eng)
    a, b = tuple(samples.index(x) for x in g1), tuple(samples.index(x) for x in g2)
    assert eng.calls == [("signedrank", 60, a, b)] and list(a) != sorted(a) and a[0] > b[0]
    lines = open(single).read().split("\n")
    assert lines[0] == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected" and 40 < len(lines) - 2 <= 60
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    both = str(tmp_path / "both.tsv")
    mpctx = mp.get_context("spawn")
    procs = [mpctx.Process(target=_rank_worker, args=(r, 2, port, table, m1, m2, both)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    assert open(both, "rb").read() == open(single, "rb").read()
    assert not [f for f in os.listdir(tmp_path) if ".part" in f]
