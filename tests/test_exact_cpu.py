"""compare_sample_sets --exact on the CPU: the referee (tests/exact_referee.py) against brute force and scipy's exact
methods, the numbers the flag exists for, the parser, the refusal and the sharded path on an engine double.  No GPU."""
import argparse
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_referee as ER  # noqa: E402
import signedrank_referee as SR  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

TIES = ("none", "some", "heavy")


def _values(rng, count, ties):
    """float32 values: distinct, drawn from about count / 2 + 1 values, or from 2 or 3 values"""
    if ties == "none":
        return rng.permutation(1000)[:count].astype(np.float32) / np.float32(1000)
    pool = count // 2 + 1 if ties == "some" else int(rng.integers(2, 4))
    return (rng.integers(0, pool, size=count) / 8.0).astype(np.float32)


@pytest.mark.parametrize("ties", TIES)
def test_ranksum_recurrence_equals_brute_force(ties):
    """every k-subset by itertools.combinations, 3..7 values per set; count and total as integers"""
    rng = np.random.default_rng(100 + TIES.index(ties))
    for _ in range(100):
        n1, n2 = (int(v) for v in rng.integers(3, 8, size=2))
        v = _values(rng, n1 + n2, ties)
        x, y = v[:n1], v[n1:]
        r = ER.doubled_ranks(v)
        k = min(n1, n2)
        mine = r[:n1] if n1 <= n2 else r[n1:]
        centre = k * (n1 + n2 + 1)
        dist = abs(sum(mine) - centre)
        sums = [sum(c) for c in itertools.combinations(r, k)]
        want = (sum(1 for s in sums if abs(s - centre) >= dist), len(sums))
        assert ER.ranksum_counts(x, y) == want, (x, y)
        # symmetric in which set is taken: the other set's sums are the complements
        other = r[n1:] if n1 <= n2 else r[:n1]
        kk = len(other)
        c2 = kk * (n1 + n2 + 1)
        sums2 = [sum(c) for c in itertools.combinations(r, kk)]
        cnt2 = sum(1 for s in sums2 if abs(s - c2) >= abs(sum(other) - c2))
        assert cnt2 * want[1] == want[0] * len(sums2)


@pytest.mark.parametrize("ties", TIES)
def test_signedrank_recurrence_equals_brute_force(ties):
    """all 2^n' sign patterns, 3..10 pairs, zero differences among them; count and total as integers"""
    rng = np.random.default_rng(200 + TIES.index(ties))
    for _ in range(70):
        m = int(rng.integers(3, 11))
        mag = _values(rng, m, ties) * np.float32(8)
        d = (mag * rng.choice(np.array([-1, 1], np.float32), size=m)).astype(np.float32)
        if ties != "none":
            d[rng.random(m) < 0.15] = 0
        nz = d[d != 0]
        n_prime = int(nz.size)
        if n_prime == 0:
            assert ER.signedrank_counts(d) == (0, 1, 1)
            continue
        r = ER.doubled_ranks(np.abs(nz))
        full = n_prime * (n_prime + 1)
        dist = abs(2 * sum(ri for ri, di in zip(r, nz) if di > 0) - full)
        count = 0
        for signs in itertools.product((0, 1), repeat=n_prime):
            count += abs(2 * sum(ri for ri, b in zip(r, signs) if b) - full) >= dist
        assert ER.signedrank_counts(d) == (n_prime, count, 2 ** n_prime), d


def test_referee_agrees_with_scipy_exact_methods():
    """untied rows: within 1e-14 relative of mannwhitneyu(method="exact") (its last division differs by an ulp); untied,
    zero-free differences: equal to wilcoxon(method="exact")"""
    from scipy import stats
    rng = np.random.default_rng(300)
    worst = 0.0
    for _ in range(150):
        n1, n2 = (int(v) for v in rng.integers(3, 13, size=2))
        v = _values(rng, n1 + n2, "none")
        count, total = ER.ranksum_counts(v[:n1], v[n1:])
        want = stats.mannwhitneyu(v[:n1].astype(np.float64), v[n1:].astype(np.float64), alternative="two-sided",
                                  method="exact").pvalue
        worst = max(worst, abs(count / total - want) / want)
    print(f"rank-sum against scipy exact: worst relative difference {worst:.3g}")
    assert worst <= 1e-14
    for _ in range(150):
        m = int(rng.integers(3, 16))
        d = (_values(rng, m, "none") + np.float32(0.001)) * rng.choice(np.array([-1, 1], np.float32), size=m)
        _, count, total = ER.signedrank_counts(d.astype(np.float32))
        try:
            want = stats.wilcoxon(d.astype(np.float64), alternative="two-sided", method="exact").pvalue
        except TypeError:                       # older scipy: mode= instead of method=
            want = stats.wilcoxon(d.astype(np.float64), alternative="two-sided", mode="exact").pvalue
        assert count / total == want, (d, count / total, want)


def test_the_numbers_the_flag_exists_for():
    """3 v 3 separated: exact p = 2 / C(6, 3) = 0.1 where the normal approximation says 0.0495; 16 v 16 separated:
    count 2 of 601 080 390, sums 272 .. 784; an all-equal row: p = 1"""
    lo, hi = np.array([0.1, 0.2, 0.3], np.float32), np.array([0.7, 0.8, 0.9], np.float32)
    assert ER.ranksum_counts(lo, hi) == (2, 20) and ER.ranksum_counts(hi, lo) == (2, 20) and 2 / 20 == 0.1
    z = (6 - 10.5) / math.sqrt(3 * 3 * 7 / 12)
    assert abs(math.erfc(abs(z) / math.sqrt(2)) - 0.0495) < 1e-4
    v = np.arange(32, dtype=np.float32)
    assert ER.ranksum_counts(v[:16], v[16:]) == (2, 601_080_390)
    table = ER.subset_sum_counts(tuple(range(2, 66, 2)), 16)
    assert min(table) == 272 and max(table) == 784 and sum(table.values()) == math.comb(32, 16) < 2 ** 32
    same = np.full(5, 0.5, np.float32)
    assert ER.ranksum_counts(same, same[:4]) == (math.comb(9, 4), math.comb(9, 4))
    # the row rules: 33 kept values are not eligible, 32 are; +-0 tie, subnormals do not
    row = np.arange(40, dtype=np.float32)
    assert ER.ranksum_row(row, range(16), range(16, 33)) == (False, None) and ER.ranksum_row(row, range(16), range(16, 32))[0]
    assert ER.doubled_ranks(np.array([-0.0, 0.0, 1e-45, -1e-45], np.float32)) == [5, 5, 8, 2]
    # signed-rank: 0.3 - 0.2 ties with 0.2 - 0.1 on a grid row; every pair equal is exact with p = 1
    row = np.array([0.3, 0.2, 0.9, 0.2, 0.1, 0.5], np.float32)
    assert ER.signedrank_row(row, [0, 1, 2], [3, 4, 5]) == (True, 2 / 8)
    assert ER.signedrank_row(np.full(6, 0.25, np.float32), [0, 1, 2], [3, 4, 5]) == (True, 1.0)
    wide = np.concatenate([np.arange(1, 33), np.zeros(32)]).astype(np.float32)
    assert ER.signedrank_row(wide, range(32), range(32, 64)) == (False, None)
    assert ER.signedrank_row(wide, range(31), range(32, 63)) == (True, 2 / 2 ** 31)


# ---------------------------------------------------------------- the command
BASE = ["compare_sample_sets", "--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "out"]


def test_exact_flag_default_and_help():
    from splicedice_amd.__main__ import build_parser
    from splicedice_amd import compare_sample_sets as css
    p = build_parser()
    assert p.parse_args(BASE).exact is False and p.parse_args(BASE + ["--exact"]).exact is True
    both = p.parse_args(BASE + ["--paired", "--exact"])
    assert both.exact is True and both.paired is True
    sub = argparse.ArgumentParser()
    css.add_parser(sub)
    text = " ".join(sub.format_help().split())
    assert "--exact" in text and "keep the asymptotic p-value" in text and "wilcox.test" in text


def _manifest(tmp_path, name, group):
    path = tmp_path / name
    path.write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    return str(path)


@pytest.mark.parametrize("paired", [False, True])
def test_exact_with_mx_exits_1_before_any_context(paired, tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(css, "Context", no_context)
    names = [f"s{j}" for j in range(9)]
    table = tmp_path / "t_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(names) + "\n" + "chr1:1-2:+\t" + "\t".join(["0.500"] * 9) + "\n")
    out = tmp_path / "out.tsv"
    args = argparse.Namespace(psiSPLICEDICE=str(table), manifest1=_manifest(tmp_path, "m1.tsv", names[:3]),
                              manifest2=_manifest(tmp_path, "m2.tsv", names[3:6]),
                              moreManifests=[_manifest(tmp_path, "m3.tsv", names[6:])], paired=paired, exact=True,
                              annotation="", outputFile=str(out))
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--exact" in err and "cannot be combined with -mx" in err, err
    assert not out.exists()


class ExactEngine:
    """engine double with the host surface compare_sharded() uses: the _exact calls answer from the referees, the plain
    calls fail the test"""

    def __init__(self):
        self.calls = []

    def _answer(self, name, ps, c1, c2, paired):
        self.calls.append(name)
        ref = SR.table_reference(ps, c1, c2)         # (the row rules and the float32 fields; its p is replaced below)
        out = {k: ref[k].copy() for k, _ in SR.FIELDS}
        exact, p = ER.table_reference(ps, c1, c2, paired)
        out["p"] = np.where(exact == 1, p, out["p"])
        out["exact"] = exact
        return out

    def ranksum_exact(self, ps, g1, g2):
        return self._answer("ranksum_exact", ps, g1, g2, False)

    def signedrank_exact(self, ps, a, b):
        return self._answer("signedrank_exact", ps, a, b, True)

    def ranksum(self, *a):
        raise AssertionError("--exact ran the asymptotic rank-sum call")

    signedrank = ranksum

    def bh(self, p):
        return O.bh_fdr(p)


@pytest.mark.parametrize("paired", [False, True])
def test_compare_sharded_calls_the_exact_method_and_drops_the_marks(paired):
    from splicedice_amd import compare_sample_sets as css
    from splicedice_amd import mgpu
    rng = np.random.default_rng(7)
    ps = (rng.integers(0, 1001, size=(12, 8)) / 1000.0).astype(np.float32)
    ps[3, :3] = np.nan                                # an untested row
    g1, g2 = np.arange(4, dtype=np.int32), np.arange(4, 8, dtype=np.int32)
    eng = ExactEngine()
    keep, out = css.compare_sharded(ps, g1, g2, eng, mgpu.Launcher(), paired=paired, exact=True)
    assert eng.calls == ["signedrank_exact" if paired else "ranksum_exact"]
    assert "exact" not in out and set(out) == {"p", "med1", "med2", "mean1", "mean2", "delta", "corrected"}
    assert 3 not in keep and keep.size == 11
    _, p = ER.table_reference(ps, g1, g2, paired)
    assert np.array_equal(out["p"], p[keep]) and np.array_equal(out["corrected"], O.bh_fdr(p[keep]))
    # the host path of compare() takes the same call
    eng = ExactEngine()
    keep2, out2 = css.compare(ps, g1, g2, eng, paired=paired, exact=True)
    assert eng.calls == ["signedrank_exact" if paired else "ranksum_exact"] and np.array_equal(keep2, keep)
    assert np.array_equal(out2["p"], out["p"])
