"""CPU: the referee of the shift suites against an independent definition, its symmetries and a hand case; the fixture
condition of every table the GPU tests run; the command's refusals and --conf on a stand-in context; the ABI prototypes.

The fixture condition.  rank = max(1, floor(v)), v = M/2 - zq sqrt(M (N + 1) / 12), is evaluated in float64 by the kernels and
at 40 digits by the referee; the two agree as long as v is not within rounding error of an integer.  v is at most 8.4e6
and each of its few float64 operations is good to 2^-53 relative, so the float64 value lies within 1e-8 of the true one;
every (n1', n2', conf) a GPU test meets is required to keep v at least 1e-6 from an integer, a hundred times that."""
import argparse
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shift_fixtures as SF  # noqa: E402
import shift_referee as SR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6
ZQ95 = 1.959963984540054


def _reference(x, y, conf=0.95):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    row = np.concatenate([x, y])
    return SR.row_reference(row, np.arange(x.size), np.arange(x.size, row.size), SR.zq_of(conf))


def _differences(x, y):
    """every difference as an exact Fraction: of the keys (thousandths) on a grid row, of the float64 subtraction's result
    otherwise -> (list, the unit the reported values are in)"""
    x, y = SR.kept(x), SR.kept(y)
    keys = SR.grid_keys(np.concatenate([x, y]))
    if keys is not None:
        return [Fraction(int(a) - int(b), 1000) for a in keys[:x.size] for b in keys[x.size:]]
    return [Fraction(float(np.float64(a) - np.float64(b))) for a in x for b in y]


def _rows(rng):
    """small rows of both flavours, tied and untied, odd and even M"""
    for n1, n2 in ((3, 3), (3, 4), (4, 5), (5, 5), (7, 9), (8, 8), (10, 13), (15, 20), (25, 31)):
        for tied in (False, True):
            for grid in (False, True):
                if grid:
                    pool = rng.permutation(1001)[: (6 if tied else n1 + n2)] / 1000.0
                else:
                    pool = rng.permutation(100003)[: (6 if tied else n1 + n2)] / 7919.0 - 3.0
                pick = rng.integers(0, pool.size, size=n1 + n2) if tied else rng.permutation(n1 + n2)
                v = pool[pick].astype(np.float32)
                yield v[:n1], v[n1:], tied, grid


def test_the_zq_of_95_percent():
    """the standard library's quantile is the documented one to the last place or the one before"""
    assert abs(SR.zq_of(0.95) - ZQ95) <= 4.5e-16


def test_referee_against_the_definition():
    """the shift is a theta with #{d < theta} <= M/2 and #{d > theta} <= M/2 that lies midway between the two middle
    differences; lo and hi are differences, with at most c - 1 strictly outside them and at least c at or outside -- on
    an untied row exactly c - 1 outside"""
    rng = np.random.default_rng(77)
    seen = set()
    for x, y, tied, grid in _rows(rng):
        for conf in (0.5, 0.95):
            ref = _reference(x, y, conf)
            d = _differences(x, y)
            M, c = len(d), ref["rank"]
            assert ref["tested"] == 1 and ref["grid"] == grid and 1 <= c <= M // 2 + 1
            assert c == max(1, int(np.floor(M / 2 - SR.zq_of(conf) * np.sqrt(M * (x.size + y.size + 1) / 12))))
            theta, lo, hi = (Fraction(float(ref[k])) if not grid else Fraction(round(ref[k] * 2000), 2000) for k in ("shift", "lo", "hi"))
            if grid:
                assert all(float(v) == ref[k] for v, k in ((theta, "shift"), (lo, "lo"), (hi, "hi")))
            below, above = sum(v < theta for v in d), sum(v > theta for v in d)
            assert 2 * below <= M and 2 * above <= M, (x, y)
            s = sorted(d)
            mid = (s[(M - 1) // 2] + s[M // 2]) / 2
            assert theta == mid if grid else ref["shift"] == float(mid)       # (off the grid: the one rounding of the sum)
            assert lo in d and hi in d and lo <= theta <= hi
            assert sum(v < lo for v in d) <= c - 1 < sum(v <= lo for v in d)
            assert sum(v > hi for v in d) <= c - 1 < sum(v >= hi for v in d)
            if len(set(d)) == M:
                assert sum(v < lo for v in d) == c - 1 == sum(v > hi for v in d)
            seen.add((tied, grid, M % 2, c == 1))
    assert len({k[:3] for k in seen}) == 8 and {k[3] for k in seen} == {False, True}


def test_the_hand_case():
    """keys 100 200 300 400 v 50 100 150: the 12 differences in thousandths are -50 0 50 50 100 150 150 200 250 250 300 350;
    c = max(1, floor(6 - 1.96 sqrt(8))) = 1"""
    ref = _reference([0.1, 0.2, 0.3, 0.4], [0.05, 0.1, 0.15])
    assert (ref["shift"], ref["lo"], ref["hi"], ref["rank"], ref["grid"]) == (0.15, -0.05, 0.35, 1, True)
    assert SR.rank_and_margin(3, 3, ZQ95)[0] == 1                      # 3 v 3 at 95 %: the clamp
    # floats that print alike: float32(0.3) - float32(0.2) != float32(0.2) - float32(0.1), but the keys' differences tie
    ref = _reference([0.3, 0.2, 0.3], [0.2, 0.1, 0.2])
    assert ref["shift"] == 0.1 and ref["lo"] == 0.0 and ref["hi"] == 0.2
    # off the grid the float64 subtraction is the definition
    x, y = np.array([0.3, 0.7, 0.9001], np.float32), np.array([0.2, 0.1, 0.25], np.float32)
    ref = _reference(x, y)
    d = sorted(float(np.float64(a) - np.float64(b)) for a in x for b in y)
    assert not ref["grid"] and (ref["shift"], ref["lo"], ref["hi"]) == (d[4], d[0], d[8])


def test_row_rules():
    nan = np.nan
    assert _reference([0.1, 0.2, nan, nan], [0.3, 0.4, 0.5]) == dict(tested=0, shift=0.0, lo=0.0, hi=0.0, rank=0, n1=2, n2=3, grid=False)
    ref = _reference([0.1, np.inf, 0.3, 0.4], [0.3, 0.4, 0.5])
    assert ref["tested"] == 1 and ref["rank"] == 1 and all(np.isnan(ref[k]) for k in ("shift", "lo", "hi"))
    ref = _reference([-0.0, 0.0, -0.0], [0.0, -0.0, 0.0, 0.0])
    assert ref["grid"] and all(ref[k] == 0 and not np.signbit(ref[k]) for k in ("shift", "lo", "hi"))
    ref = _reference(np.array([-0.0, 0.0, -0.0], np.float32), np.array([0.0, -0.0, 1e-40], np.float32))
    assert not ref["grid"] and ref["hi"] == 0 and not np.signbit(ref["hi"]) and ref["lo"] < 0
    top = np.finfo(np.float32).max
    ref = _reference([top, top, top], [-top, -top, -top])
    assert ref["shift"] == 2.0 * float(top) and np.isfinite(ref["shift"])


def test_symmetries():
    rng = np.random.default_rng(78)
    for x, y, tied, grid in _rows(rng):
        ref, swapped = _reference(x, y), _reference(y, x)
        assert swapped["rank"] == ref["rank"]
        for a, b in (("shift", "shift"), ("lo", "hi"), ("hi", "lo")):
            want = -ref[b] + 0.0
            assert np.float64(swapped[a]).view(np.uint64) == np.float64(want).view(np.uint64), (a, x, y)
        # a permutation of the columns of either group changes nothing
        again = _reference(x[rng.permutation(x.size)], y[rng.permutation(y.size)])
        assert again == ref
        if grid:
            # a constant number of thousandths added to group 1 moves all three by exactly that
            keys = SR.grid_keys(x)
            k = int(rng.integers(-int(keys.min()), 1001 - int(keys.max())))
            moved = _reference(((keys + k) / 1000.0).astype(np.float32), y)
            assert moved["grid"] and moved["rank"] == ref["rank"]
            for name in ("shift", "lo", "hi"):
                assert round(moved[name] * 2000) == round(ref[name] * 2000) + 2 * k, (name, k)


# ---------------------------------------------------------------- the fixtures
def _kept_counts(ps, g1, g2):
    k1, k2 = (~np.isnan(ps[:, g1])).sum(axis=1), (~np.isnan(ps[:, g2])).sum(axis=1)
    t = (k1 >= 3) & (k2 >= 3)
    return k1, k2, t


def test_fixture_condition_of_every_gpu_case():
    """M/2 - zq sqrt(M (N + 1) / 12) lies at least 1e-6 from an integer at every (n1', n2', conf) a GPU test meets; and the
    cases hold what the suites claim: odd and even M, the clamp c = 1 and ranks above it, untested rows"""
    worst, seen = 1.0, set()
    triples = set()
    for args, conf in SF.cases():
        ps, g1, g2, _ = SF.table(*args)
        k1, k2, t = _kept_counts(ps, g1, g2)
        assert t.any() and (not t.all() or len(args) == 5), args              # (the large tables hold tested rows only)
        triples |= {(int(a), int(b), conf) for a, b in zip(k1[t], k2[t])}
    for n1, n2, conf in sorted(triples):
        c, margin = SR.rank_and_margin(n1, n2, SR.zq_of(conf))
        worst = min(worst, margin)
        assert margin >= MARGIN, (n1, n2, conf, margin)
        seen.add(((n1 * n2) % 2, c == 1))
    print(f"{len(triples)} (n1', n2', conf), the nearest to an integer at {worst:.3g}")
    assert seen == {(0, False), (0, True), (1, False), (1, True)}
    assert {conf for _, _, conf in triples} == set(SF.LEVELS)


def test_the_survey_of_small_counts():
    """every pair of counts 3..199 at 95 %: the worst case of the condition (2.7e-5)"""
    worst = min(SR.rank_and_margin(a, b, ZQ95)[1] for a in range(3, 200) for b in range(a, 200))
    print(f"worst margin {worst:.3g}")
    assert worst >= 2e-5


def test_tables_are_what_they_claim():
    for total in (6, 7, 33, 64, 65, 129):
        n1, n2 = SF.split(total)
        assert n1 >= 3 and n2 >= 3 and n1 + n2 == total
        for flavour in SF.FLAVOURS:
            ps, g1, g2, what = SF.table(n1, n2, flavour)
            assert ps.shape == (len(what), total + 3) and not ps.flags.writeable
            assert np.intersect1d(g1, g2).size == 0 and g1.size == n1 and g2.size == n2
            names = {name for name, _ in what}
            assert names == {k for k, fl in SF.KINDS.items() if flavour == "mixed" or flavour in fl}
            for r, (name, grid) in enumerate(what):
                x, y = SR.kept(ps[r, g1]), SR.kept(ps[r, g2])
                assert (SR.grid_keys(np.concatenate([x, y])) is not None) == grid, (total, flavour, name)
                if name == "NaNs leaving 2 v 3":
                    assert (x.size, y.size) == (2, 3)
                if name == "NaNs leaving 3 v 3":
                    assert (x.size, y.size) == (3, 3)
                if name == "a kept infinity":
                    assert np.isinf(np.concatenate([x, y])).sum() == 1
                if name == "keys 0 and 1000":
                    assert {0.0, 1.0} == set(x.tolist()) == set(y.tolist())
                if name == "signed zeros":
                    assert all(np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all() for v in (x, y))
                if name == "+-FLT_MAX":
                    assert np.abs(x).max() == np.abs(y).max() == np.finfo(np.float32).max
                if name == "outside [0, 1]":
                    assert x.max() > 1 and y.min() < 0
            if flavour == "mixed":
                assert {g for _, g in what} == {False, True}


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
    cells = [f"{0.05 * (j + 1):.3f}" for j in range(len(NAMES))]
    table.write_text("cluster\t" + "\t".join(NAMES) + "\n" + "chr1:1-2:+\t" + "\t".join(cells) + "\n" +
                     "chr1:5-9:+\t" + "\t".join(["nan"] * 3 + cells[3:]) + "\n")
    base = dict(psiSPLICEDICE=str(table), manifest1=_manifest(tmp_path, "m1.tsv", NAMES[:4]),
                manifest2=_manifest(tmp_path, "m2.tsv", NAMES[4:8]), moreManifests=None, paired=False, exact=False,
                strata=None, trend=False, ks=False, shift=True, conf=None, annotation="", outputFile=str(tmp_path / "out.tsv"))
    if extra.pop("mx", False):
        base["moreManifests"] = [_manifest(tmp_path, "m3.tsv", NAMES[8:12])]
    if extra.pop("with_strata", False):
        lab = tmp_path / "batches.tsv"
        lab.write_text("".join(f"{x}\tA\n" for x in NAMES))
        base["strata"] = str(lab)
    base.update(extra)
    return argparse.Namespace(**base)


REFUSALS = {
    "with --paired": (dict(paired=True), "compare_sample_sets --shift: cannot be combined with --paired (the paired estimate is the median of the Walsh averages"),
    "with -mx": (dict(mx=True), "compare_sample_sets --shift: cannot be combined with -mx"),
    "with --trend": (dict(trend=True, mx=True), "compare_sample_sets --shift: cannot be combined with -mx"),
    "with --trend alone": (dict(trend=True), "compare_sample_sets --shift: cannot be combined with --trend"),
    "with --ks": (dict(ks=True), "compare_sample_sets --shift: cannot be combined with --ks"),
    "with --strata": (dict(with_strata=True), "compare_sample_sets --shift: cannot be combined with --strata"),
    "--conf without --shift": (dict(shift=False, conf=0.9), "compare_sample_sets --conf: needs --shift"),
    "--conf 0": (dict(conf=0.0), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 0.0)"),
    "--conf 1": (dict(conf=1.0), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 1.0)"),
    "--conf -0.5": (dict(conf=-0.5), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got -0.5)"),
    "--conf nan": (dict(conf=float("nan")), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got nan)"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_1_before_any_engine_call(case, tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")

    def no_table(*a, **k):
        raise AssertionError("the table was read")
    monkeypatch.setattr(css, "Context", no_context)
    monkeypatch.setattr(css, "read_ps_table", no_table)
    kw, words = REFUSALS[case]
    args = _args(tmp_path, **kw)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith(words) and err.endswith(". Exit.\n"), err
    assert not os.path.exists(args.outputFile)


def test_multi_rank_launcher_is_refused(tmp_path, monkeypatch, capsys):
    from splicedice_amd import compare_sample_sets as css
    from splicedice_amd import mgpu

    class TwoRanks:
        world, rank, local_rank, root = 2, 0, 0, True
    monkeypatch.setattr(mgpu, "launcher", lambda: TwoRanks())
    with pytest.raises(SystemExit) as e:
        css.run_with(_args(tmp_path), ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err == css.BY_FLAG["--shift"].multi_rank + "\n"
    assert err == css.KS_MULTI_RANK_REFUSAL.replace("--ks", "--shift") + "\n"


def test_the_flags_parse():
    from splicedice_amd import compare_sample_sets as css
    p = argparse.ArgumentParser()
    css.add_parser(p)
    base = ["--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "o"]
    a = p.parse_args(base)
    assert a.shift is False and a.conf is None
    a = p.parse_args(base + ["--shift", "--exact"])
    assert a.shift is True and a.exact is True and a.conf is None
    assert p.parse_args(base + ["--shift", "--conf", "0.9"]).conf == 0.9
    p.format_help()                                     # (a stray % in a help text raises here)


class StandIn:
    """a context without a device: the referee's shift beside made-up rank-sum fields; records what it was asked"""

    def __init__(self):
        self.asked = []

    def _plain(self, name, ps, g1, g2):
        self.asked.append(name)
        t = SR.table_reference(ps, g1, g2, ZQ95)["tested"]
        f32 = {k: np.where(t, np.float32(i + 1) / 8, 0).astype(np.float32) for i, k in enumerate(("med1", "med2", "mean1", "mean2", "delta"))}
        return dict(tested=t, p=np.where(t, 0.25, 0.0), z=np.zeros(t.size), exact=t.copy(), **f32)

    def ranksum(self, ps, g1, g2):
        return self._plain("ranksum", ps, g1, g2)

    def ranksum_exact(self, ps, g1, g2):
        return self._plain("ranksum_exact", ps, g1, g2)

    def shift(self, ps, g1, g2, conf=0.95):
        self.asked.append(("shift", conf))
        return SR.table_reference(ps, g1, g2, SR.zq_of(conf))

    def bh(self, p):
        return np.asarray(p) * 2


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("conf", [None, 0.5])
def test_the_command_on_a_stand_in_context(tmp_path, exact, conf):
    """the table gains shift, shift_lo and shift_hi between delta and p-value; --conf reaches the call, 0.95 without it;
    with --exact the exact rank-sum call is the one beside it; without --shift the shift call is not made"""
    from splicedice_amd import compare_sample_sets as css
    ctx = StandIn()
    args = _args(tmp_path, exact=exact, conf=conf)
    css.run_with(args, ctx=ctx)
    level = 0.95 if conf is None else conf
    assert ctx.asked == ["ranksum_exact" if exact else "ranksum", ("shift", level)]
    lines = open(args.outputFile).read().split("\n")
    assert lines[0] == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tshift\tshift_lo\tshift_hi\tp-value\tcorrected"
    # s0..s3 = 0.05 .. 0.20 v s4..s7 = 0.25 .. 0.40: the 16 differences run from -0.35 to -0.05, the median is -0.2
    c = SR.rank_and_margin(4, 4, SR.zq_of(level))[0]
    d = sorted(50 * (i - j) for i in range(1, 5) for j in range(5, 9))
    want = [repr(v / 1000.0) for v in (-200, d[c - 1], d[16 - c])]
    assert lines[1].split("\t") == ["chr1:1-2:+", "0.375", "0.5", "0.125", "0.25", "0.625"] + want + ["0.25", "0.5"]
    assert lines[2:] == [""]                                   # the second row keeps 1 v 4 values: not tested
    plain = StandIn()
    css.run_with(_args(tmp_path, shift=False, exact=exact), ctx=plain)
    assert plain.asked == ["ranksum_exact" if exact else "ranksum"]
    assert open(args.outputFile).read().split("\n")[0] == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected"


# ---------------------------------------------------------------- the ABI
def test_abi_of_the_two_calls():
    from splicedice_amd import _ffi
    from splicedice_amd.engine import SHIFT_FIELDS, Context, shift_quantile
    lib = _ffi.load()
    header = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_shift", "sdice_shift_dev"):
        assert len(_ffi.SIGNATURES[name]) == 14 and hasattr(lib, name)
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and proto.group(1).count(",") == 13, name
        assert "double zq" in proto.group(1)
    assert [f[0] for f in SHIFT_FIELDS] == [name for name, _ in SR.FIELDS] == list(SR.OUTS)
    assert [np.dtype(f[1]) for f in SHIFT_FIELDS] == [np.dtype(dt) for _, dt in SR.FIELDS]
    assert callable(Context.shift) and callable(Context.shift_dev)
    assert shift_quantile(0.95) == SR.zq_of(0.95) and abs(shift_quantile(0.95) - ZQ95) <= 4.5e-16
    for bad in (0.0, 1.0, -1.0, 2.0, float("nan")):
        with pytest.raises(ValueError):
            shift_quantile(bad)
