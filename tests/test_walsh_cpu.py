"""CPU: the referee of the paired-shift suites against an independent definition, its symmetries and hand cases; the levels
and the fixture condition of every table the GPU tests run; the command's flag, refusals and --conf on a stand-in context;
the ABI prototypes.

The fixture condition.  rank = max(1, floor(v)), v = M/2 - zq sqrt(m'(m'+1)(2m'+1)/24), is evaluated in float64 by the kernels
and at 40 digits by the referee; the two agree as long as v is not within rounding error of an integer.  v is at most 4.2e6
and each of its few float64 operations is good to 2^-53 relative, so the float64 value lies within 1e-8 of the true one;
every m' = 3..4096 at every level of walsh_fixtures.LEVELS keeps v at least 1e-6 from an integer, a hundred times that."""
import argparse
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walsh_fixtures as WF  # noqa: E402
import walsh_referee as WR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6
ZQ95 = 1.959963984540054
F64 = ("shift", "lo", "hi")


def _reference(x, y, conf=0.95):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    row = np.concatenate([x, y])
    return WR.row_reference(row, np.arange(x.size), np.arange(x.size, row.size), WR.zq_of(conf))


def _averages(x, y):
    """every Walsh average as an exact Fraction: of the keys (thousandths) on a grid row, of the float64 addition's result
    otherwise -> list"""
    x, y = WR.kept_pairs(np.concatenate([x, y]), np.arange(len(x)), np.arange(len(x), 2 * len(x)))
    keys = WR.grid_keys(np.concatenate([x, y]))
    m = x.size
    if keys is not None:
        d = [int(p) - int(q) for p, q in zip(keys[:m], keys[m:])]
        return [Fraction(d[i] + d[j], 2000) for i in range(m) for j in range(i, m)]
    d = (x - y).astype(np.float64)
    return [Fraction(float(d[i] + d[j])) / 2 for i in range(m) for j in range(i, m)]


def _rows(rng):
    """small rows of both flavours, tied and untied, with and without zero differences, odd and even M"""
    for m in (3, 4, 5, 6, 7, 8, 9, 13, 20, 31):
        for tied in (False, True):
            for grid in (False, True):
                pool = (rng.permutation(1001)[: (5 if tied else 2 * m)] / 1000.0 if grid
                        else rng.permutation(100003)[: (5 if tied else 2 * m)] / 7919.0 - 3.0)
                pick = rng.integers(0, pool.size, size=2 * m) if tied else rng.permutation(2 * m)
                v = pool[pick].astype(np.float32)
                x, y = v[:m].copy(), v[m:].copy()
                if tied:
                    x[0] = y[0]                            # a zero difference
                yield x, y, tied, grid


def test_the_zq_of_95_percent():
    assert abs(WR.zq_of(0.95) - ZQ95) <= 4.5e-16


def test_referee_against_the_definition():
    """the shift is a theta with #{w < theta} <= M/2 and #{w > theta} <= M/2 that lies midway between the two middle
    averages; lo and hi are averages, with at most c - 1 strictly outside them and at least c at or outside -- on a row
    without tied averages exactly c - 1 outside"""
    rng = np.random.default_rng(91)
    seen = set()
    for x, y, tied, grid in _rows(rng):
        for conf in (0.5, 0.95):
            ref = _reference(x, y, conf)
            w = _averages(x, y)
            m, M, c = x.size, len(w), ref["rank"]
            assert M == m * (m + 1) // 2 and ref["m"] == m          # zero differences are kept
            assert ref["tested"] == 1 and ref["grid"] == grid and 1 <= c <= M // 2 + 1
            assert c == max(1, int(np.floor(M / 2 - WR.zq_of(conf) * np.sqrt(m * (m + 1) * (2 * m + 1) / 24))))
            if grid:
                theta, lo, hi = (Fraction(round(ref[k] * 4000), 4000) for k in F64)
                assert all(float(v) == ref[k] for v, k in zip((theta, lo, hi), F64))
            else:
                theta, lo, hi = (Fraction(float(ref[k])) for k in F64)
            below, above = sum(v < theta for v in w), sum(v > theta for v in w)
            assert 2 * below <= M and 2 * above <= M, (x, y)
            s = sorted(w)
            mid = (s[(M - 1) // 2] + s[M // 2]) / 2
            assert theta == mid if grid else ref["shift"] == float(mid)       # (off the grid: the one rounding of the mean)
            assert lo in w and hi in w and lo <= theta <= hi
            assert sum(v < lo for v in w) <= c - 1 < sum(v <= lo for v in w)
            assert sum(v > hi for v in w) <= c - 1 < sum(v >= hi for v in w)
            if len(set(w)) == M:
                assert sum(v < lo for v in w) == c - 1 == sum(v > hi for v in w)
            seen.add((tied, grid, M % 2, c == 1))
    assert len({k[:3] for k in seen}) == 8 and {k[3] for k in seen} == {False, True}


def test_the_hand_cases():
    """3 pairs, keys 300 500 900 v 200 100 400: d = 100 400 500, the 6 sums 200 500 600 800 900 1000, the averages 0.1 0.25 0.3
    0.4 0.45 0.5; the median is (600 + 800) / 4000 = 0.35, c = 1 at 95 %, so lo = 0.1 and hi = 0.5.
    4 pairs, keys 100 200 400 500 v 200 200 200 200: d = -100 0 200 300 with its ZERO KEPT, the 10 sums
    -200 -100 0 100 200 200 300 400 500 600; the median is (200 + 200) / 4000 = 0.1, lo = -0.1, hi = 0.3 at 95 % (c = 1); at
    50 % c = floor(5 - 0.6745 sqrt 7.5) = 3, lo = 0 / 2000 and hi = 400 / 2000.  Without the zero the 6 sums would be -200 100
    200 400 500 600 and the median 0.15."""
    ref = _reference([0.3, 0.5, 0.9], [0.2, 0.1, 0.4])
    assert (ref["shift"], ref["lo"], ref["hi"], ref["rank"], ref["grid"], ref["m"]) == (0.35, 0.1, 0.5, 1, True, 3)
    ref = _reference([0.1, 0.2, 0.4, 0.5], [0.2, 0.2, 0.2, 0.2])
    assert (ref["shift"], ref["lo"], ref["hi"], ref["rank"], ref["grid"], ref["m"]) == (0.1, -0.1, 0.3, 1, True, 4)
    ref = _reference([0.1, 0.2, 0.4, 0.5], [0.2, 0.2, 0.2, 0.2], conf=0.5)
    assert (ref["shift"], ref["lo"], ref["hi"], ref["rank"]) == (0.1, 0.0, 0.2, 3)
    assert _reference([0.1, 0.4, 0.5], [0.2, 0.2, 0.2])["shift"] == 0.15
    # floats that print alike: float32(0.3) - float32(0.2) != float32(0.2) - float32(0.1), but the keys' differences tie
    ref = _reference([0.3, 0.2, 0.3], [0.2, 0.1, 0.2])
    assert ref["shift"] == ref["lo"] == ref["hi"] == 0.1
    # off the grid the float32 differences and the float64 sums are the definition
    x, y = np.array([0.3, 0.7, 0.9001], np.float32), np.array([0.2, 0.1, 0.25], np.float32)
    ref = _reference(x, y)
    d = (x - y).astype(np.float64)
    s = sorted(float(d[i] + d[j]) for i in range(3) for j in range(i, 3))
    assert not ref["grid"] and (ref["shift"], ref["lo"], ref["hi"]) == (0.5 * (0.5 * s[2] + 0.5 * s[3]), 0.5 * s[0], 0.5 * s[5])


def test_row_rules():
    nan = np.nan
    assert _reference([0.1, 0.2, nan, 0.3], [0.3, nan, 0.5, nan]) == dict(tested=0, shift=0.0, lo=0.0, hi=0.0, rank=0, m=1, grid=False)
    ref = _reference([0.1, nan, 0.3, 0.4, 0.7], [0.3, 0.4, 0.5, nan, 0.6])
    assert ref["tested"] == 1 and ref["m"] == 3
    # zeros kept: a row of all-zero differences is tested and gives (0, 0, 0), all +0.0
    for x in ([0.25, 0.5, 0.75, 0.1], [0.1234567, -3.5, 7.25], [-0.0, 0.0, -0.0, 0.0]):
        y = [-v for v in x] if x[0] == 0 else x
        ref = _reference(x, y)
        assert ref["tested"] == 1 and all(ref[k] == 0 and not np.signbit(ref[k]) for k in F64), x
    ref = _reference([0.1, np.inf, 0.3, 0.4], [0.3, 0.4, 0.5, 0.2])
    assert ref["tested"] == 1 and ref["rank"] == 1 and all(np.isnan(ref[k]) for k in F64)
    top = np.finfo(np.float32).max
    ref = _reference([top, 0.5, 0.25], [-top, 0.1, 0.2])            # the float32 difference overflows
    assert ref["tested"] == 1 and all(np.isnan(ref[k]) for k in F64)
    ref = _reference([top, top, top], [0.0, 0.0, 0.0])              # a sum of 2 FLT_MAX is finite in float64
    assert ref["shift"] == ref["hi"] == float(top) and np.isfinite(ref["shift"])


def test_symmetries():
    rng = np.random.default_rng(92)
    for x, y, tied, grid in _rows(rng):
        ref, swapped = _reference(x, y), _reference(y, x)
        assert swapped["rank"] == ref["rank"]
        for a, b in (("shift", "shift"), ("lo", "hi"), ("hi", "lo")):
            want = -ref[b] + 0.0
            assert np.float64(swapped[a]).view(np.uint64) == np.float64(want).view(np.uint64), (a, x, y)
        # the order of the pairs changes nothing
        perm = rng.permutation(x.size)
        assert _reference(x[perm], y[perm]) == ref
        if grid:
            # a constant number of thousandths added to side 1 moves all three by exactly that, as integers
            keys = WR.grid_keys(x)
            k = int(rng.integers(-int(keys.min()), 1001 - int(keys.max())))
            moved = _reference(((keys + k) / 1000.0).astype(np.float32), y)
            assert moved["grid"] and moved["rank"] == ref["rank"]
            for name in F64:
                assert round(moved[name] * 4000) == round(ref[name] * 4000) + 4 * k, (name, k)


# ---------------------------------------------------------------- the levels and the fixtures
def test_no_rank_hangs_on_a_rounding_at_the_levels_of_the_fixtures():
    """M/2 - zq sqrt(m'(m'+1)(2m'+1)/24) is at least 1e-6 from an integer for every m' = 3..4096 at 50, 80, 90, 95 and 99 %;
    the nearest is 2.6e-6, at m' = 553 and 80 %"""
    assert WF.LEVELS == (0.5, 0.8, 0.9, 0.95, 0.99)
    worst = min((WR.rank_and_margin(m, WR.zq_of(conf))[1], m, conf) for m in range(3, 4097) for conf in WF.LEVELS)
    print(f"the nearest to an integer: {worst[0]:.3g} at m' = {worst[1]} and {worst[2]}")
    assert worst[0] >= MARGIN
    assert worst[1:] == (553, 0.8) and 2.5e-6 < worst[0] < 2.7e-6


def test_the_clamp_ends_at_seven_pairs_at_95_percent():
    assert [WR.rank_and_margin(m, ZQ95)[0] for m in range(3, 9)] == [1, 1, 1, 1, 2, 4]
    # the float64 expression as the kernels evaluate it gives the referee's rank at every pair count and level
    for conf in WF.LEVELS:
        zq = WR.zq_of(conf)
        for m in range(3, 4097):
            M = m * (m + 1) // 2
            assert max(1, int(np.floor(M / 2.0 - zq * np.sqrt(float(m * (m + 1) * (2 * m + 1)) / 24.0)))) == WR.rank_and_margin(m, zq)[0]


def test_fixture_condition_of_every_gpu_case():
    """the cases use the surveyed levels only and hold what the suites claim: odd and even M, the clamp c = 1 and ranks above
    it, untested rows, rows of every kept count from 0"""
    seen, counts = set(), set()
    for args, conf in WF.cases():
        assert conf in WF.LEVELS
        ps, a, b, _ = WF.table(*args)
        kept = (~(np.isnan(ps[:, a]) | np.isnan(ps[:, b]))).sum(axis=1)
        assert (kept >= 3).any() and (kept < 3).any(), args
        counts |= set(kept.tolist())
        for m in set(kept[kept >= 3].tolist()):
            c, margin = WR.rank_and_margin(m, WR.zq_of(conf))
            assert margin >= MARGIN
            seen.add(((m * (m + 1) // 2) % 2, c == 1))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}
    assert {0, 2, 3} <= counts and set(WF.PAIRS) <= counts


def test_tables_are_what_they_claim():
    top = np.finfo(np.float32).max
    for m in (3, 4, 8, 33, 64, 65, 129):
        for flavour in WF.FLAVOURS:
            ps, a, b, what = WF.table(m, flavour)
            assert ps.shape == (len(what), 2 * m + 3) and not ps.flags.writeable
            assert np.intersect1d(a, b).size == 0 and a.size == b.size == m
            assert {name for name, _ in what} == {k for k, fl in WF.KINDS.items() if flavour == "mixed" or flavour in fl}
            ref = WF.reference(m, flavour)
            for r, (name, grid) in enumerate(what):
                x, y = WR.kept_pairs(ps[r], a, b)
                assert (WR.grid_keys(np.concatenate([x, y])) is not None) == grid or x.size == 0, (m, flavour, name)
                with np.errstate(over="ignore", invalid="ignore"):
                    d = x - y
                if grid and x.size:                         # the differences of a grid row are those of its keys
                    keys = WR.grid_keys(np.concatenate([x, y]))
                    d = (keys[:x.size] - keys[x.size:]) / 1000.0
                if name.startswith("NaNs leaving"):
                    assert x.size == {"3": 3, "2": 2, "n": 0}[name[13]]
                if name == "no NaN":
                    assert x.size == m
                if name == "all differences zero":
                    assert x.size == m and not d.any() and ref["tested"][r] and not any(ref[k][r] for k in F64)
                if name == "all differences equal":
                    assert d[0] != 0 and (d == d[0]).all() and ref["shift"][r] == ref["lo"][r] == ref["hi"][r] != 0
                if name == "all positive":
                    assert (d > 0).all() and ref["lo"][r] > 0
                if name == "all negative":
                    assert (d < 0).all() and ref["hi"][r] < 0
                if name == "signed zeros":
                    zeros = np.concatenate([x, y])
                    zeros = zeros[zeros == 0]
                    assert np.signbit(zeros).any() and not np.signbit(zeros).all() and (grid or np.signbit(d[d == 0]).any())
                if name == "keys 0 and 1000":
                    assert {-1.0, 1.0} <= set(d.tolist()) and (m > 6 or (ref["lo"][r], ref["hi"][r]) == (-1.0, 1.0))
                if name == "+-FLT_MAX":
                    assert d.max() == top and d.min() == -top and np.isfinite(ref["shift"][r])
                if name == "subnormals":
                    assert 0 < np.abs(np.concatenate([x, y])).max() < np.finfo(np.float32).tiny
                if name == "outside [0, 1]":
                    assert x.max() > 1 and y.min() < 0
                if name == "a kept infinity":
                    assert np.isinf(np.concatenate([x, y])).sum() == 1
                if name == "FLT_MAX overflow":
                    assert np.isfinite(np.concatenate([x, y])).all() and np.isinf(d).sum() == 1
                assert np.isnan(ref["shift"][r]) == (name in WF.NAN_TRIPLES)
            if flavour == "mixed":
                assert {g for _, g in what} == {False, True}


# ---------------------------------------------------------------- the command's flag and refusals
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the context was touched: {name}")


NAMES = [f"s{j}" for j in range(12)]
SET1, SET2 = [0, 1, 2, 3], [4, 6, 9, 11]


def _manifest(tmp_path, name, group):
    path = tmp_path / name
    path.write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    return str(path)


def _args(tmp_path, **extra):
    table = tmp_path / "t_allPS.tsv"
    cells = [f"{0.05 * (j + 1):.3f}" for j in range(len(NAMES))]
    table.write_text("cluster\t" + "\t".join(NAMES) + "\n" + "chr1:1-2:+\t" + "\t".join(cells) + "\n" +
                     "chr1:5-9:+\t" + "\t".join(["nan"] * 3 + cells[3:]) + "\n")
    base = dict(psiSPLICEDICE=str(table), manifest1=_manifest(tmp_path, "m1.tsv", [NAMES[j] for j in SET1]),
                manifest2=_manifest(tmp_path, "m2.tsv", [NAMES[j] for j in SET2]), moreManifests=None, paired=True, exact=False,
                strata=None, trend=False, ks=False, shift=False, conf=None, posthoc=False, repeated=False, pseudomedian=True,
                annotation="", outputFile=str(tmp_path / "out.tsv"))
    if extra.pop("mx", False):
        base["moreManifests"] = [_manifest(tmp_path, "m3.tsv", [NAMES[j] for j in (5, 7, 8, 10)])]
    if extra.pop("with_strata", False):
        lab = tmp_path / "batches.tsv"
        lab.write_text("".join(f"{x}\tA\n" for x in NAMES))
        base["strata"] = str(lab)
    base.update(extra)
    return argparse.Namespace(**base)


NEEDS_PAIRED = ("compare_sample_sets --pseudomedian: needs --paired (it is the estimate that belongs to the signed-rank test of "
                "matched samples; two independent sets have --shift). Exit.")
OLD_CONF_LINE = "compare_sample_sets --conf: needs --shift (it is the level of the shift's confidence interval). Exit."
REFUSALS = {
    "without --paired": (dict(paired=False), NEEDS_PAIRED),
    "without --paired, with --exact": (dict(paired=False, exact=True), NEEDS_PAIRED),
    "without --paired, with --conf": (dict(paired=False, conf=0.9), NEEDS_PAIRED),
    "--conf with neither flag": (dict(pseudomedian=False, conf=0.9), OLD_CONF_LINE),
    "--conf with neither flag, unpaired": (dict(pseudomedian=False, paired=False, conf=0.9), OLD_CONF_LINE),
    "--conf 0": (dict(conf=0.0), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 0.0). Exit."),
    "--conf 1": (dict(conf=1.0), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 1.0). Exit."),
    "--conf -0.5": (dict(conf=-0.5), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got -0.5). Exit."),
    "--conf nan": (dict(conf=float("nan")), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got nan). Exit."),
    # the older refusals of --paired win, unchanged
    "with --shift": (dict(shift=True), "compare_sample_sets --shift: cannot be combined with --paired (the paired estimate is the "
                                       "median of the Walsh averages, which is not offered). Exit."),
    "with -mx": (dict(mx=True), "compare_sample_sets --paired: cannot be combined with -mx/--moreManifests (the signed-rank test "
                                "compares two matched sets). Exit."),
    "with --ks": (dict(ks=True), "compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares "
                                 "matched samples; this test compares two distributions). Exit."),
    "with --trend": (dict(trend=True), "compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two "
                                       "sets are the rank-sum test). Exit."),
    "with --trend -mx": (dict(trend=True, mx=True), "compare_sample_sets --trend: cannot be combined with --paired (the "
                                                    "signed-rank test compares two matched sets). Exit."),
    "with --strata": (dict(with_strata=True), "compare_sample_sets --strata: cannot be combined with --paired (the signed-rank "
                                              "test pairs samples one to one). Exit."),
    "with --repeated -mx": (dict(repeated=True, mx=True), "compare_sample_sets --repeated: cannot be combined with --paired (the "
                                                          "signed-rank test compares two matched sets; this test compares three "
                                                          "or more). Exit."),
}


def _refused(args, monkeypatch, capsys):
    """run_with must exit with status 1 before the table is read or a Context made -> the one line of stderr"""
    from splicedice_amd import compare_sample_sets as css

    def no_context(*a, **k):
        raise AssertionError("a Context was created")

    def no_table(*a, **k):
        raise AssertionError("the table was read")
    monkeypatch.setattr(css, "Context", no_context)
    monkeypatch.setattr(css, "read_ps_table", no_table)
    with pytest.raises(SystemExit) as e:
        css.run_with(args, ctx=Untouchable())
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.endswith(". Exit.\n"), err
    assert not os.path.exists(args.outputFile)
    return err[:-1]


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_1_before_any_engine_call(case, tmp_path, monkeypatch, capsys):
    kw, line = REFUSALS[case]
    assert _refused(_args(tmp_path, **kw), monkeypatch, capsys) == line


CSS_FLAGS = ("--paired", "--exact", "--strata", "--trend", "--ks", "-mx")
CSS_SUBSETS = [tuple(f for i, f in enumerate(CSS_FLAGS) if bits >> i & 1) for bits in range(1 << len(CSS_FLAGS))]


class _ReadsTheTable(Exception):
    pass


def _outcome(flags, pseudomedian, tmp_path, monkeypatch, capsys):
    """-> the line of the refusal, or None when the command gets as far as reading the table"""
    from splicedice_amd import compare_sample_sets as css

    def reads_the_table(*a, **k):
        raise _ReadsTheTable()
    monkeypatch.setattr(css, "read_ps_table", reads_the_table)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    args = _args(tmp_path, paired="--paired" in flags, exact="--exact" in flags, with_strata="--strata" in flags,
                 trend="--trend" in flags, ks="--ks" in flags, mx="-mx" in flags, pseudomedian=pseudomedian)
    try:
        css.run_with(args, ctx=Untouchable())
    except _ReadsTheTable:
        return None
    except SystemExit as e:
        err = capsys.readouterr().err
        assert e.code == 1 and err.count("\n") == 1 and not os.path.exists(args.outputFile)
        return err[:-1]
    raise AssertionError("run_with returned without reading the table")


@pytest.mark.parametrize("flags", CSS_SUBSETS, ids=lambda f: "+".join(f) or "plain")
def test_every_older_refusal_comes_first_and_unchanged(flags, tmp_path, monkeypatch, capsys):
    """with every combination of the older flags: where the command refuses without --pseudomedian it refuses with the same
    line with it; where it runs, it runs with --paired and names --paired as missing without"""
    before = _outcome(flags, False, tmp_path, monkeypatch, capsys)
    after = _outcome(flags, True, tmp_path, monkeypatch, capsys)
    if before is not None:
        assert after == before
    else:
        assert after == (None if "--paired" in flags else NEEDS_PAIRED)


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
    assert err == css.BY_FLAG["--pseudomedian"].multi_rank + "\n"
    assert err == ("compare_sample_sets: --pseudomedian is not available under the multi-rank launcher (the packed all-gather "
                   "carries the signed-rank fields only); run it in one process.\n")
    # the plain --paired command still runs sharded: it gets as far as the table
    assert _outcome(("--paired",), False, tmp_path, monkeypatch, capsys) is None


def test_the_flags_parse():
    from splicedice_amd import compare_sample_sets as css
    p = argparse.ArgumentParser()
    css.add_parser(p)
    base = ["--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "o"]
    a = p.parse_args(base)
    assert a.pseudomedian is False and a.conf is None
    a = p.parse_args(base + ["--paired", "--pseudomedian", "--exact"])
    assert a.pseudomedian is True and a.paired is True and a.exact is True and a.shift is False and a.conf is None
    assert p.parse_args(base + ["--paired", "--pseudomedian", "--conf", "0.9"]).conf == 0.9
    text = " ".join(p.format_help().split())               # (a stray % in a help text raises here)
    assert "--pseudomedian" in text and "(pseudo)median" in text and "With --shift or --pseudomedian" in text
    assert "--pseudomedian" in css.__doc__ and css.PSEUDOMEDIAN == css.TESTS[-1].flag == "--pseudomedian"
    assert css.BY_FLAG["--pseudomedian"].conflicts == () and css.BY_FLAG["--pseudomedian"].needs[0] == "--paired"


class StandIn:
    """a context without a device: the referee's paired shift beside made-up signed-rank fields; records what it was asked"""

    def __init__(self):
        self.asked = []

    def _plain(self, name, ps, a, b):
        self.asked.append(name)
        t = WR.table_reference(ps, a, b, ZQ95)["tested"]
        f32 = {k: np.where(t, np.float32(i + 1) / 8, 0).astype(np.float32) for i, k in enumerate(("med1", "med2", "mean1", "mean2", "delta"))}
        return dict(tested=t, p=np.where(t, 0.25, 0.0), z=np.zeros(t.size), exact=t.copy(), **f32)

    def signedrank(self, ps, a, b):
        return self._plain("signedrank", ps, a, b)

    def signedrank_exact(self, ps, a, b):
        return self._plain("signedrank_exact", ps, a, b)

    def walsh(self, ps, a, b, conf=0.95):
        self.asked.append(("walsh", conf, np.asarray(a).tolist(), np.asarray(b).tolist()))
        return WR.table_reference(ps, a, b, WR.zq_of(conf))

    def bh(self, p):
        return np.asarray(p) * 2


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("conf", [None, 0.5])
def test_the_command_on_a_stand_in_context(tmp_path, exact, conf):
    """the table gains shift, shift_lo and shift_hi between delta and p-value; the pairs are the manifests' lines; --conf
    reaches the call, 0.95 without it; with --exact the exact signed-rank call is the one beside it; without the flag the
    walsh call is not made and the table is the plain one"""
    from splicedice_amd import compare_sample_sets as css
    ctx = StandIn()
    args = _args(tmp_path, exact=exact, conf=conf)
    css.run_with(args, ctx=ctx)
    level = 0.95 if conf is None else conf
    assert ctx.asked == ["signedrank_exact" if exact else "signedrank", ("walsh", level, SET1, SET2)]
    lines = open(args.outputFile).read().split("\n")
    assert lines[0] == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tshift\tshift_lo\tshift_hi\tp-value\tcorrected"
    # s0 s1 s2 s3 = 0.05 .. 0.20 v s4 s6 s9 s11 = 0.25 0.35 0.50 0.60: d = -200 -250 -350 -400 thousandths, the 10 sums
    # -800 -750 -700 -650 -600 -600 -550 -500 -450 -400; the median is -1200 / 4000; c = 1 at 95 %, 3 at 50 %
    c = WR.rank_and_margin(4, WR.zq_of(level))[0]
    assert c == (1 if conf is None else 3)
    s = [-800, -750, -700, -650, -600, -600, -550, -500, -450, -400]
    want = [repr(v) for v in (-1200 / 4000.0, s[c - 1] / 2000.0, s[10 - c] / 2000.0)]
    assert lines[1].split("\t") == ["chr1:1-2:+", "0.375", "0.5", "0.125", "0.25", "0.625"] + want + ["0.25", "0.5"]
    assert lines[2:] == [""]                                   # the second row keeps one pair: not tested
    plain = StandIn()
    css.run_with(_args(tmp_path, pseudomedian=False, exact=exact), ctx=plain)
    assert plain.asked == ["signedrank_exact" if exact else "signedrank"]
    bare = open(args.outputFile).read().split("\n")
    assert bare[0] == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected"
    assert [line.split("\t") for line in bare] == [[c for i, c in enumerate(line.split("\t")) if i not in (6, 7, 8)] for line in lines]


# ---------------------------------------------------------------- the ABI
def test_abi_of_the_two_calls():
    from splicedice_amd import _ffi, engine
    from splicedice_amd.engine import Context
    lib = _ffi.load()
    header = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_walsh", "sdice_walsh_dev"):
        assert len(_ffi.SIGNATURES[name]) == 13 and hasattr(lib, name)
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and proto.group(1).count(",") == 12, name
        assert "double zq" in proto.group(1)
        assert _ffi.SIGNATURES[name][:7] == _ffi.SIGNATURES[name.replace("walsh", "signedrank")][:7]      # signedrank's inputs
        assert _ffi.SIGNATURES[name][7:] == _ffi.SIGNATURES[name.replace("walsh", "shift")][8:]           # + zq, shift's outputs
    assert engine.WALSH_FIELDS == engine.SHIFT_FIELDS and engine.ROW_TESTS["walsh"] == (engine.WALSH_FIELDS, ())
    assert [f[0] for f in engine.WALSH_FIELDS] == list(WR.OUTS)
    assert [np.dtype(f[1]) for f in engine.WALSH_FIELDS] == [np.dtype(dt) for _, dt in WR.FIELDS]
    assert callable(Context.walsh) and callable(Context.walsh_resident) and not hasattr(Context, "walsh_dev")
    assert "Zero differences are kept".upper() in header.upper()
