"""CPU: the host side of `compare_sample_sets -mx --posthoc` (Dunn's test for every pair of sets): the exact referee the GPU
tests lean on (tests/dunn_referee.py) against an independent float path (scipy's rankdata, the textbook formula, norm.sf),
the identity that ties the pair z's to H, k = 2, set permutations, Holm's step-down by brute force and a case small enough
for paper; the ABI declarations, the engine's field table, the flag with every new refusal, the header of the command's
table; and the condition on the GPU fixtures that no Holm order hangs on a rounding.  No device is touched."""
import argparse
import itertools
import os
import re
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dunn_fixtures as DF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import kruskal_referee as KR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_sets(rng, k, lo, hi, levels):
    return [rng.integers(0, levels, size=int(m)) for m in rng.integers(lo, hi + 1, size=k)]


def _not_constant(sets):
    return np.unique(np.concatenate(sets)).size > 1


# ------------------------------------------------------------------------------ the referee
def test_referee_against_scipy_float_path():
    """ranks from scipy.stats.rankdata, the textbook z = (Rbar_i - Rbar_j) / sqrt(sigma2 (1/n_i + 1/n_j)) with sigma2 =
    (N (N + 1) / 12) (1 - sum(t^3 - t) / (N^3 - N)), p = 2 norm.sf(|z|): z within 1e-13 relative, p within 1e-11"""
    from scipy.stats import norm, rankdata
    rng = np.random.default_rng(2901)
    worst_z = worst_p = 0.0
    for case in range(150):
        sets = _random_sets(rng, int(rng.integers(2, 8)), 3, 25, (4, 30, 1001)[case % 3])
        if not _not_constant(sets):
            continue
        allv = np.concatenate(sets).astype(np.float64)
        N = allv.size
        ranks = rankdata(allv)
        cuts = np.cumsum([0] + [g.size for g in sets])
        mean_rank = [ranks[cuts[i]: cuts[i + 1]].mean() for i in range(len(sets))]
        t = np.unique(allv, return_counts=True)[1].astype(np.float64)
        sigma2 = N * (N + 1) / 12.0 * (1.0 - (t ** 3 - t).sum() / (N ** 3 - N))
        z, p, _, _, _ = DR.row_pairs(DR.exact_pieces(sets))
        for q, (i, j) in enumerate(DR.pairs(len(sets))):
            zf = (mean_rank[i] - mean_rank[j]) / np.sqrt(sigma2 * (1.0 / sets[i].size + 1.0 / sets[j].size))
            pf = 2.0 * norm.sf(abs(zf))
            worst_z = max(worst_z, abs(z[q] - zf) / max(1.0, abs(zf)))
            worst_p = max(worst_p, abs(float(p[q]) - pf) / pf)
    print("worst z difference", worst_z, "worst relative p difference", worst_p)
    assert worst_z <= 1e-13 and worst_p <= 1e-11


def test_referee_pair_identity_with_h():
    """H = (1 / N) sum_{i<j} (n_i + n_j) z_ij^2 as exact Fractions against kruskal_referee.exact_h, tied and untied rows"""
    rng = np.random.default_rng(2902)
    seen = 0
    for case in range(200):
        sets = _random_sets(rng, int(rng.integers(2, 9)), 3, 20, (3, 12, 10 ** 6)[case % 3])
        h = KR.exact_h(sets)
        pc = DR.exact_pieces(sets)
        assert (h is None) == (pc["den"] == 0)
        if h is None:
            continue
        total = sum((pc["n"][i] + pc["n"][j]) * DR.z_squared(pc, i, j) for i, j in DR.pairs(len(sets)))
        assert total / pc["N"] == h, case
        seen += 1
    assert seen > 150


def test_referee_two_sets_z_squared_is_h():
    rng = np.random.default_rng(2903)
    for case in range(100):
        sets = _random_sets(rng, 2, 3, 30, (4, 1001)[case % 2])
        h = KR.exact_h(sets)
        if h is not None:
            assert DR.z_squared(DR.exact_pieces(sets), 0, 1) == h


def test_referee_set_permutation():
    """the sets in another order: z permutes and changes sign exactly where a pair turns round; the multiset of p and of
    padj is unchanged"""
    rng = np.random.default_rng(2904)
    for case in range(60):
        k = int(rng.integers(3, 7))
        sets = _random_sets(rng, k, 3, 15, (5, 1001)[case % 2])
        if not _not_constant(sets):
            continue
        perm = rng.permutation(k)
        z, p, padj, _, _ = DR.row_pairs(DR.exact_pieces(sets))
        z2, p2, padj2, _, _ = DR.row_pairs(DR.exact_pieces([sets[i] for i in perm]))
        where = {pr: q for q, pr in enumerate(DR.pairs(k))}
        for q, (a, b) in enumerate(DR.pairs(k)):               # new pair (a, b) holds the old sets perm[a], perm[b]
            i, j = int(perm[a]), int(perm[b])
            old = where[(min(i, j), max(i, j))]
            assert z2[q] == (z[old] if i < j else -z[old]) and p2[q] == p[old] and padj2[q] == padj[old]
        assert sorted(map(float, p)) == sorted(map(float, p2)) and sorted(map(float, padj)) == sorted(map(float, padj2))


def _holm_brute(ps):
    """Holm's step-down straight from its definition: padj_(r) = min(1, max_{t <= r} (m - t + 1) p_(t)) over EVERY ordering
    that sorts the p's ascending; the orderings must agree"""
    m = len(ps)
    results = set()
    for order in itertools.permutations(range(m)):
        if any(ps[order[r]] > ps[order[r + 1]] for r in range(m - 1)):
            continue
        out = [None] * m
        for r in range(m):
            out[order[r]] = min(Fraction(1), max((m - t) * ps[order[t]] for t in range(r + 1)))
        results.add(tuple(out))
    assert len(results) == 1, "the result depends on the order of equal p's"
    return list(results.pop())


def test_holm_by_brute_force():
    rng = np.random.default_rng(2905)
    cases = [[Fraction(1, 100)], [Fraction(1, 2), Fraction(1, 2)], [Fraction(1, 10), Fraction(1, 10), Fraction(1, 10)],
             [Fraction(1, 100), Fraction(1, 25), Fraction(3, 100)], [Fraction(9, 10), Fraction(1, 1000), Fraction(1, 2)],
             [Fraction(1, 1000), Fraction(1, 1000), Fraction(1, 2), Fraction(1, 2), Fraction(1, 3), Fraction(1)]]
    for _ in range(60):
        m = int(rng.integers(1, 7))
        cases.append([Fraction(int(x), 40) for x in rng.integers(0, 41, size=m)])          # many ties, many clipped
    clipped = tied = 0
    for ps in cases:
        got = DR.holm(ps)
        assert got == _holm_brute(ps), ps
        assert all(a >= p and a <= 1 for a, p in zip(got, ps))
        assert got[ps.index(min(ps))] == min(Fraction(1), len(ps) * min(ps))
        clipped += any(a == 1 and p < 1 for a, p in zip(got, ps))
        tied += len(set(ps)) < len(ps)
        for q, t in itertools.combinations(range(len(ps)), 2):
            assert ps[q] != ps[t] or got[q] == got[t]
    assert clipped > 10 and tied > 10


def test_hand_case():
    """k = 3 sets of 3, the values 1..9 in order, no ties: N = 9, mean ranks 2, 5, 8, sigma2 = 9 * 10 / 12 = 7.5;
    z12 = -3 / sqrt(7.5 * 2/3) = -3 / sqrt 5, z13 = -6 / sqrt 5, z23 = -3 / sqrt 5.  D = 2 R - n (N + 1) = (-18, 0, 18),
    den = 9^3 - 9 = 720.  Holm: p13 is the smallest, times 3; the two equal p's, times 2, both"""
    import mpmath
    pc = DR.exact_pieces([np.array([1, 2, 3]), np.array([4, 5, 6]), np.array([7, 8, 9])])
    assert pc == dict(N=9, n=[3, 3, 3], D=[-18, 0, 18], den=720)
    assert [DR.pair_num(pc, i, j) for i, j in DR.pairs(3)] == [-54, -108, -54]
    assert [DR.z_squared(pc, i, j) for i, j in DR.pairs(3)] == [Fraction(9, 5), Fraction(36, 5), Fraction(9, 5)]
    z, p, padj, _, _ = DR.row_pairs(pc)
    assert z == [-3 / 5 ** 0.5, -6 / 5 ** 0.5, -3 / 5 ** 0.5] == [-1.3416407864998738, -2.6832815729997477, -1.3416407864998738]
    from scipy.stats import norm
    with mpmath.workdps(DR.DPS):
        assert abs(p[0] - mpmath.mpf("0.179712494879")) < 1e-11 and abs(float(p[0]) - 2 * norm.sf(3 / 5 ** 0.5)) < 1e-15
        assert abs(p[1] - mpmath.mpf("0.0072903580915")) < 1e-12 and abs(float(p[1]) - 2 * norm.sf(6 / 5 ** 0.5)) < 1e-16
        assert padj[1] == 3 * p[1] and padj[0] == padj[2] == 2 * p[0] and p[0] == p[2]
    row = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], np.float32)
    ref = DR.row_reference(row, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], True)
    assert ref["tested"] == 1 and ref["pair_z"].tolist() == z and ref["hf"] == 7.2
    swapped = DR.row_reference(row, [[6, 7, 8], [3, 4, 5], [0, 1, 2]], True)
    assert swapped["pair_z"].tolist() == [-x for x in z][::-1]


def test_referee_all_equal_and_untested_rows():
    row = np.array([0.5] * 9 + [np.nan], np.float32)
    sets = [[0, 1, 2], [3, 4, 5], [6, 7, 8, 9]]
    ref = DR.row_reference(row, sets, True)
    assert ref["tested"] == 1 and ref["pieces"]["den"] == 0 and ref["hf"] == 0.0 and ref["p"] == 1.0
    assert ref["pair_z"].tolist() == [0.0] * 3 and [float(x) for x in ref["pair_p"] + ref["pair_padj"]] == [1.0] * 6
    row[1] = np.nan
    ref = DR.row_reference(row, sets, True)
    assert ref["tested"] == 0 and not ref["pair_z"].any() and ref["pair_p"] == ref["pair_padj"] == [0.0] * 3
    table = DR.table_reference(np.stack([row, row]), sets)
    assert table["pair_z"].shape == (3, 2) and not table["pair_p"].any() and table["exact"] == [None, None]


def test_rounded_sqrt_is_the_nearest_float():
    rng = np.random.default_rng(2906)
    for _ in range(300):
        q = Fraction(int(rng.integers(1, 10 ** 12)), int(rng.integers(1, 10 ** 9)))
        f = DR.rounded_sqrt(q)
        assert abs(Fraction(f) ** 2 - q) <= abs(Fraction(np.nextafter(f, 0.0)) ** 2 - q)
        assert abs(Fraction(f) ** 2 - q) <= abs(Fraction(np.nextafter(f, np.inf)) ** 2 - q)
    assert DR.rounded_sqrt(Fraction(9, 4)) == 1.5 and DR.rounded_sqrt(Fraction(0)) == 0.0


# ------------------------------------------------------------------------------ the GPU fixtures
def test_fixtures_cover_what_they_claim():
    assert DF.KS == (2, 3, 4, 5, 10, 11) and [k * (k - 1) // 2 for k in DF.KS] == [1, 3, 6, 10, 45, 55]
    assert set(DF.TOTALS) == set(range(9, 67)) | {127, 128, 129}
    for ps, sets, label in DF.column_count_fixtures("grid"):
        assert min(g.size for g in sets) >= 3 and f"total {sum(g.size for g in sets)} " in label
    assert [sum(g.size for g in sets) for _, sets, _ in DF.column_count_fixtures("mixed")] == list(DF.TOTALS)
    assert [g.size for g in DF.fixture("unequal 3v3v64 grid")[1]] == [3, 3, 64]
    assert [g.size for g in DF.fixture("unequal 4096v3v3 off")[1]] == [4096, 3, 3]
    from rank_support import on_grid
    for flavour in DF.FLAVOURS:
        ps, sets, _ = DF.fixture(f"row kinds {flavour}")
        grid = on_grid(ps[:, np.concatenate(sets)]).all(axis=1)
        assert {"grid": grid.all(), "off": not grid.any(), "mixed": grid.any() and not grid.all()}[flavour]
        ref = DF.reference(f"row kinds {flavour}")
        kinds = DF._kind_rows()[1]
        t = ref["tested"].astype(bool)
        assert not t[kinds == DF.KINDS.index("a set left with 2 kept values")].any() and t.sum() == t.size - 3
        equal = kinds == DF.KINDS.index("all values equal")
        assert np.all(ref["pair_p"][:, equal] == 1.0) and np.all(ref["pair_padj"][:, equal] == 1.0) and not ref["pair_z"][:, equal].any()
        ident = kinds == DF.KINDS.index("two sets identical")
        q13 = DR.pairs(4).index((1, 3))
        assert ref["zero_num"][q13, ident].all() and not ref["pair_z"][q13, ident].any()
        assert np.abs(ref["pair_z"][:, kinds == DF.KINDS.index("one set fully separated")]).max() > 3
    ref = DF.reference("ladder grid")
    z01 = ref["pair_z"][0]
    assert z01[0] == 0.0 and ref["zero_num"][0, 0] and np.all(np.diff(z01[8:]) > 0) and z01[-1] > 38 and ref["pair_p"][0, -1] == 0.0
    assert abs(z01[-1] - (1.5 * DF.LADDER_A) ** 0.5) < 0.5
    for lo, hi in ((1e-3, 1.0), (1e-20, 1e-3), (1e-100, 1e-20), (1e-280, 1e-100), (0.0, 1e-280)):
        assert np.any((ref["pair_p"][0] >= lo) & (ref["pair_p"][0] < hi)), (lo, hi)
    edges = DF.reference("block edges")
    with np.errstate(over="ignore"):
        assert edges["tested"].all() and not on_grid(DF.fixture("block edges")[0]).all(axis=1).any()


def _all_references():
    for name in DF.FIXTURES:
        yield name, DF.reference(name)
    for flavour in DF.FLAVOURS:
        for (_, _, label), ref in zip(DF.column_count_fixtures(flavour), DF.column_count_references(flavour)):
            yield label, ref
    yield "palette", DF.palette_reference()


def test_no_fixture_row_hangs_a_holm_order_on_a_rounding():
    """no row of a GPU fixture has two pair p-values closer than 1e-6 relative unless they are equal as Fractions (equal
    z^2): the float64 order of a row's p-values on the device is then the referee's, ties included"""
    rows = 0
    for name, ref in _all_references():
        assert DR.close_pairs(ref, 1e-6) == [], name
        rows += int(ref["tested"].sum())
    assert rows > 1400


# ------------------------------------------------------------------------------ ABI, engine, command line
def test_abi_declarations():
    from splicedice_amd import _ffi, engine
    lib = _ffi.load()
    header = open(os.path.join(REPO, "include", "sdice.h")).read()
    for name in ("sdice_kruskal_dunn", "sdice_kruskal_dunn_dev"):
        assert len(_ffi.SIGNATURES[name]) == len(_ffi.SIGNATURES["sdice_kruskal"]) + 3 == 16 and hasattr(lib, name)
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and proto.group(1).count(",") == 15, name
        assert re.search(r"pair_z, double\* (d_)?pair_p,\s+double\* (d_)?pair_padj$", proto.group(1)), proto.group(1)
    assert "#define SDICE_DUNN_MAX_SETS 11" in header and engine.DUNN_MAX_SETS == 11
    source = open(os.path.join(REPO, "splicedice_amd", "csrc", "kruskal.hip")).read()
    assert "rounding count 1," in source and "DUNN_MAX_SETS = SDICE_DUNN_MAX_SETS" in source


def test_engine_field_table_and_pair_order():
    from splicedice_amd import engine
    assert [f[0] for f in engine.KRUSKAL_DUNN_FIELDS] == [f[0] for f in engine.KRUSKAL_FIELDS] + ["pair_z", "pair_p", "pair_padj"]
    shapes = engine.field_shapes(engine.KRUSKAL_DUNN_FIELDS, 5, 4)
    assert shapes["med"] == ((4, 5), np.float32) and shapes["h"] == (5, np.float64)
    assert shapes["pair_z"] == shapes["pair_p"] == shapes["pair_padj"] == ((6, 5), np.float64)
    assert engine.field_shapes(engine.KRUSKAL_DUNN_FIELDS, 7, 11)["pair_padj"][0] == (55, 7)
    assert engine.dunn_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] == DR.pairs(4)
    assert engine.dunn_pairs(2) == [(0, 1)] and len(engine.dunn_pairs(11)) == 55
    assert hasattr(engine.Context, "kruskal_dunn") and hasattr(engine.Context, "kruskal_dunn_dev")


def test_posthoc_flag_default_and_parse():
    from splicedice_amd.__main__ import build_parser
    p = build_parser()
    base = ["compare_sample_sets", "--psiSPLICEDICE", "p", "-m1", "a", "-m2", "b", "-o", "x"]
    assert p.parse_args(base).posthoc is False
    got = p.parse_args(base + ["-mx", "c", "d", "--posthoc"])
    assert got.posthoc is True and got.moreManifests == ["c", "d"] and got.trend is False
    help_text = " ".join(a.help for sp in p._subparsers._group_actions for a in sp.choices["compare_sample_sets"]._actions
                         if a.dest == "posthoc")
    for word in ("Dunn's test", "z{i}v{j}", "padj{i}v{j}", "Holm", "At most 11 sets", "Not with --trend", "not part of the reference"):
        assert word in " ".join(help_text.split()), word


def _manifest(path, names):
    path.write_text("".join(f"{x}\tp\tm\tA\n" for x in names))
    return str(path)


def _args(tmp_path, n_sets, **flags):
    ms = [_manifest(tmp_path / f"m{i}.tsv", [f"s{i}_{j}" for j in range(3)]) for i in range(n_sets)]
    return argparse.Namespace(psiSPLICEDICE=str(tmp_path / "absent_allPS.tsv"), manifest1=ms[0], manifest2=ms[1],
                              moreManifests=ms[2:] or None, annotation="", outputFile=str(tmp_path / "x.tsv"), posthoc=True,
                              **flags)


def _refused(args, capsys, monkeypatch):
    """runs the command with every way to a device and to the table closed -> the single stderr line"""
    from splicedice_amd import compare_sample_sets as css

    def closed(*a, **k):
        raise AssertionError("a device was opened or the table was read")
    monkeypatch.setattr(css, "Context", closed)
    monkeypatch.setattr(css, "read_ps_table", closed)
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.endswith("\n") and "\n" not in err.strip() and err.strip()
    return err.strip()


def test_posthoc_without_more_manifests_is_refused(tmp_path, capsys, monkeypatch):
    err = _refused(_args(tmp_path, 2), capsys, monkeypatch)
    assert err.startswith("compare_sample_sets --posthoc: needs -mx/--moreManifests") and "rank-sum" in err


def test_posthoc_with_trend_is_refused(tmp_path, capsys, monkeypatch):
    err = _refused(_args(tmp_path, 3, trend=True), capsys, monkeypatch)
    assert err == ("compare_sample_sets --posthoc: cannot be combined with --trend (the trend test has one ordered "
                   "alternative, not pairs). Exit.")


@pytest.mark.parametrize("flag, value, start", [
    ("paired", True, "compare_sample_sets --paired: cannot be combined with -mx/--moreManifests"),
    ("exact", True, "compare_sample_sets --exact: cannot be combined with -mx/--moreManifests"),
    ("strata", "labels.tsv", "compare_sample_sets --strata: cannot be combined with -mx/--moreManifests"),
    ("ks", True, "compare_sample_sets --ks: cannot be combined with -mx/--moreManifests"),
    ("shift", True, "compare_sample_sets --shift: cannot be combined with -mx/--moreManifests")])
def test_posthoc_with_a_two_set_test_meets_that_tests_refusal_of_mx(tmp_path, capsys, monkeypatch, flag, value, start):
    assert _refused(_args(tmp_path, 3, **{flag: value}), capsys, monkeypatch).startswith(start)


def test_posthoc_under_the_launcher_is_refused(tmp_path, capsys, monkeypatch):
    from splicedice_amd import compare_sample_sets as css, mgpu
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))
    err = _refused(_args(tmp_path, 3), capsys, monkeypatch)
    assert err == css.BY_FLAG[css.POSTHOC].multi_rank and "--posthoc" in err and err != css.MULTI_RANK_REFUSAL


def test_posthoc_with_twelve_sets_is_refused_before_the_table_is_read(tmp_path, capsys, monkeypatch):
    err = _refused(_args(tmp_path, 12), capsys, monkeypatch)
    assert err.startswith("compare_sample_sets --posthoc: 12 sample sets, at most 11 are supported") and "66 pairs" in err


def test_posthoc_too_few_samples_exit(tmp_path, capsys):
    """the `<3 samples` exit stays as it is"""
    from splicedice_amd import compare_sample_sets as css
    args = _args(tmp_path, 3)
    _manifest(tmp_path / "m2.tsv", ["a", "b"])
    with pytest.raises(SystemExit) as e:
        css.run_with(args)
    assert e.value.code == 1
    assert "Cannot conduct wilcoxon with less than 3 samples in either group. Exit." in capsys.readouterr().err


class _StandIn:
    """a context without a device: kruskal_dunn() answers from the referee (no `ranksum_dev`: the host pipeline)"""
    def __init__(self):
        self.calls = []

    def kruskal_dunn(self, ps, sets):
        self.calls.append([np.asarray(g).tolist() for g in sets])
        ref = DR.table_reference(np.asarray(ps, np.float32), sets)
        return dict(tested=ref["tested"], p=ref["p"], h=ref["hf"], med=ref["med"], mean=ref["mean"], delta=ref["delta"],
                    pair_z=ref["pair_z"], pair_p=ref["pair_p"], pair_padj=ref["pair_padj"])

    def bh_masked_dev(self, *a):
        raise AssertionError("no device here")


@pytest.mark.parametrize("k", [3, 4])
def test_command_header_and_column_order_on_a_stand_in_context(tmp_path, monkeypatch, k):
    """the table of the command for k = 3 and 4 with the engine replaced by the referee: the header, the order of the
    columns and every cell; the -mx columns stand where they stand without the flag"""
    from splicedice_amd import _cli, compare_sample_sets as css
    import rank_support as RS
    rng = np.random.default_rng(2910 + k)
    n, per = 12, 4
    s = k * per + 1
    samples, _ = RS.ps_names(n, s)
    text = np.char.mod("%.3f", rng.integers(0, 1001, size=(n, s)) / 1000.0)
    text[3, :per - 1] = "nan"                                            # the first set keeps one value: row dropped
    text[5] = "0.500"
    groups = [([samples[i * per + j] for j in range(per)], "A") for i in range(k)]
    table, manifests, names = RS.write_ps_inputs(tmp_path, text, groups)
    matrix = text.astype(np.float64).astype(np.float32)
    sets = [np.arange(i * per, (i + 1) * per) for i in range(k)]
    ref = DR.table_reference(matrix, sets)
    stand_in = _StandIn()

    def host_pipeline(ctx, inputs, outputs, launch):                     # (_cli.tested_rows without a device)
        res = ctx.kruskal_dunn(inputs["ps"][0], sets)
        keep = np.flatnonzero(res.pop("tested"))
        r = {name: v[keep] if v.ndim == 1 else np.ascontiguousarray(v[:, keep]) for name, v in res.items() if name in outputs}
        r["corrected"] = r["p"] * 2.0
        return keep, r
    monkeypatch.setattr(_cli, "tested_rows", host_pipeline)
    out = str(tmp_path / "out.tsv")
    css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1],
                                    moreManifests=manifests[2:], posthoc=True, annotation="", outputFile=out), ctx=stand_in)
    assert stand_in.calls == [[g.tolist() for g in sets]]
    lines = [ln.split("\t") for ln in open(out).read()[:-1].split("\n")]
    header, keep, want = DR.command_table(ref, names, k, ref["p"][ref["tested"].astype(bool)] * 2.0)
    assert lines[0] == header == DR.command_header(k)
    m = k * (k - 1) // 2
    assert header[:2 + 2 * k] == ["event"] + [f"mean{i}" for i in range(1, k + 1)] + [f"median{i}" for i in range(1, k + 1)] + ["delta"]
    assert header[2 + 2 * k] == "H" and header[-2:] == ["p-value", "corrected"] and len(header) == 2 * k + 5 + 2 * m
    assert header[3 + 2 * k: 7 + 2 * k] == ["z1v2", "padj1v2", "z1v3", "padj1v3"] and header[-4:-2] == [f"z{k - 1}v{k}", f"padj{k - 1}v{k}"]
    assert DR.pair_cells(k)[0][0] == header.index("z1v2") and DR.pair_cells(k)[1][-1] == header.index(f"padj{k - 1}v{k}")
    assert keep.tolist() == [r for r in range(n) if r != 3] and len(lines) == keep.size + 1
    for got, cells in zip(lines[1:], want):
        assert got == [c if isinstance(c, str) else str(np.float64(c)) for c in cells]
