"""CPU: the referee of the Friedman / Page suites against scipy, brute force and identities; the fixtures; the parser, the
refusals and the table of compare_sample_sets --repeated on a stand-in context; the ABI declarations."""
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
import friedman_fixtures as FF  # noqa: E402
import friedman_referee as FR  # noqa: E402
import rank_support as RS  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(X):
    """a [k, m] block table as one table row and its sets"""
    X = np.asarray(X, np.float32)
    k, m = X.shape
    return X.reshape(1, -1), np.arange(k * m).reshape(k, m)


def _ref(X):
    ps, sets = _row(X)
    return {name: v[..., 0] for name, v in FR.table_reference(ps, sets).items()}


def _tied_tables(seed, shapes):
    rng = np.random.default_rng(seed)
    for k, m in shapes:
        levels = int(rng.integers(2, 9))
        yield np.round(rng.random((k, m)) * levels) / levels


# ------------------------------------------------------------------------------ the referee
def test_referee_against_scipy_friedmanchisquare():
    """Q and p at rtol 1e-12 wherever scipy is finite, on random tied tables k = 3..7, m = 3..19"""
    from scipy import stats
    seen = 0
    for X in _tied_tables(1, [(k, m) for k in range(3, 8) for m in range(3, 20)]):
        ref, sc = _ref(X), stats.friedmanchisquare(*np.asarray(X, np.float32))
        if not np.isfinite(sc.statistic):
            assert ref["q"] == 0 and ref["p_friedman"] == 1
            continue
        seen += 1
        assert abs(ref["q"] - sc.statistic) <= 1e-12 * sc.statistic and abs(ref["p_friedman"] - sc.pvalue) <= 1e-12 * sc.pvalue
        assert abs(ref["w"] - sc.statistic / (X.shape[1] * (X.shape[0] - 1))) <= 1e-12
    assert seen > 70


def test_referee_against_scipy_page_trend_test():
    """L on any data; z and p on untied data, where the conditional variance is the untied one scipy uses"""
    from scipy import stats
    rng = np.random.default_rng(2)
    for X in _tied_tables(3, [(3, 5), (4, 9), (6, 12)]):
        assert _ref(X)["l"] == stats.page_trend_test(np.asarray(X, np.float32).T).statistic
    for k, m in ((3, 4), (4, 10), (7, 25)):
        X = rng.permuted(np.tile(np.arange(k * m, dtype=np.float32).reshape(m, k).T, 1), axis=0)
        ref, sc = _ref(X), stats.page_trend_test(X.T, method="asymptotic")
        assert ref["l"] == sc.statistic
        z = (sc.statistic - m * k * (k + 1) ** 2 / 4) / np.sqrt(m * k ** 2 * (k + 1) ** 2 * (k - 1) / 144)
        assert abs(ref["z"] - z) <= 1e-12 * max(abs(z), 1e-300)
        assert abs(ref["p_page"] / 2 - sc.pvalue) <= 1e-9 * sc.pvalue if z > 0 else True      # (scipy: one-sided)


@pytest.mark.parametrize("m,k", [(2, 3), (3, 3), (2, 4)])
def test_page_mean_and_variance_by_brute_force(m, k):
    """E[L] = m k (k + 1)^2 / 4 and Var L = k (k + 1) den / 144 against all (k!)^m permutations inside the blocks, on tied
    data, as Fractions"""
    rng = np.random.default_rng(10 * m + k)
    X = rng.integers(0, 3, size=(k, m)).astype(np.float32)
    r2, C = FR.integers(X)
    den = m * (k ** 3 - k) - int(C)
    assert 0 < den < m * (k ** 3 - k)
    # the mid-ranks of every block, permuted over the sets
    lt = (X[None, :, :] < X[:, None, :]).sum(axis=1)
    eq = (X[None, :, :] == X[:, None, :]).sum(axis=1)
    half = [[Fraction(int(2 * lt[j, q] + eq[j, q] + 1), 2) for j in range(k)] for q in range(m)]
    values = []
    for perms in itertools.product(*[itertools.permutations(b) for b in half]):
        values.append(sum((j + 1) * sum(p[j] for p in perms) for j in range(k)))
    mean = sum(values) / len(values)
    var = sum((v - mean) ** 2 for v in values) / len(values)
    assert mean == Fraction(m * k * (k + 1) ** 2, 4)
    assert var == Fraction(k * (k + 1) * den, 144)


def test_two_sets_are_the_sign_test():
    """k = 2: Q = (n+ - n-)^2 / (n+ + n-), tied blocks count for nothing"""
    rng = np.random.default_rng(4)
    for _ in range(30):
        m = int(rng.integers(3, 40))
        X = rng.integers(0, 4, size=(2, m)).astype(np.float32)
        up, down = int((X[0] > X[1]).sum()), int((X[0] < X[1]).sum())
        ref = _ref(X)
        assert ref["q"] == (float(Fraction((up - down) ** 2, up + down)) if up + down else 0.0)


def test_invariances_of_the_referee():
    rng = np.random.default_rng(5)
    for X in _tied_tables(6, [(3, 6), (5, 11), (8, 30)]):
        k, m = X.shape
        X[rng.integers(0, k), rng.integers(0, m)] = np.nan
        ref = _ref(X)
        order = rng.permutation(k)
        for other, names in ((_ref(X[order]), ("q", "w", "p_friedman", "blocks", "delta")),
                             (_ref(X[:, rng.permutation(m)]), ("q", "w", "p_friedman", "z", "l", "p_page", "blocks", "med", "delta")),
                             (_ref(np.exp(3 * X) - 2), ("q", "w", "p_friedman", "z", "l", "p_page", "blocks"))):      # strictly increasing
            for name in names:
                assert np.array_equal(ref[name], other[name]), name
        rev = _ref(X[::-1])
        assert rev["z"] == -ref["z"] and rev["p_page"] == ref["p_page"] and ref["z"] != 0


def test_hand_case():
    """three subjects, three sets, one tie: ranks (1, 2, 3), (1, 2.5, 2.5), (2, 1, 3)"""
    X = np.float32([[0.1, 0.2, 0.5], [0.2, 0.4, 0.3], [0.3, 0.4, 0.9]])
    ref = _ref(X)
    # R = (4, 5.5, 8.5): D = 2R - 12 = (-4, -1, 5), sum D^2 = 42, C = 6, den = 3 * 24 - 6 = 66
    assert ref["q"] == float(Fraction(3 * 2 * 42, 66)) and ref["w"] == float(Fraction(3 * 42, 3 * 66)) and ref["blocks"] == 3
    assert ref["l"] == 4 + 2 * 5.5 + 3 * 8.5
    A, B = 6 * (-4 - 2 + 15), 3 * 4 * 66
    assert ref["z"] == FR.z_page(A, B)[0] and abs(ref["z"] - A / np.sqrt(B)) < 1e-15
    assert abs(ref["p_friedman"] - np.exp(-ref["q"] / 2)) < 1e-15                                # chi2.sf, 2 degrees of freedom
    assert ref["med"].tolist() == [np.float32(0.2), np.float32(0.3), np.float32(0.4)] and ref["delta"] == np.float32(0.4) - np.float32(0.2)
    untested = _ref(np.float32([[0.1, np.nan, 0.5], [0.2, 0.4, 0.3], [0.3, 0.4, 0.9]]))
    assert not any(np.any(untested[name]) for name in FR.FIELDS)


def test_every_magnitude_bound_holds_at_the_limits():
    """the bounds the header states, at the shapes that reach them: 3 (k - 1) sum D^2 < 2^50, den < 2^31, m' den < 2^43,
    |A| < 2^33, B < 2^43, and the 32-bit sums of the kernel"""
    for k, m in ((64, 256), (4, 4096), (2, 4096), (3, 4096), (63, 260), (16, 1024)):
        assert k * m <= FR.MAX_N and k <= FR.MAX_SETS and m <= FR.MAX_BLOCKS
        X = np.tile(np.arange(k, dtype=np.float32)[:, None], (1, m))          # every block in the same order: the largest D
        r2, C = FR.integers(X)
        pc = FR.pieces(r2, C, k, m)
        assert 3 * (k - 1) * pc["S"] < 2 ** 50 and pc["den"] < 2 ** 31 and m * pc["den"] < 2 ** 43
        assert abs(pc["A"]) < 2 ** 33 and pc["B"] < 2 ** 43
        assert max(r2) < 2 ** 32 and m * k * (k * k - 1) < 2 ** 32           # r2 per set, sum (t^2 - 1) per row
        assert float(FR.friedman_exact(pc["S"], pc["den"], k, m)[1]) == 1.0


def test_fixtures_cover_the_shapes_the_row_kinds_and_the_boundary():
    assert FF.staged(3, 3) == 12 and FF.staged(4, 256) == 1024 and FF.staged(4, 257) == 2048 and FF.staged(2, 1) == 4
    for k in FF.KS:
        ms = FF.shapes(k)
        assert {FF.staged(k, m) <= FF.WAVE_MAX for m in ms} == {True, False}
        assert all(k * m <= FR.MAX_N for m in ms) and (4096 in ms) == (k in (2, 3, 4))
    assert 256 in FF.shapes(64) and FF.WAVE_MAX in FF.KNOB_VALUES and 0 in FF.KNOB_VALUES
    rng = np.random.default_rng(7)
    sets, s = FF.draw_sets(rng, 5, 9)
    assert np.unique(sets).size == 45 and sets.max() < s
    for turn in range(3):
        ps, kinds = FF.table(rng, sets, s, turn)
        ref = FR.table_reference(ps, sets)
        by = dict(zip(kinds, range(len(kinds))))
        assert ref["blocks"][by["two blocks left"]] == 0 and ref["blocks"][by["three blocks left"]] == 3
        assert not ref["tested"][by["no block left"]] and not ref["tested"][by["a set of NaNs"]]
        r = by["blocks fully tied"]
        assert ref["tested"][r] and ref["q"][r] == 0 and ref["p_friedman"][r] == 1 and ref["z"][r] == 0 and ref["p_page"][r] == 1
        assert ref["w"][by["same order"]] == 1.0 and ref["q"][by["same order"]] == 9 * 4
        grid = RS.on_grid(ps[:, sets.reshape(-1)]).all(axis=1)
        assert grid.any() and not grid.all()
    special = ps[by["specials"], sets.reshape(-1)]
    assert np.signbit(special[special == 0]).any() and FF.FLT_MAX in special and -FF.FLT_MAX in special
    assert np.any((special != 0) & (np.abs(special) < np.finfo(np.float32).tiny))


# ------------------------------------------------------------------------------ engine, ABI
def test_friedman_columns():
    from splicedice_amd.engine import friedman_columns
    cols = friedman_columns([[4, 0, 2], [1, 5, 3]], 6)
    assert cols.dtype == np.int32 and cols.tolist() == [4, 0, 2, 1, 5, 3]
    for bad, what in (([[0, 1, 2], [3, 4]], "differ in length"), ([[0, 1, 2], [3, 4, 0]], "more than once"),
                      ([[0, 1, 2], [3, 4, 6]], "outside"), ([[0, 1, -1], [3, 4, 5]], "outside")):
        with pytest.raises(ValueError, match=what):
            friedman_columns(bad, 6)


def test_abi_declarations():
    from splicedice_amd import _ffi, engine
    header = open(os.path.join(REPO, "include", "sdice.h")).read()
    assert "#define SDICE_ABI_VERSION 1" in header
    for test, stats in (("friedman", ("q", "w")), ("page", ("z", "l"))):
        for form, d in (("", ""), ("_dev", "d_")):
            decl = re.search(r"int sdice_%s%s\(([^;]*)\);" % (test, form), header).group(1)
            names = [a.split()[-1].lstrip("*") for a in " ".join(decl.split()).split(",")]
            assert names == (["ctx", "n", "s", d + "ps", d + "cols", "k", "m"] +
                             [d + x for x in ("tested", "p", *stats, "blocks", "med", "mean", "delta")]), names
            sig = _ffi.SIGNATURES[f"sdice_{test}{form}"]
            assert len(sig) == len(names) and sig[5:7] == [_ffi.C.c_int32, _ffi.C.c_int32]
        fields, optional = engine.ROW_TESTS[test]
        assert [f[0] for f in fields] == ["tested", "p", *stats, "blocks", "med", "mean", "delta"]
        assert set(optional) == ({"q", "w", "blocks"} if test == "friedman" else {"l", "blocks"})
    assert engine.FRIEDMAN_FIELDS is engine.ROW_TESTS["friedman"][0] and engine.PAGE_FIELDS is engine.ROW_TESTS["page"][0]


def test_the_resident_methods_stay_out_of_the_dev_catalogue():
    """no Context method of this feature ends in _dev (tests/call_order_fixtures.py lists every _dev method and is not
    open for change); the resident forms say where they go"""
    from splicedice_amd.engine import Context
    import call_order_fixtures as COF
    for name in ("friedman", "friedman_resident", "page", "page_resident"):
        assert callable(getattr(Context, name))
    assert not hasattr(Context, "friedman_dev") and not hasattr(Context, "page_dev")
    for name in ("friedman_resident", "page_resident"):
        assert "catalogue" in getattr(Context, name).__doc__
    assert COF.CASES


# ------------------------------------------------------------------------------ the command
def test_parser():
    from splicedice_amd import compare_sample_sets as css
    p = argparse.ArgumentParser()
    css.add_parser(p)
    base = ["--psiSPLICEDICE", "t", "-m1", "a", "-m2", "b", "-o", "o"]
    assert p.parse_args(base).repeated is False
    a = p.parse_args(base + ["-mx", "c", "d", "--repeated", "--trend"])
    assert a.repeated is True and a.trend is True and a.moreManifests == ["c", "d"]
    text = " ".join(p.format_help().split())
    for word in ("Friedman", "Page", "same subject", "MANIFEST order", "Not with --paired, --exact, --strata, --ks, --shift or --posthoc"):
        assert word in text, word


def _manifests(tmp_path, lengths=(3, 3, 3), names=None):
    names = names or [[f"s{i}_{j}" for j in range(n)] for i, n in enumerate(lengths)]
    paths = []
    for i, g in enumerate(names):
        paths.append(tmp_path / f"m{i}.tsv")
        paths[-1].write_text("".join(f"{x}\tp\tm\tA\n" for x in g))
    table = tmp_path / "in_allPS.tsv"
    table.write_text("\t".join(["cluster"] + sorted({x for g in names for x in g})) + "\n")
    return [str(p) for p in paths], str(table)


def _args(tmp_path, manifests, table, **flags):
    return argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1],
                              moreManifests=manifests[2:] or None, annotation="", outputFile=str(tmp_path / "x.tsv"), **flags)


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
    assert not os.path.exists(args.outputFile)
    return err.strip()


REFUSALS = [
    (2, {}, "compare_sample_sets --repeated: needs -mx/--moreManifests (two matched sets are the signed-rank test: --paired). Exit."),
    (3, dict(paired=True), "compare_sample_sets --repeated: cannot be combined with --paired (the signed-rank test compares two "
                           "matched sets; this test compares three or more). Exit."),
    (3, dict(exact=True), "compare_sample_sets --repeated: cannot be combined with --exact (there is no exact Friedman test here). Exit."),
    (3, dict(strata="labels.tsv"), "compare_sample_sets --repeated: cannot be combined with --strata (the subjects are the blocks "
                                   "already; there is no stratified form). Exit."),
    (3, dict(ks=True), "compare_sample_sets --repeated: cannot be combined with --ks (the Kolmogorov-Smirnov test compares two "
                       "independent sets). Exit."),
    (3, dict(shift=True), "compare_sample_sets --repeated: cannot be combined with --shift (the shift is an estimate between two "
                          "independent sets). Exit."),
    (3, dict(posthoc=True), "compare_sample_sets --repeated: cannot be combined with --posthoc (there is no post-hoc test of "
                            "matched sets here). Exit."),
    (3, dict(posthoc=True, trend=True), "compare_sample_sets --repeated: cannot be combined with --posthoc (there is no post-hoc "
                                        "test of matched sets here). Exit."),
]


@pytest.mark.parametrize("n_sets,flags,line", REFUSALS, ids=[" ".join(f) or "alone" for _, f, _ in REFUSALS])
def test_every_refusal_of_repeated(tmp_path, capsys, monkeypatch, n_sets, flags, line):
    manifests, table = _manifests(tmp_path, (3,) * n_sets)
    assert _refused(_args(tmp_path, manifests, table, repeated=True, **flags), capsys, monkeypatch) == line


@pytest.mark.parametrize("trend", [False, True])
def test_repeated_under_the_launcher_is_refused(tmp_path, capsys, monkeypatch, trend):
    from splicedice_amd import compare_sample_sets as css, mgpu
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))
    manifests, table = _manifests(tmp_path)
    err = _refused(_args(tmp_path, manifests, table, repeated=True, trend=trend), capsys, monkeypatch)
    assert err == css.BY_FLAG[css.REPEATED].multi_rank == css.PAGE.multi_rank
    assert err.startswith("compare_sample_sets: --repeated is not available under the multi-rank launcher") and err != css.MULTI_RANK_REFUSAL


def test_paired_with_more_manifests_is_still_refused_with_its_old_line(tmp_path, capsys, monkeypatch):
    manifests, table = _manifests(tmp_path)
    err = _refused(_args(tmp_path, manifests, table, paired=True), capsys, monkeypatch)
    assert err == ("compare_sample_sets --paired: cannot be combined with -mx/--moreManifests (the signed-rank test compares "
                   "two matched sets). Exit.")


def test_manifests_that_are_not_one_line_per_subject_are_refused(tmp_path, capsys, monkeypatch):
    manifests, table = _manifests(tmp_path, (4, 4, 3))
    err = _refused(_args(tmp_path, manifests, table, repeated=True), capsys, monkeypatch)
    assert err == ("compare_sample_sets --repeated: the manifests differ in length (4, 4, 3 samples); line i of every manifest "
                   "is the same subject. Exit.")
    manifests, table = _manifests(tmp_path, names=[["a", "b", "c"], ["d", "e", "f"], ["g", "b", "h"]])
    err = _refused(_args(tmp_path, manifests, table, repeated=True, trend=True), capsys, monkeypatch)
    assert err == ("compare_sample_sets --repeated: sample 'b' appears twice in the manifests; a sample belongs to one set and "
                   "one subject only. Exit.")
    manifests, table = _manifests(tmp_path, (2, 2, 2))
    err = _refused(_args(tmp_path, manifests, table, repeated=True), capsys, monkeypatch)
    assert err == "compare_sample_sets --repeated: cannot conduct Friedman's test with fewer than 3 subjects (got 2). Exit."
    manifests, table = _manifests(tmp_path)
    open(table, "w").write("cluster\ts0_0\ts0_1\n")
    err = _refused(_args(tmp_path, manifests, table, repeated=True), capsys, monkeypatch)
    assert err == "compare_sample_sets --repeated: sample 's0_2' is missing from the table header. Exit."


def test_the_round_trip_keeps_q_apart_from_the_corrected_vector():
    """_cli.tested_rows holds its corrected p-values under a name no test's field has: Friedman's field `q` comes back as the
    launch wrote it, and the resident call gets the row's own buffers"""
    from splicedice_amd import _cli, compare_sample_sets as css, engine
    from oracle import oracle_np as O

    class Array:
        def __init__(self, host):
            self.host = host

        def to_host(self):
            return self.host.copy()

        def free(self):
            pass

    class Ctx:
        def to_device(self, host, dtype=None):
            return Array(np.array(host, dtype=dtype))

        def empty(self, shape, dtype):
            return Array(np.full(shape, 99, dtype))

        def sync(self):
            pass

        def bh_masked_dev(self, d_p, d_tested, d_q):
            d_q.host[:] = 0
            d_q.host[d_tested.host != 0] = O.bh_fdr(d_p.host[d_tested.host != 0])

        def friedman_resident(self, d_ps, d_cols, k, out):
            assert k == 3 and d_cols.host.tolist() == list(range(9))
            for f in engine.FRIEDMAN_FIELDS:
                out[f[0]].host[...] = {"tested": 1, "p": 0.25, "q": 7.5, "w": 0.5}.get(f[0], 3)

    sel = types.SimpleNamespace(set_idx=[[0, 1, 2], [3, 4, 5], [6, 7, 8]], cols=np.arange(9, dtype=np.int32))
    row, ctx = css.BY_FLAG[css.REPEATED], Ctx()
    keep, r = _cli.tested_rows(ctx, dict(ps=(np.zeros((4, 9)), np.float32), **row.inputs(sel)),
                               engine.field_shapes(row.fields, 4, row.k(sel)), row.dev(ctx, sel))
    assert keep.tolist() == [0, 1, 2, 3] and r["q"].tolist() == [7.5] * 4 and r["w"].tolist() == [0.5] * 4
    assert r["corrected"].tolist() == [0.25] * 4 and r["med"].shape == (3, 4)
    assert row.columns(3) == (("Q", "q"), ("W", "w")) and css.PAGE.columns(3) == (("z", "z"),)


class _StandIn:
    """a context without a device: friedman() and page() answer from the referee"""
    def __init__(self):
        self.calls = []

    def _answer(self, test, ps, sets):
        self.calls.append((test, [np.asarray(g).tolist() for g in sets]))
        ref = FR.table_reference(np.asarray(ps, np.float32), np.asarray(sets))
        stats = dict(q=ref["q"], w=ref["w"]) if test == "friedman" else dict(z=ref["z"], l=ref["l"])
        return dict(tested=ref["tested"], p=ref["p_" + test], blocks=ref["blocks"], med=ref["med"], mean=ref["mean"],
                    delta=ref["delta"], **stats)

    def friedman(self, ps, sets):
        return self._answer("friedman", ps, sets)

    def page(self, ps, sets):
        return self._answer("page", ps, sets)


@pytest.mark.parametrize("trend", [False, True])
def test_command_table_on_a_stand_in_context(tmp_path, monkeypatch, trend):
    """the table of the command with the engine replaced by the referee: the header, the order of the columns and every
    cell; the sets are taken in MANIFEST order (not the table's)"""
    from splicedice_amd import _cli, compare_sample_sets as css
    rng = np.random.default_rng(77 + trend)
    n, k, m = 14, 4, 5
    s = k * m + 2
    samples, _ = RS.ps_names(n, s)
    text = np.char.mod("%.3f", rng.integers(0, 1001, size=(n, s)) / 1000.0)
    sets = rng.permutation(s)[: k * m].reshape(k, m)
    text[3, sets[0, :3]] = "nan"                                            # two complete subjects: row dropped
    text[4, sets[2, 1]] = "nan"                                             # four complete subjects
    text[5] = "0.500"                                                       # fully tied: stays, p = 1
    table, manifests, names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in g], "A") for g in sets])
    ref = FR.table_reference(text.astype(np.float64).astype(np.float32), sets)
    assert ref["blocks"][[3, 4, 5]].tolist() == [0, 4, 5]
    stand_in = _StandIn()

    def host_pipeline(ctx, inputs, outputs, launch):                       # (_cli.tested_rows without a device)
        assert inputs["cols"][0].tolist() == sets.reshape(-1).tolist()
        res = getattr(ctx, "page" if trend else "friedman")(inputs["ps"][0], sets)
        assert set(outputs) == set(res)
        keep = np.flatnonzero(res.pop("tested"))
        r = {name: v[keep] if v.ndim == 1 else np.ascontiguousarray(v[:, keep]) for name, v in res.items() if name in outputs}
        r["corrected"] = r["p"] * 0.5
        return keep, r
    monkeypatch.setattr(_cli, "tested_rows", host_pipeline)
    out = str(tmp_path / "out.tsv")
    css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1], moreManifests=manifests[2:],
                                    repeated=True, trend=trend, annotation="", outputFile=out), ctx=stand_in)
    assert stand_in.calls == [("page" if trend else "friedman", sets.tolist())]
    lines = [ln.split("\t") for ln in open(out).read()[:-1].split("\n")]
    p = ref["p_page" if trend else "p_friedman"]
    keep, want = FR.command_table(ref, names, trend, p[ref["tested"].astype(bool)] * 0.5)
    assert lines[0] == FR.command_header(k, trend)
    assert lines[0][2 * k + 2: -2] == (["z"] if trend else ["Q", "W"])
    assert keep.tolist() == [r for r in range(n) if r != 3] and lines[1:] == want
