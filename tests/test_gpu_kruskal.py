"""GPU: sdice_kruskal (Kruskal-Wallis across k sample sets) and compare_sample_sets -mx against the exact referee
(tests/kruskal_referee.py: H as a rational number, p = chi2.sf of it) and numpy.

Bars: tested mask, medians, means and delta bit-exact against numpy; H within 1e-12 relative of the
exact rational; p within 1e-9 relative wherever the referee's p >= 1e-280, and those excluded cells are at most 1 % of
the tested rows (asserted)."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kruskal_referee as KR  # noqa: E402
import kset_fixtures as KF  # noqa: E402
import rank_support as RS  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import N_LIMIT, P_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

H_RTOL = 1e-12
KS = (3, 4, 5, 8, 16, 33, 64)
SIZE_RANGES = ((3, 6), (3, 40), (3, 300))
SHAPES = ("uniform", "shifted", "ties", "cluster")
OUTS = ("tested", "p", "h", "med", "mean", "delta")


def _table(rng, sets, s, hi, rows_per_shape, grid):
    return KF.table(rng, sets, s, hi, rows_per_shape, grid, SHAPES, lambda shape, r: r % 6 == 5)


def _check(got, ref, label):
    """-> (tested rows, cells below the p floor); asserts every bar"""
    t = RS.check_common(got, ref, ("med", "mean", "delta"), ("p", "h"), label)
    h, hr = got["h"][t], ref["hf"][t]
    err_h = np.abs(h - hr) / np.where(hr > 0, hr, 1.0)
    print(f"{label}: rows {t.size} tested {int(t.sum())} worst H rel {err_h.max() if err_h.size else 0:.3g}", end=" ")
    assert np.all(err_h <= H_RTOL), (label, float(err_h.max()))
    return int(t.sum()), RS.check_p(got["p"][t], ref["p"][t], label)[0]


def _parity(ctx, grid, seed, rows_per_shape):
    rng = np.random.default_rng(seed)
    tested = below = 0
    for k in KS:
        for lo, hi in SIZE_RANGES:
            sets, s = KF.draw_sets(rng, k, lo, hi)
            assert sum(g.size for g in sets) <= N_LIMIT
            ps = _table(rng, sets, s, hi, rows_per_shape, grid)
            got = ctx.kruskal(ps, sets)
            a, b = _check(got, KR.table_reference(ps, sets, grid), f"{'grid' if grid else 'general'} k={k} sizes {lo}..{hi}")
            tested += a
            below += b
    RS.check_floor_share(tested, below, "parity")


def test_parity_grid_path(ctx):
    """3-decimal PS values (the histogram kernel): every k x size range x value shape, NaNs, rows with a starved set"""
    _parity(ctx, True, 1207, 6)


def test_parity_general_path(ctx):
    """float32 values off the grid with random mantissas and exact duplicates (the sorting kernel); keys of the referee are
    the dense rank of the float32 values"""
    _parity(ctx, False, 1208, 6)


def test_general_path_row_at_the_limit(ctx):
    """N = 16384 selected columns, the most a call accepts: four sets of 4096, off-grid values with duplicates"""
    rng = np.random.default_rng(77)
    s = N_LIMIT
    perm = rng.permutation(s).astype(np.int32)
    sets = [perm[i * 4096: (i + 1) * 4096] for i in range(4)]
    ps = rng.random((2, s), dtype=np.float32)
    ps[0, perm[:4096]] += np.float32(0.01)
    ps[1, rng.integers(0, s, 500)] = ps[1, rng.integers(0, s, 500)]
    ps[1, rng.integers(0, s, 300)] = np.nan
    got = ctx.kruskal(ps, sets)
    _check(got, KR.table_reference(ps, sets, False), "general N=16384")
    grid = (np.rint(ps * 1000.0) / 1000.0).astype(np.float32)
    _check(ctx.kruskal(grid, sets), KR.table_reference(grid, sets, True), "grid N=16384")


def test_two_sets_equal_the_rank_sum_test(ctx):
    """k = 2 without ties: H = z^2 of sdice_ranksum and the p-values agree to 1e-12 relative; same tested mask"""
    rng = np.random.default_rng(5)
    n, s = 600, 80
    # distinct 20-bit fractions per row: no two values of a row are equal
    ps = np.stack([rng.choice(1 << 20, size=s, replace=False) for _ in range(n)]).astype(np.float32) / np.float32(1 << 20)
    ps[rng.random((n, s)) < 0.05] = np.nan
    ps[7, 40:78] = np.nan           # the second set keeps at most 2 values in this row
    g1, g2 = np.arange(0, 38, dtype=np.int32), np.arange(38, 78, dtype=np.int32)
    for r in range(n):              # no ties among the kept values of a row
        v = ps[r, :78]
        v = v[~np.isnan(v)]
        assert np.unique(v).size == v.size
    kw = ctx.kruskal(ps, [g1, g2])
    rs = ctx.ranksum(ps, g1, g2)
    assert np.array_equal(kw["tested"], rs["tested"]) and kw["tested"][7] == 0 and kw["tested"].sum() > 500
    t = rs["tested"].astype(bool)
    z2 = rs["z"][t] ** 2
    assert np.all(np.abs(kw["h"][t] - z2) <= 1e-12 * z2)
    assert np.all(np.abs(kw["p"][t] - rs["p"][t]) <= 1e-12 * rs["p"][t])
    assert np.array_equal(kw["med"][0], rs["med1"]) and np.array_equal(kw["med"][1], rs["med2"])
    assert np.array_equal(kw["mean"][0], rs["mean1"]) and np.array_equal(kw["mean"][1], rs["mean2"])


def test_invariants_at_one_million_rows(ctx):
    """1 M x 100, four sets of 25: permuting the sets permutes med / mean and leaves H and p bit-identical; permuting the
    columns inside a set leaves H, p and the medians bit-identical (the mean may move in its last bit)"""
    rng = np.random.default_rng(99)
    n, s = 1_000_000, 100
    ps = (rng.integers(0, 1001, size=(n, s), dtype=np.int32) / 1000.0).astype(np.float32)
    ps[rng.random((n, s), dtype=np.float32) < 0.02] = np.nan
    ps[::1000, :23] = np.nan        # a starved first set every 1000th row
    sets = [np.arange(25 * i, 25 * i + 25, dtype=np.int32) for i in range(4)]
    base = ctx.kruskal(ps, sets)
    assert base["tested"].sum() == n - n // 1000
    for r in (1, 2, 999_999):       # spot rows against the referee
        ref = KR.row_reference(ps[r], sets, True)
        assert abs(base["h"][r] - ref["hf"]) <= H_RTOL * ref["hf"] and abs(base["p"][r] - ref["p"]) <= P_RTOL * ref["p"]
        assert np.array_equal(base["med"][:, r], ref["med"]) and np.array_equal(base["mean"][:, r], ref["mean"])
    order = [2, 0, 3, 1]
    perm = ctx.kruskal(ps, [sets[i] for i in order])
    assert np.array_equal(perm["tested"], base["tested"])
    assert np.array_equal(perm["h"].view(np.uint64), base["h"].view(np.uint64))
    assert np.array_equal(perm["p"].view(np.uint64), base["p"].view(np.uint64))
    assert np.array_equal(perm["med"].view(np.uint32), base["med"][order].view(np.uint32))
    assert np.array_equal(perm["mean"].view(np.uint32), base["mean"][order].view(np.uint32))
    assert np.array_equal(perm["delta"].view(np.uint32), base["delta"].view(np.uint32))
    inner = ctx.kruskal(ps, [rng.permutation(g).astype(np.int32) for g in sets])
    assert np.array_equal(inner["tested"], base["tested"])
    assert np.array_equal(inner["h"].view(np.uint64), base["h"].view(np.uint64))
    assert np.array_equal(inner["p"].view(np.uint64), base["p"].view(np.uint64))
    assert np.array_equal(inner["med"].view(np.uint32), base["med"].view(np.uint32))


def test_all_equal_rows(ctx):
    """every kept value the same: tested, H = 0, p = 1 on both kernels (scipy raises there)"""
    ps = np.empty((4, 20), dtype=np.float32)
    ps[0] = 0.5
    ps[1] = 0.0
    ps[2] = np.float32(0.1234567)   # off the grid: the sorting kernel
    ps[3] = 1.0
    ps[3, 4] = np.nan
    sets = [np.arange(0, 6), np.arange(6, 13), np.arange(13, 20)]
    got = ctx.kruskal(ps, sets)
    assert got["tested"].tolist() == [1, 1, 1, 1]
    assert got["h"].tolist() == [0.0] * 4 and got["p"].tolist() == [1.0] * 4 and got["delta"].tolist() == [0.0] * 4
    ref = KR.table_reference(ps, sets, False)
    assert np.array_equal(got["med"], ref["med"]) and np.array_equal(got["mean"], ref["mean"])
    assert np.array_equal(got["med"], np.repeat(ps[:, :1], 3, axis=1).T)


@pytest.mark.parametrize("case", ["k=1", "k=65", "empty set", "N over the limit", "column in two sets"])
def test_errors_leave_the_outputs_untouched(ctx, case):
    n = 3
    if case == "k=1":
        s, cols, set_ptr, k = 10, np.arange(5), [0, 5], 1
    elif case == "k=65":
        s, cols, set_ptr, k = 200, np.arange(195), np.arange(0, 196, 3), 65
    elif case == "empty set":
        s, cols, set_ptr, k = 10, np.arange(8), [0, 4, 4, 8], 3
    elif case == "N over the limit":
        s, cols, set_ptr, k = N_LIMIT + 1, np.arange(N_LIMIT + 1), [0, 8000, N_LIMIT + 1], 2
    else:
        s, cols, set_ptr, k = 10, [0, 1, 2, 3, 4, 2], [0, 3, 6], 2
    ps = np.full((n, s), 0.5, dtype=np.float32)
    kk = max(k, 2)
    outs = dict(tested=np.full(n, 7, np.uint8), p=np.full(n, -3.0), h=np.full(n, -4.0), med=np.full((kk, n), -5.0, np.float32),
                mean=np.full((kk, n), -6.0, np.float32), delta=np.full(n, -7.0, np.float32))
    before = {x: v.copy() for x, v in outs.items()}
    rc = RS.raw_call(ctx, "sdice_kruskal", ps, (cols, set_ptr, k), outs, OUTS)
    assert rc < 0, case
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "N over the limit":
        assert b"16384" in ctx.lib.sdice_last_error()
    # the context still works
    ok = ctx.kruskal(np.full((2, 9), 0.25, np.float32), [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    assert ok["tested"].tolist() == [1, 1]


def test_engine_refuses_a_column_in_two_sets_before_any_launch(ctx):
    with pytest.raises(ValueError, match="one set only"):
        ctx.kruskal(np.zeros((2, 9), np.float32), [[0, 1, 2], [3, 4, 5], [6, 7, 0]])


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    rng = np.random.default_rng(4242)
    n, s = 300, 24
    samples, _ = RS.ps_names(n, s)
    v = rng.integers(0, 1001, size=(n, s)) / 1000.0
    v[:, 6:12] = np.clip(v[:, 6:12] * 0.7 + 0.2 * rng.random((n, 1)), 0, 1)
    v[:40] = np.round(v[:40] * 2) / 2                                     # heavy ties
    v[40:50] = 0.5                                                        # all-equal rows stay in the table
    text = np.where(rng.random((n, s)) < 0.08, "nan", np.char.mod("%.3f", v))
    text[40:50] = "0.500"
    text[60:70, 0:5] = "nan"                                              # the first set keeps one value: rows dropped
    groups = [samples[0:6], samples[6:12] + ["not_in_the_table"], samples[12:17], samples[17:23]]
    table, manifests, names = RS.write_ps_inputs(tmp_path, text, [(g, "A") for g in groups])
    return table, manifests, groups, samples, names


@pytest.mark.parametrize("gtf", [False, True])
def test_cli_more_manifests(ctx, golden_dir, tmp_path, gtf):
    """compare_sample_sets -mx on a synthesised 300 x 24 table and four manifests (one names a sample the table lacks):
    event, means, medians, delta and the GTF columns are compared as strings built from numpy and the host annotation
    code; H, p-value and corrected are float64 and the engine's last bits differ from the referee's, so those fields are
    parsed and held to the parity bars (H 1e-12, p and BH 1e-9 relative) and must be repr round-trips."""
    from splicedice_amd import compare_sample_sets as css
    table, manifests, groups, samples, names = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    args = argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1], moreManifests=manifests[2:],
                              annotation=anno, outputFile=out)
    css.run_with(args, ctx=ctx)
    _, cols, matrix = css.read_ps_table(table)
    sets = [np.flatnonzero(np.isin(np.array(samples), g)) for g in groups]
    assert [len(g) for g in sets] == [6, 6, 5, 6]
    ref = KR.table_reference(matrix, sets, True)
    keep = np.flatnonzero(ref["tested"])
    assert 200 < keep.size < 300 and set(range(40, 50)) <= set(keep.tolist()) and not set(range(60, 70)) & set(keep.tolist())
    q = O.bh_fdr(ref["p"][keep])
    lines = [ln.rstrip("\n").split("\t") for ln in open(out)]
    header = ["event"] + [f"mean{i}" for i in range(1, 5)] + [f"median{i}" for i in range(1, 5)] + ["delta", "H", "p-value", "corrected"]
    if gtf:
        header += ["gene", "overlapping", "transcript_id"]
        sfx = css.annotation_suffixes([names[r] for r in keep], anno)
    assert lines[0] == header
    assert len(lines) == keep.size + 1
    for i, r in enumerate(keep):
        f = lines[i + 1]
        want = [names[r]] + [str(x) for x in ref["mean"][:, r]] + [str(x) for x in ref["med"][:, r]] + [str(ref["delta"][r])]
        assert f[:10] == want, (r, f[:10], want)
        for field, val, tol in ((f[10], ref["hf"][r], H_RTOL), (f[11], ref["p"][r], P_RTOL), (f[12], q[i], P_RTOL)):
            assert str(np.float64(float(field))) == field
            assert abs(float(field) - val) <= tol * abs(val), (r, field, val)
        if gtf:
            assert "\t" + "\t".join(f[13:]) == sfx[i]
        else:
            assert len(f) == 13


def test_cli_two_manifests_unchanged(ctx, tmp_path):
    """without -mx the command is the two-set command: its file equals the table built from compare() called directly"""
    from splicedice_amd import compare_sample_sets as css, textio
    table, manifests, groups, samples, names = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "two.tsv")
    args = argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1], annotation="", outputFile=out)
    css.run_with(args, ctx=ctx)
    args.moreManifests = None
    out2 = str(tmp_path / "two_again.tsv")
    args.outputFile = out2
    css.run_with(args, ctx=ctx)
    rows, cols, matrix = css.read_ps_table(table, as_table=True)
    keep, r = css.compare(matrix, css.column_indices(groups[0], cols), css.column_indices(groups[1], cols), ctx)
    want = str(tmp_path / "want.tsv")
    textio.write_columns(want, "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected\n", rows.take(keep),
                         [r["mean1"], r["mean2"], r["med1"], r["med2"], r["delta"], r["p"], r["corrected"]], ["repr"] * 7)
    assert open(out, "rb").read() == open(want, "rb").read() == open(out2, "rb").read()
    assert keep.size > 200
