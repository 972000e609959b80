"""sdice_spearman (Spearman rank correlation of the PS values of the listed columns with a sample covariate) and the
`correlate` sub-command against the referee (tests/spearman_referee.py: integer rank sums, mpmath at 50 digits) and numpy.

Bars: tested mask, n_kept, mean and median bit-exact; rho within 1e-12 relative of the referee and
exactly 0 / +-1 where the referee's is; p within 1e-9 relative wherever the referee's p >= 1e-280 and under 2e-280 below
that, exactly 0 where |rho| = 1 and exactly 1 where rho = 0.  No float32 field is compared by value only: zero means and
medians carry numpy's sign.

One table per column count mixes every row kind of KINDS in 72 (from 127 columns: 48) distinct rows, repeated into 3109; the listed columns are a scrambled subset of the table's columns
(s = m + 3) and every table is tested against three covariates: heavy ties, no ties, every value tied but one.  The table
builders and their references are cached and shared with tests/test_gpu_spearman_sweeps.py.  Tests without the gpu mark
check on the CPU that the tables are what they claim."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import spearman_referee as SP  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

gpu = pytest.mark.gpu

RHO_RTOL = 1e-12
M_LIMIT = 4096                      # columns a call accepts (include/sdice.h)
# every column count of the lane-group kernel and past it (groups of 8, 16, 32 and 64 lanes, the wave-per-row kernel from 65)
MS_SMALL = tuple(range(3, 67))
# the wave-per-row kernel with 2 (to 128) and 4 (to 256) columns a lane, the workgroup kernel from 257: each side of its
# LDS sizes (powers of two from 512), the limit
MS_BIG = (127, 128, 129, 191, 192, 193, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4095, 4096)
KINDS = ("all NaN", "two kept", "three kept", "constant PS", "covariate constant among the kept", "monotone up",
         "monotone down", "heavy ties", "off-grid", "signed zeros", "3-decimal", "mixed")
COVARIATES = ("tied", "untied", "all but one tied")
OUTS = ("tested", "p", "rho", "n_kept", "med", "mean")
F32 = ("med", "mean")


def per_kind(m):
    return 6 if m <= 66 else 4


@functools.lru_cache(maxsize=None)
def design(m):
    """-> (cols int32[m]: a scrambled subset of s = m + 3 table columns, a int64[m]: the base covariate of each listed
    column, integers with heavy ties and, from 5 columns up, a tie group of at least 3)"""
    rng = np.random.default_rng(77000 + m)
    s = m + 3
    cols = rng.permutation(s)[:m].astype(np.int32)
    a = rng.integers(0, max(2, m // 3), size=m)
    if m >= 5:
        a[rng.permutation(m)[:3]] = a[0]
    if np.unique(a).size == 1:
        a[-1] += 1
    return cols, a


def covariate(m, which):
    """the covariate value of each listed column, float64"""
    _, a = design(m)
    rng = np.random.default_rng(88000 + m)
    if which == "tied":
        return a.astype(np.float64)
    if which == "untied":
        return a + rng.permutation(m) / (2.0 * m)            # the order between the tie groups of `a` stays
    x = np.full(m, 2.5)
    x[int(rng.integers(0, m))] = -1.0 if m % 2 else 7.0
    return x


def make_row(rng, kind, v, m):
    """the listed values of one row of KINDS[kind], variant v, in the order of design(m)'s columns"""
    name = KINDS[kind]
    _, a = design(m)
    z = (a - a.mean()) / (a.std() + 1e-9)
    slope = rng.choice([-1.0, 1.0]) * rng.choice([0.0, 0.5, 1.5, 4.0]) / np.sqrt(m)      # |t| of 0 .. 4 or so
    base = np.clip(0.5 + 0.25 * (slope * z + rng.standard_normal(m)), 0.0, 1.0)
    grid = (np.rint(base * 1000.0) / 1000.0).astype(np.float32)
    off = (base * 1.7 - 0.3).astype(np.float32) + rng.random(m, dtype=np.float32) * np.float32(1e-3)
    if m > 3:
        dup = rng.integers(0, m, size=(max(1, m // 6), 2))
        off[dup[:, 0]] = off[dup[:, 1]]
    if name == "all NaN":
        return np.full(m, np.nan, np.float32)
    if name in ("two kept", "three kept"):
        y = grid if v % 2 else off
        y[rng.permutation(m)[(2 if name == "two kept" else 3):]] = np.nan
        return y
    if name == "constant PS":
        y = np.full(m, [0.5, 0.0, 1.0, 0.1234567, -0.0, 0.25][v % 6], np.float32)
        if v % 2:
            y[rng.random(m) < 0.2] = np.nan
        return y
    if name == "covariate constant among the kept":
        vals, cnt = np.unique(a, return_counts=True)
        y = grid if v % 2 else off
        if cnt.max() >= 3:
            y[a != vals[np.argmax(cnt)]] = np.nan
        return y
    if name in ("monotone up", "monotone down"):
        y = (a.astype(np.float32) + np.float32(1)) / np.float32(a.max() + 2)          # distinct for distinct a
        y = y if name == "monotone up" else np.float32(1) - y
        if v % 2:
            y[rng.random(m) < 0.15] = np.nan
        return y.astype(np.float32)
    if name == "heavy ties":
        y = (np.rint(base * 4) / 4).astype(np.float32)
        if v % 3 == 0:
            y[rng.random(m) < 0.1] = np.nan
        return y
    if name == "off-grid":
        if v % 2:
            off[rng.random(m) < 0.06] = np.nan
        return off
    if name == "signed zeros":
        y = grid if v % 2 else off
        sel = rng.permutation(m)[: max(1, m // 3)]
        y[sel] = rng.choice(np.array([-0.0, 0.0], np.float32), size=sel.size)
        if v >= 4:
            y[:] = rng.choice(np.array([-0.0, 0.0], np.float32), size=m)          # nothing but zeros of either sign
            if v == 5:
                y[:] = -0.0
        return y
    if name == "3-decimal":
        if v % 2:
            grid[rng.random(m) < [0.06, 0.3][v // 2 % 2]] = np.nan
        return grid
    y = np.where(rng.random(m) < 0.5, grid, off).astype(np.float32)                   # mixed
    y[rng.random(m) < 0.1] = np.nan
    return y


@functools.lru_cache(maxsize=None)
def table(m):
    """-> (ps float32[rows, m + 3], cols, kind[rows]); the kinds interleaved, so that neighbouring rows (and the rows side
    by side in a wave) are of different kinds; the spare columns hold what would show if one were read"""
    rng = np.random.default_rng(20260 + m)
    cols, _ = design(m)
    rows, kinds = [], []
    for v in range(per_kind(m)):
        for k in range(len(KINDS)):
            row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=m + 3)
            row[cols] = make_row(rng, k, v, m)
            rows.append(row)
            kinds.append(k)
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, cols, np.array(kinds)


def sorted_design(cols, x):
    """the order the library gets: by covariate, ties in the order given -> (cols, x) sorted"""
    order = np.argsort(np.asarray(x, np.float64), kind="stable")
    return np.asarray(cols)[order], np.asarray(x, np.float64)[order]


@functools.lru_cache(maxsize=None)
def reference(m, which):
    ps, cols, _ = table(m)
    return SP.table_reference(ps, *sorted_design(cols, covariate(m, which)))


def check(got, ref, label):
    """asserts every bar -> dict(tested, below, rho_err, p_err)"""
    bad = np.flatnonzero(got["n_kept"] != ref["n_kept"])
    assert bad.size == 0 and got["n_kept"].dtype == np.int32, (label, "n_kept", bad[:5])
    t = RS.check_common(got, ref, F32, ("p", "rho"), label)
    r, rr = got["rho"][t], ref["rho"][t]
    edge = (rr == 0) | (np.abs(rr) == 1)
    assert np.array_equal(r[edge], rr[edge]), (label, "rho at 0 / +-1")
    err_r = np.abs(r - rr) / np.where(rr != 0, np.abs(rr), 1.0)
    p = got["p"][t]
    assert np.all(p[np.abs(rr) == 1] == 0) and np.all(p[rr == 0] == 1), (label, "p at the edges")
    out = dict(tested=int(t.sum()), rho_err=float(err_r.max()) if err_r.size else 0.0)
    print(f"{label}: rows {t.size} tested {out['tested']} worst rho rel {out['rho_err']:.3g}", end=" ")
    assert np.all(err_r <= RHO_RTOL), (label, out["rho_err"])
    out["below"], out["p_err"] = RS.check_p(p, ref["p"][t], label)
    return out


# ---------------------------------------------------------------- the tables, on the CPU
@pytest.mark.parametrize("m", (3, 4, 5, 8, 9, 33, 66, 129, 193, 1024))
def test_tables_are_what_they_claim(m):
    """every kind is what its name says under the tied covariate, by the referee alone; the listed columns are a scrambled
    subset of a wider table"""
    ps, cols, kind = table(m)
    ref = reference(m, "tied")
    _, a = design(m)
    assert ps.shape == (len(KINDS) * per_kind(m), m + 3) and np.unique(cols).size == m
    if m >= 8:
        assert (np.diff(cols) < 0).any() and (np.diff(cols) > 0).any()
    xs = sorted_design(cols, covariate(m, "tied"))[1]
    assert np.unique(xs).size < m or m < 5                                     # ties
    assert np.unique(covariate(m, "untied")).size == m and np.unique(covariate(m, "all but one tied")).size == 2
    assert np.array_equal(a[np.argsort(covariate(m, "untied"))], np.sort(a))     # the untied one keeps the order of the groups
    y = ps[:, cols]
    kept = ~np.isnan(y)
    seen_one, negative_zero = set(), False
    for r in range(ps.shape[0]):
        name, nk = KINDS[kind[r]], int(kept[r].sum())
        assert ref["tested"][r] == (nk >= 3) and ref["n_kept"][r] == (nk if nk >= 3 else 0), (r, name)
        if name == "all NaN":
            assert nk == 0
        if name == "two kept":
            assert nk == 2
        if name == "three kept":
            assert nk == 3 and ref["tested"][r]
        if name == "constant PS" and nk >= 3:
            assert (ref["rho"][r], ref["p"][r]) == (0.0, 1.0) and ref["tested"][r]
        if name == "covariate constant among the kept" and m >= 5:
            assert nk >= 3 and np.unique(a[kept[r]]).size == 1 and (ref["rho"][r], ref["p"][r]) == (0.0, 1.0)
        if name in ("monotone up", "monotone down") and ref["tested"][r] and np.unique(a[kept[r]]).size > 1:
            assert ref["rho"][r] == (1.0 if name == "monotone up" else -1.0) and ref["p"][r] == 0.0
            seen_one.add(name)
        if name == "signed zeros":
            yy = y[r][kept[r]]
            assert (yy == 0).any()
            negative_zero |= bool(np.signbit(yy[yy == 0]).any())
    assert seen_one == {"monotone up", "monotone down"} and negative_zero
    t = ref["tested"].astype(bool)
    if m >= 9:
        assert np.unique(ref["rho"][t]).size > 20 and ((ref["p"][t] > 0) & (ref["p"][t] < 1)).sum() > 20


# ---------------------------------------------------------------- the library
PARITY_ROWS = 3109                  # rows of a parity call: more than the workgroup kernel's grid has workgroups


def _parity(ctx, m):
    """the table's distinct rows (the referee costs milliseconds a row) repeated into a few thousand, every one compared"""
    ps, cols, _ = table(m)
    idx = RS.palette_index(PARITY_ROWS, ps.shape[0])
    big = np.ascontiguousarray(ps[idx])
    for which in COVARIATES:
        check(ctx.spearman(big, cols, covariate(m, which)), RS.scatter(reference(m, which), idx), f"m={m} {which}")


@gpu
@pytest.mark.parametrize("m", MS_SMALL)
def test_spearman_parity_every_small_m(ctx, m):
    """every row kind, mixed in one table, at every column count of the lane-group kernel and the first two of the
    wave-per-row kernel, under three covariates"""
    _parity(ctx, m)


@gpu
@pytest.mark.parametrize("m", MS_BIG)
def test_spearman_parity_wave_and_workgroup_sizes(ctx, m):
    """the wave-per-row kernel where its columns per lane change (128 | 129) and inside a lane's last element (191..193),
    its hand-over to the workgroup kernel (256 | 257), that kernel on each side of its LDS sizes, 4095 and 4096 columns"""
    _parity(ctx, m)


@gpu
def test_table_order_of_the_columns_does_not_matter_but_list_order_does_for_ties_only(ctx):
    """the same samples listed in another order: the same statistics (rho, p, n, median); an untied covariate fixes the
    library's order, so the mean is the same bits too"""
    m = 23
    ps, cols, _ = table(m)
    x = covariate(m, "untied")
    base = ctx.spearman(ps, cols, x)
    perm = np.random.default_rng(4).permutation(m)
    again = ctx.spearman(ps, cols[perm], x[perm])
    for name in OUTS:
        assert np.array_equal(base[name].view(np.uint8), again[name].view(np.uint8)), name
    check(again, reference(m, "untied"), "listed in another order")


@gpu
def test_edges_and_tiny_calls(ctx):
    """|rho| = 1 gives p = 0 from 3 kept samples up, constant sides give rho = 0 and p = 1 and stay tested; n = 0 is a
    no-op"""
    ps = np.array([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, np.nan], [0.5, 0.5, 0.5, 0.5], [np.nan, 0.2, np.nan, 0.9],
                   [0.3, 0.1, 0.2, 0.25]], dtype=np.float32)
    got = ctx.spearman(ps, [0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0])
    assert got["tested"].tolist() == [1, 1, 1, 0, 1] and got["n_kept"].tolist() == [4, 3, 4, 0, 4]
    assert got["rho"][:4].tolist() == [1.0, -1.0, 0.0, 0.0] and got["p"][:4].tolist() == [0.0, 0.0, 1.0, 0.0]
    check(got, SP.table_reference(ps, [0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0]), "edges")
    flat = ctx.spearman(ps, [0, 1, 2, 3], [5.0, 5.0, 5.0, 5.0])
    assert flat["tested"].tolist() == [1, 1, 1, 0, 1] and not flat["rho"].any() and flat["p"].tolist() == [1, 1, 1, 0, 1]
    empty = ctx.spearman(np.zeros((0, 8), np.float32), [0, 1, 2], [1.0, 2.0, 3.0])
    assert all(empty[name].shape == (0,) for name in OUTS)


@gpu
@pytest.mark.parametrize("m", (7, 40, 100, 200, 300))
def test_dev_entry_with_and_without_rho(ctx, m):
    """sdice_spearman_dev on resident vectors: with rho it equals the host call bit for bit; without it (NULL) the other
    five outputs do"""
    from splicedice_amd.engine import spearman_order
    ps, cols, _ = table(m)
    x = covariate(m, "tied")
    host = ctx.spearman(ps, cols, x)
    sc, xg = spearman_order(cols, x)
    n = ps.shape[0]
    d_ps, d_cols, d_xg = ctx.to_device(ps, np.float32), ctx.to_device(sc, np.int32), ctx.to_device(xg, np.int32)
    dts = dict(SP.FIELDS)
    for with_rho in (True, False):
        out = {name: ctx.to_device(np.full(n, 7, dts[name]), dts[name]) for name in OUTS if with_rho or name != "rho"}
        ctx.spearman_dev(d_ps, d_cols, d_xg, out)
        ctx.sync()
        for name, v in out.items():
            assert np.array_equal(v.to_host().view(np.uint8), host[name].view(np.uint8)), (name, with_rho)
            v.free()
    for a in (d_ps, d_cols, d_xg):
        a.free()


ERROR_CASES = ("m=2", "m=0", "m over the limit", "more columns than the table has", "index out of range", "negative index",
               "column listed twice", "xg starts at 1", "xg falls", "xg steps by 2", "xg negative")


@gpu
@pytest.mark.parametrize("case", ERROR_CASES)
def test_errors_leave_the_outputs_untouched(ctx, case):
    n, s, m = 3, 12, 5
    cols, xg = np.array([4, 0, 9, 2, 7]), np.array([0, 0, 1, 2, 2])
    if case == "m=2":
        m = 2
    elif case == "m=0":
        m = 0
    elif case == "m over the limit":
        m, s = M_LIMIT + 1, M_LIMIT + 2
        cols, xg = np.arange(m), np.arange(m)
    elif case == "more columns than the table has":
        m, s = 5, 4
        cols = np.array([0, 1, 2, 3, 3])
    elif case == "index out of range":
        cols[3] = s
    elif case == "negative index":
        cols[0] = -1
    elif case == "column listed twice":
        cols[4] = cols[1]
    elif case == "xg starts at 1":
        xg = xg + 1
    elif case == "xg falls":
        xg = np.array([0, 1, 0, 1, 2])
    elif case == "xg steps by 2":
        xg = np.array([0, 0, 2, 3, 3])
    else:
        xg = np.array([0, -1, 0, 1, 2])
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(SP.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    rc = RS.raw_call(ctx, "sdice_spearman", ps, (cols, xg, m), outs, OUTS)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "m over the limit":
        assert b"4096" in ctx.lib.sdice_last_error() and b"4097" in ctx.lib.sdice_last_error()
    # the context still works
    ok = ctx.spearman(np.tile(np.array([0.1, 0.2, 0.3, 0.3], np.float32), (2, 1)), [0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0])
    assert ok["tested"].tolist() == [1, 1]


@gpu
@pytest.mark.parametrize("case", ["m=2", "m over the limit", "more columns than the table has", "negative rows"])
def test_dev_errors_leave_the_outputs_untouched(ctx, case):
    """the _dev call checks the scalars before any launch"""
    n, s, m = 4, 10, 5
    if case == "m=2":
        m = 2
    elif case == "m over the limit":
        m, s = M_LIMIT + 1, M_LIMIT + 1
    elif case == "more columns than the table has":
        m, s = 6, 5
    rows = n
    d_ps = ctx.to_device(np.full((rows, s), 0.5, np.float32), np.float32)
    d_cols = ctx.to_device(np.arange(max(m, 1), dtype=np.int32) % s, np.int32)
    d_xg = ctx.to_device(np.zeros(max(m, 1), np.int32), np.int32)
    dts = dict(SP.FIELDS)
    out = {name: ctx.to_device(np.full(rows, 9, dts[name]), dts[name]) for name in OUTS}
    rc = ctx.lib.sdice_spearman_dev(ctx.h, -1 if case == "negative rows" else n, s, d_ps.ptr, d_cols.ptr, d_xg.ptr, m,
                                    *[out[name].ptr for name in OUTS])
    assert rc == -1, case
    ctx.sync()
    for name in OUTS:
        assert np.array_equal(out[name].to_host(), np.full(rows, 9, dts[name])), (case, name)
    for a in (d_ps, d_cols, d_xg, *out.values()):
        a.free()


@gpu
def test_engine_refuses_a_bad_covariate(ctx):
    with pytest.raises(ValueError, match="finite"):
        ctx.spearman(np.zeros((2, 4), np.float32), [0, 1, 2], [1.0, np.nan, 2.0])
    with pytest.raises(ValueError, match="3 columns but 2"):
        ctx.spearman(np.zeros((2, 4), np.float32), [0, 1, 2], [1.0, 2.0])


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    """48 rows x 14 samples, 11 of them in the covariate file (one as NA, so 10 are used) in an order unlike the table's,
    with covariate ties"""
    rng = np.random.default_rng(707)
    n, s = 48, 14
    samples, _ = RS.ps_names(n, s)
    listed = [9, 2, 12, 0, 5, 7, 3, 11, 1, 6, 13]                # table columns in file order; 13 is the NA line
    age = {9: "31", 2: "45.5", 12: "31", 0: "62", 5: "1e1", 7: "45.5", 3: "58", 11: "-3", 1: "31", 6: "70.25", 13: "NA"}
    v = rng.integers(0, 1001, size=(n, s)) / 1000.0
    used = [j for j in listed if age[j] != "NA"]
    xs = np.array([float(age[j]) for j in used])
    v[:, used] = np.clip(v[:, used] * 0.5 + 0.25 + np.outer(rng.uniform(-1, 1, n), (xs - xs.mean()) / 120.0), 0, 1)
    v[:8] = np.round(v[:8] * 4) / 4                                                        # heavy ties
    text = np.where(rng.random((n, s)) < 0.1, "nan", np.char.mod("%.3f", v))
    text[8:11] = "0.500"                                                                    # constant rows stay in the table
    text[11:14, [j for j in used[2:]]] = "nan"                                              # two kept: rows dropped
    text[14, used] = np.char.mod("%.3f", (xs - xs.min()) / 100.0)                           # rho = +1
    text[15, used] = np.char.mod("%.3f", (xs.max() - xs) / 100.0)                           # rho = -1
    path, _, names = RS.write_ps_inputs(tmp_path, text)
    cov = tmp_path / "age.tsv"
    cov.write_text("".join(f"{samples[j]}\t{age[j]}\n" + ("\n" if j == 0 else "") for j in listed))
    matrix = text.astype(np.float64).astype(np.float32)
    return path, str(cov), names, matrix, np.array(used, np.int32), xs


def _run_cli(ctx, golden_dir, tmp_path, gtf):
    """-> (the command's file as lines of cells, the referee's table as lines of cells: n as an integer, float32 / float64
    cells as numpy str(), BH over the tested rows from the oracle, the GTF columns from the host annotation code)"""
    from splicedice_amd import compare_sample_sets as css, correlate
    table_path, cov, names, matrix, cols, x = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    correlate.run_with(argparse.Namespace(psiSPLICEDICE=table_path, covariate=cov, annotation=anno, outputFile=out), ctx=ctx)
    ref = SP.table_reference(matrix, *sorted_design(cols, x))
    keep = np.flatnonzero(ref["tested"])
    assert 38 <= keep.size < 48 and {8, 9, 10, 14, 15} <= set(keep.tolist()) and not {11, 12, 13} & set(keep.tolist())
    assert ref["rho"][14] == 1.0 and ref["rho"][15] == -1.0 and ref["p"][8] == 1.0
    q = O.bh_fdr(ref["p"][keep])
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    lines = ["event\tn\tmean\tmedian\trho\tp-value\tcorrected" + ("\tgene\toverlapping\ttranscript_id" if gtf else "")]
    for i, r in enumerate(keep):
        cells = [int(ref["n_kept"][r]), ref["mean"][r], ref["med"][r], np.float64(ref["rho"][r]), np.float64(ref["p"][r]),
                 np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + sfx[i])
    text = open(out).read()
    assert text.endswith("\n")
    return [ln.split("\t") for ln in text[:-1].split("\n")], [ln.split("\t") for ln in lines]


@gpu
@pytest.mark.parametrize("gtf", [False, True])
def test_cli_correlate_byte_for_byte(ctx, golden_dir, tmp_path, gtf):
    """`correlate` end to end on 48 rows x 10 usable samples: the output file equals the referee's table formatted with
    numpy str(), plus BH from the oracle, byte for byte.  rho and p are the correctly rounded float64 here because the
    library forms them in double-double arithmetic for rows of at most 64 kept samples."""
    got, want = _run_cli(ctx, golden_dir, tmp_path, gtf)
    rows = [(g, w) for g, w in zip(got, want) if g != w]
    print(f"rows that differ: {len(rows)} of {len(want) - 1}")
    for g, w in rows:
        print("got ", "\t".join(g), "\nwant", "\t".join(w))
    assert len(got[1]) == (10 if gtf else 7)
    assert got == want


def test_correlate_under_the_launcher_is_refused(tmp_path, monkeypatch, capsys):
    """world > 1: one clear line and exit status 1, before a file is read or a device is opened"""
    import types
    from splicedice_amd import correlate, mgpu
    monkeypatch.setattr(mgpu, "_launcher", types.SimpleNamespace(world=2, rank=0, local_rank=0, root=True))

    def no_context(*a, **k):
        raise AssertionError("a Context was created")
    monkeypatch.setattr(correlate, "Context", no_context)
    args = argparse.Namespace(psiSPLICEDICE=str(tmp_path / "absent_allPS.tsv"), covariate=str(tmp_path / "absent.tsv"),
                              annotation="", outputFile=str(tmp_path / "x.tsv"))
    with pytest.raises(SystemExit) as e:
        correlate.run_with(args)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.strip() == correlate.MULTI_RANK_REFUSAL and "\n" not in err.strip() and "multi-rank launcher" in err
    assert not (tmp_path / "x.tsv").exists()
