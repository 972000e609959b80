"""sdice_signedrank (Wilcoxon signed-rank test over matched column pairs) and compare_sample_sets --paired against the
referee (tests/signedrank_referee.py: integers, one mpmath square root, mpmath erfc) and numpy.

Bars: tested mask, medians, means and delta bit-exact against numpy; z within 1e-12 relative of the
referee and exactly 0 where the referee's is 0; p within 1e-9 relative wherever the referee's p >= 1e-280 and under 2e-280
below that; such cells are at most 1 % of a table's tested rows (asserted).  No float32 field is compared by value only:
zero means and medians carry numpy's sign (+0.0 also of -0.0 values: np.median ends in np.mean, which starts from 0).

The tables mix every row kind of KINDS at every pair count of MS, with shuffled columns; the table builders and their
references are cached and shared with tests/test_gpu_signedrank_sweeps.py.  Tests without the gpu mark check on the CPU
that the tables are what they claim."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import signedrank_referee as SR  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import P_FLOOR, P_RTOL, draw_pairs  # noqa: E402

gpu = pytest.mark.gpu

Z_RTOL = 1e-12
M_LIMIT = 4096                      # pairs a call accepts (include/sdice.h)
# every dispatch and lane-group edge: a lane per row with 4 and 8 registers a side, groups of 16, 32 and 64 lanes, the
# workgroup kernel from 65, its LDS sizes
MS = (3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 1024, 1025, 4096)
KINDS = ("grid", "off-grid", "grid with NaNs", "off-grid with NaNs", "two kept pairs", "30 % equal pairs", "all pairs equal",
         "one sign", "equal |d|", "signed zeros", "subnormal differences")
PER_KIND = 20
F32 = ("med1", "med2", "mean1", "mean2", "delta")
OUTS = ("tested", "p", "z") + F32


def _base(rng, m, grid):
    """the two sides of a row before its kind is applied: uniform values, side 1 shifted by what moves z by a draw from
    -5..5 (the differences of two uniforms have a standard deviation of 0.41), so p stays far above the floor at any m"""
    shift = rng.uniform(-5.0, 5.0) * 0.41 / np.sqrt(m)
    x, y = rng.random(m) + shift, rng.random(m)
    if grid:
        return ((np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32) for v in (x, y))     # float32(k / 1000.0)
    x, y = ((v * 1.7 - 0.3).astype(np.float32) + rng.random(m, dtype=np.float32) * np.float32(1e-3) for v in (x, y))
    dup = rng.integers(0, m, size=(max(1, m // 6), 2))       # exact duplicates: of a whole pair (equal differences) ...
    x[dup[:, 0]], y[dup[:, 0]] = x[dup[:, 1]], y[dup[:, 1]]
    dup = rng.integers(0, m, size=(max(1, m // 8), 2))       # ... and of single values across the sides
    x[dup[:, 0]] = y[dup[:, 1]]
    return x, y


def make_row(rng, kind, v, m, a, b, s):
    """one row of KINDS[kind], variant v (grid and off-grid, or the two signs, alternate with v where the kind has both)"""
    name = KINDS[kind]
    grid = name.startswith("grid") or (not name.startswith("off-grid") and v % 2 == 0)
    x, y = _base(rng, m, grid)
    if name.endswith("with NaNs"):
        x[rng.random(m) < 0.06] = np.nan
        y[rng.random(m) < 0.06] = np.nan
    elif name == "two kept pairs":
        gone = rng.permutation(m)[2:]
        side = rng.integers(0, 3, size=gone.size)
        x[gone[side != 1]] = np.nan
        y[gone[side != 0]] = np.nan
    elif name == "30 % equal pairs":
        sel = rng.random(m) < 0.3
        y[sel] = x[sel]
    elif name == "all pairs equal":
        y = x.copy()
    elif name == "one sign":
        lo, hi = np.minimum(x, y), np.maximum(x, y)
        x, y = (hi, lo) if ((v + 1) // 2) % 2 == 0 else (lo, hi)      # v = 0, 1, 2, 3: grid +, off-grid -, grid -, off-grid +
    elif name == "equal |d|":
        sign = rng.choice([-1, 1], size=m)
        if grid:
            ky = rng.integers(60, 941, size=m)
            kx = ky + sign * int(rng.integers(1, 60))
            x, y = ((k / 1000.0).astype(np.float32) for k in (kx, ky))
        else:
            y = rng.integers(2, 61, size=m).astype(np.float32)
            x = y + sign.astype(np.float32) * np.float32(0.5)
    elif name == "signed zeros":
        sel = rng.permutation(m)[: max(1, m // 4)]
        x[sel] = rng.choice(np.array([-0.0, 0.0], np.float32), size=sel.size)
        y[sel] = -x[sel]
        y[sel[1::3]] = x[sel[1::3]]
    elif name == "subnormal differences":
        x, y = (rng.integers(1, 5001, size=m).astype(np.uint32).view(np.float32) *
                rng.choice(np.array([-1, 1], np.float32), size=m) for _ in range(2))       # multiples of 2^-149 of either sign
    row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)       # would show if a spare column were read
    row[a], row[b] = x, y
    return row


def kind_counts(m):
    """rows per kind.  From 1289 pairs up a row of one sign lies below the p floor (|z| = sqrt(3 n' / 2) or so), so there
    the kind has one row of each sign and the others have more rows: 2 cells under the floor stay inside 1 %"""
    if m < 1289:
        return [PER_KIND] * len(KINDS)
    return [2 if k == "one sign" else PER_KIND + 4 for k in KINDS]


@functools.lru_cache(maxsize=None)
def table(m):
    """-> (ps float32[rows, 2 m + 3], a, b, kind[rows]); the kinds interleaved, so that neighbouring rows (and the rows
    side by side in a wave) are of different kinds"""
    rng = np.random.default_rng(20250 + m)
    a, b, s = draw_pairs(rng, m)
    rows, kinds = [], []
    for v in range(max(kind_counts(m))):
        for k, cnt in enumerate(kind_counts(m)):
            if v < cnt:
                rows.append(make_row(rng, k, v, m, a, b, s))
                kinds.append(k)
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, a, b, np.array(kinds)


@functools.lru_cache(maxsize=None)
def reference(m):
    ps, a, b, _ = table(m)
    return SR.table_reference(ps, a, b)


def check(got, ref, label, floor_share=True):
    """asserts every bar -> dict(tested, below, z_err, p_err)"""
    t = RS.check_common(got, ref, F32, ("p", "z"), label)
    z, zr = got["z"][t], ref["z"][t]
    assert np.all(z[zr == 0] == 0), label
    err_z = np.abs(z - zr) / np.where(zr != 0, np.abs(zr), 1.0)
    out = dict(tested=int(t.sum()), z_err=float(err_z.max()) if err_z.size else 0.0)
    print(f"{label}: rows {t.size} tested {out['tested']} worst z rel {out['z_err']:.3g}", end=" ")
    assert np.all(err_z <= Z_RTOL), (label, out["z_err"])
    out["below"], out["p_err"] = RS.check_p(got["p"][t], ref["p"][t], label)
    if floor_share:
        RS.check_floor_share(out["tested"], out["below"], label)
    return out


# ---------------------------------------------------------------- the tables, on the CPU
@pytest.mark.parametrize("m", MS)
def test_tables_are_what_they_claim(m):
    """every kind at every pair count is what its name says, by the referee alone; the cells under the p floor stay
    inside 1 % of the tested rows (from 1289 pairs up: the two rows of one sign), checked here before any GPU run"""
    ps, a, b, kind = table(m)
    ref = reference(m)
    assert np.unique(np.concatenate([a, b])).size == 2 * m and ps.shape[1] == 2 * m + 3
    if m >= 8:
        assert (a < b).any() and (a > b).any() and (np.diff(a) < 0).any() and (np.diff(a) > 0).any()
    assert 190 <= ps.shape[0] <= 260 and set(kind.tolist()) == set(range(len(KINDS)))
    x, y = ps[:, a], ps[:, b]
    kept = ~(np.isnan(x) | np.isnan(y))
    for r in range(ps.shape[0]):
        name = KINDS[kind[r]]
        nk = int(kept[r].sum())
        assert ref["tested"][r] == (nk >= 3), (r, name)
        if name == "two kept pairs":
            assert nk == min(m, 2) and not ref["tested"][r]
        if name.startswith("grid"):
            assert ref["grid"][r] or not ref["tested"][r]
        if name.startswith("off-grid") or name == "subnormal differences":
            assert not ref["grid"][r]
        if name.endswith("with NaNs") and m >= 64:
            assert nk < m
        if not ref["tested"][r]:
            continue
        d = (x[r] - y[r])[kept[r]]
        if name == "all pairs equal":
            assert ref["npairs"][r] == 0 and ref["z"][r] == 0.0 and ref["p"][r] == 1.0
        if name == "one sign":
            assert (d >= 0).all() or (d <= 0).all()
        if name == "equal |d|":
            assert abs(abs(ref["z"][r]) - abs(int((d > 0).sum()) - int((d < 0).sum())) / np.sqrt(m)) < 1e-9
        if name == "signed zeros":
            assert (np.signbit(x[r]) != np.signbit(y[r]))[(x[r] == 0) & (y[r] == 0)].any() and ref["npairs"][r] < nk
        if name == "subnormal differences":
            assert (np.abs(d[d != 0]) < np.finfo(np.float32).tiny).all() and ref["npairs"][r] > 0
    t = ref["tested"].astype(bool)
    for name in ("grid", "off-grid"):        # both kinds of row are tested rows of every table
        assert (t & (ref["grid"] == (name == "grid"))).sum() >= 40
    below = int((ref["p"][t] < P_FLOOR).sum())
    assert below <= 0.01 * t.sum() and (below == 0) == (m < 1289), (m, below, int(t.sum()))
    if m >= 32:
        assert np.unique(ref["z"][t]).size > 100


# ---------------------------------------------------------------- the library
@gpu
@pytest.mark.parametrize("m", MS)
def test_signedrank_parity(ctx, m):
    """every row kind, mixed in one table, at every dispatch and lane-group edge"""
    ps, a, b, _ = table(m)
    check(ctx.signedrank(ps, a, b), reference(m), f"m={m}")


@gpu
def test_equal_printed_differences_tie(ctx):
    """the reason for the grid rule, on the device: 0.3 - 0.2 and 0.2 - 0.1 tie on a row of 3-decimal values and do not
    once one value of the row is off the grid"""
    f = np.float32
    ps = np.array([[0.3, 0.2, 0.9, 0.2, 0.1, 0.5],
                   [0.3, 0.2, 0.9, 0.2, 0.1, f(0.5) + f(1e-6)]], dtype=np.float32)
    a, b = np.array([0, 1, 2], np.int32), np.array([3, 4, 5], np.int32)
    ref = SR.table_reference(ps, a, b)
    assert ref["grid"].tolist() == [True, False] and ref["z"][0] != ref["z"][1]
    check(ctx.signedrank(ps, a, b), ref, "tie rule")


@gpu
def test_all_equal_rows_and_tiny_calls(ctx):
    """every kept pair equal: tested, z = 0, p = 1 (scipy: NaN); m = 1 and 2 test nothing; n = 0 is a no-op"""
    ps = np.array([[0.5] * 8, [0.25, 0.5, 0.75, np.nan] * 2, [0.1234567] * 8, [1.0, 0.0, 0.5, 0.25] * 2], dtype=np.float32)
    a, b = np.arange(0, 4, dtype=np.int32), np.arange(4, 8, dtype=np.int32)
    got = ctx.signedrank(ps, a, b)
    assert got["tested"].tolist() == [1, 1, 1, 1] and got["z"].tolist() == [0.0] * 4 and got["p"].tolist() == [1.0] * 4
    check(got, SR.table_reference(ps, a, b), "all equal")
    for m in (1, 2):
        got = ctx.signedrank(ps, a[:m], b[:m])
        assert not any(got[name].any() for name in OUTS)
    empty = ctx.signedrank(np.zeros((0, 8), np.float32), a, b)
    assert all(empty[name].shape == (0,) for name in OUTS)


@gpu
@pytest.mark.parametrize("case", ["m=0", "m over the limit", "index out of range", "negative index", "twice in one list",
                                  "in both lists"])
def test_errors_leave_the_outputs_untouched(ctx, case):
    n, s = 3, 12
    a, b = np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7])
    m = 4
    if case == "m=0":
        m = 0
    elif case == "m over the limit":
        m, s = M_LIMIT + 1, 2 * M_LIMIT + 2
        a, b = np.arange(m), np.arange(m, 2 * m)
    elif case == "index out of range":
        b[3] = s
    elif case == "negative index":
        a[0] = -1
    elif case == "twice in one list":
        a[3] = a[1]
    else:
        b[2] = a[0]
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(SR.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    rc = RS.raw_call(ctx, "sdice_signedrank", ps, (a, b, m), outs, OUTS)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "m over the limit":
        assert b"4096" in ctx.lib.sdice_last_error() and b"4097" in ctx.lib.sdice_last_error()
    # the context still works
    ok = ctx.signedrank(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5])
    assert ok["tested"].tolist() == [1, 1]


@gpu
def test_engine_refuses_pair_lists_of_two_lengths(ctx):
    with pytest.raises(ValueError, match="one length"):
        ctx.signedrank(np.zeros((2, 9), np.float32), [0, 1, 2], [3, 4])


# ---------------------------------------------------------------- command line
def _run_cli_paired(ctx, golden_dir, tmp_path, gtf):
    """-> (the command's file as lines of cells, the referee's table as lines of cells: float32 / float64 cells as numpy
    str(), BH over the tested rows from the oracle, the GTF columns from the host annotation code)"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, names, matrix, a, b = RS.write_paired_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    args = argparse.Namespace(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=True,
                              annotation=anno, outputFile=out)
    css.run_with(args, ctx=ctx)
    ref = SR.table_reference(matrix, a, b)
    keep = np.flatnonzero(ref["tested"])
    assert 30 <= keep.size < 40 and {8, 9, 10} <= set(keep.tolist()) and not {11, 12, 13} & set(keep.tolist())
    q = O.bh_fdr(ref["p"][keep])
    header = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected"
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    lines = [header + ("\tgene\toverlapping\ttranscript_id" if gtf else "")]
    for i, r in enumerate(keep):
        cells = [ref["mean1"][r], ref["mean2"][r], ref["med1"][r], ref["med2"][r], ref["delta"][r], ref["p"][r], np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + sfx[i])
    text = open(out).read()
    assert text.endswith("\n")
    return [ln.split("\t") for ln in text[:-1].split("\n")], [ln.split("\t") for ln in lines]


@gpu
@pytest.mark.parametrize("gtf", [False, True])
def test_cli_paired(ctx, golden_dir, tmp_path, gtf):
    """compare_sample_sets --paired on 40 rows x 6 pairs, manifest order unlike the table's: header, rows, event names,
    the float32 cells and the GTF columns are the referee's strings; p-value and corrected are repr round-trips within the
    parity bar (1e-9 relative) of the referee's p and the oracle's BH of it"""
    got, want = _run_cli_paired(ctx, golden_dir, tmp_path, gtf)
    assert got[0] == want[0] and len(got) == len(want)
    for g, w in zip(got[1:], want[1:]):
        assert g[:6] == w[:6] and g[8:] == w[8:] and len(g) == (11 if gtf else 8)
        for cell, ref in zip(g[6:8], w[6:8]):
            assert str(np.float64(float(cell))) == cell
            assert abs(float(cell) - float(ref)) <= P_RTOL * float(ref), (g, w)


@gpu
@pytest.mark.parametrize("gtf", [False, True])
def test_cli_paired_byte_for_byte(ctx, golden_dir, tmp_path, gtf):
    """the same run, every byte: the output file equals the referee's table formatted with numpy str(), plus BH from the
    oracle.  p-value is erfc to the last bit here because the library evaluates it in double-double arithmetic wherever
    p >= 2.2e-5 (x^2 = z^2 / 2 <= 9; six pairs cannot leave that range: |z| <= sqrt 6); with the library erfc alone 25 of
    the 37 rows differed in the last printed digit of p-value or corrected."""
    got, want = _run_cli_paired(ctx, golden_dir, tmp_path, gtf)
    rows = [(g, w) for g, w in zip(got, want) if g != w]
    worst = [max((abs(float(g[c]) - float(w[c])) / float(w[c]) for g, w in rows if g[:6] == w[:6]), default=0.0) for c in (6, 7)]
    print(f"rows that differ: {len(rows)} of {len(want) - 1}; worst relative difference p-value {worst[0]:.3g} corrected {worst[1]:.3g}")
    for g, w in rows:
        print("got ", "\t".join(g), "\nwant", "\t".join(w))
    assert got == want


@gpu
def test_cli_without_the_flag_is_unchanged(ctx, golden_dir, tmp_path):
    """the golden two-set run, with paired absent and with paired=False: the same bytes, and the golden's cells by the rule
    of tests/test_gpu_cli.py (float32 cells as strings, p-value and corrected to 1e-6 relative)"""
    from splicedice_amd import compare_sample_sets as css
    d = os.path.join(golden_dir, "compare")
    outs = []
    for extra in ({}, dict(paired=False, moreManifests=None)):
        outs.append(str(tmp_path / f"cmp{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "in_allPS.tsv"), manifest1=os.path.join(d, "m1.tsv"),
                                        manifest2=os.path.join(d, "m2.tsv"), annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
    got = [ln.rstrip("\n").split("\t") for ln in open(outs[1])]
    want = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(d, "expected_out.tsv"))]
    assert len(got) == len(want) and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert g[:6] == w[:6]
        np.testing.assert_allclose([float(x) for x in g[6:]], [float(x) for x in w[6:]], rtol=1e-6)
