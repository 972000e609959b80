"""sdice_ks (the two-sample Kolmogorov-Smirnov test) and compare_sample_sets --ks against the referee (tests/ks_referee.py:
M by its definition, D as a Fraction, the exact p by the path recurrence in Python ints, the asymptotic p by mpmath at 50
digits), numpy and the rank-sum call.

Bars: tested mask, medians, means and delta bit-exact against numpy, and bit-exact against ctx.ranksum on the same lists
on the rows both calls test (with the one licence tests/test_gpu_strata.py documents: sdice_ranksum reports np.median by
value and returns -0.0 for the median of an even count of -0.0 values where numpy, and this call, return +0.0, so a zero
median or zero delta of the plain call that differs from numpy's in sign alone is let through); D bit-exact against
float(Fraction(M, n1' n2')); p within 1e-9 relative wherever the referee's p >= 1e-280 and under 2e-280 below that
(rank_support.check_p), such cells at most 1 % of a table's tested rows; the exact marks equal to the referee's
eligibility, and where a mark is 1 the p equal as float64 to float(Fraction); every slot 0 where a row is not tested.

The tables (tests/ks_fixtures.py) mix every row kind, each on 3-decimal values and on off-grid float32 values, at every
total column count that changes the kernel or its lane-group width; tests/test_ks_cpu.py checks on the CPU that they are
what they claim."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_fixtures as KF  # noqa: E402
import ks_referee as KR  # noqa: E402
import rank_support as RS  # noqa: E402
from ks_fixtures import F32, OUTS  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import same_f32  # noqa: E402

gpu = pytest.mark.gpu
GROUP_LIMIT = 4096                  # columns of one group (include/sdice.h)


def check(got, ref, label, floor_share=True, plain=None, quiet=False):
    """asserts every bar -> dict(tested, below, p_err, exact); plain: ctx.ranksum's result on the same lists"""
    t = RS.check_common(got, ref, F32, OUTS, label)
    if plain is not None:
        for name in F32:
            both = t & plain["tested"].astype(bool)
            unlike = both & ~same_f32(got[name], plain[name])
            # the one licence: where the plain call itself departs from numpy, in the sign of a zero median (or of the
            # delta of two zero medians), this call keeps numpy's zero
            excused = ~same_f32(plain[name], ref[name]) & (plain[name] == 0) & (ref[name] == 0) & (name in ("med1", "med2", "delta"))
            assert not (unlike & ~excused).any(), (label, name, "unlike the rank-sum call", np.flatnonzero(unlike & ~excused)[:5])
        assert np.array_equal(plain["tested"], ref["tested"]), label          # (both calls test the same rows)
    RS.assert_same_bits(got["d"], ref["d"], (label, "d"))
    assert got["exact"].dtype == np.uint8 and np.array_equal(got["exact"], ref["exact"]), (label, "exact marks")
    ex = ref["exact"].astype(bool)
    RS.assert_same_bits(got["p"][ex], ref["p"][ex], (label, "exact p"))
    out = dict(tested=int(t.sum()), exact=int(ex.sum()))
    out["below"], out["p_err"] = RS.check_p(got["p"][t], ref["p"][t], label, quiet)
    if floor_share:
        RS.check_floor_share(out["tested"], out["below"], label)
    return out


def dev_call(ctx, d_ps, g1, g2, n, exact, skip=()):
    """the _dev entry point on a resident table (or a view of it) -> host copies of the outputs; skip: fields left out"""
    from splicedice_amd.engine import KS_FIELDS, field_shapes
    held = [ctx.to_device(v, np.int32) for v in (g1, g2)]
    out = {name: ctx.empty(*sd) for name, sd in field_shapes(KS_FIELDS, n).items() if name not in skip}
    try:
        ctx.ks_dev(d_ps, *held, out, exact)
        ctx.sync()
        return {name: a.to_host() for name, a in out.items()}
    finally:
        for a in (*held, *out.values()):
            a.free()


def dev_table(ctx, ps, g1, g2, exact, skip=()):
    d_ps = ctx.to_device(ps, np.float32)
    try:
        return dev_call(ctx, d_ps, g1, g2, ps.shape[0], exact, skip)
    finally:
        d_ps.free()


# ---------------------------------------------------------------- the library
@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_ks_parity(ctx, entry):
    """every row kind, mixed in one table, at every total: both kernels, every lane-group width, 64 | 65; exact asked for"""
    worst = dict(p_err=0.0, tested=0, below=0, exact=0)
    for total in KF.TOTALS:
        n1, n2 = KF.split(total)
        ps, g1, g2, _ = KF.table(n1, n2)
        got = ctx.ks(ps, g1, g2, exact=True) if entry == "host" else dev_table(ctx, ps, g1, g2, True)
        out = check(got, KF.reference(n1, n2), f"total={total} {entry}", plain=ctx.ranksum(ps, g1, g2), quiet=True)
        worst["p_err"] = max(worst["p_err"], out["p_err"])
        for k in ("tested", "below", "exact"):
            worst[k] += out[k]
    print(f"{entry}: {len(KF.TOTALS)} tables, {worst}")
    assert worst["exact"] > 300 and worst["tested"] - worst["exact"] > 300


@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_without_exact_every_mark_is_0(ctx, entry):
    """want_exact = 0: the same table with every mark 0 and the asymptotic p; and on the rows that are not exact in either
    mode the two modes' p is bit for bit the same"""
    for total in KF.TOTALS:
        n1, n2 = KF.split(total)
        ps, g1, g2, _ = KF.table(n1, n2)
        ref = KF.reference(n1, n2, 2, None, False)
        assert not ref["exact"].any() and np.array_equal(ref["p"], ref["p_asym"])
        if entry == "host":
            got, with_exact = ctx.ks(ps, g1, g2), ctx.ks(ps, g1, g2, exact=True)
        else:
            got, with_exact = dev_table(ctx, ps, g1, g2, False), dev_table(ctx, ps, g1, g2, True)
        check(got, ref, f"total={total} {entry} asymptotic", quiet=True)
        rest = with_exact["exact"] == 0
        RS.assert_same_bits(with_exact["p"][rest], got["p"][rest], (total, "p of the rows not exact in either mode"))
        for name in ("tested", "d") + F32:
            RS.assert_same_bits(with_exact[name], got[name], (total, name))
    # d and exact may be left out of a _dev call that does not ask for exact p
    ps, g1, g2, _ = KF.table(*KF.split(40))
    lean = dev_table(ctx, ps, g1, g2, False, skip=("d", "exact"))
    full = ctx.ks(ps, g1, g2)
    assert set(lean) == set(OUTS) - {"d", "exact"}
    for name in lean:
        RS.assert_same_bits(lean[name], full[name], ("without d and exact", name))


@gpu
@pytest.mark.parametrize("total", [9, 40, 66])
def test_row_slices(ctx, total):
    """views ps[a:b] of a resident table at odd a and b, and the host call on the same slices"""
    n1, n2 = KF.split(total)
    ps, g1, g2, _ = KF.table(n1, n2, 8)
    rows, width = ps.shape
    want = ctx.ks(ps, g1, g2, exact=True)
    check(want, KF.reference(n1, n2, 8), f"total={total} 8 per kind", quiet=True)
    d_ps = ctx.to_device(ps, np.float32)
    try:
        for a, b in ((1, rows), (3, 70), (65, rows - 1), (rows - 1, rows)):
            cut = dev_call(ctx, d_ps.offset(a * width, (b - a, width)), g1, g2, b - a, True)
            host = ctx.ks(ps[a:b], g1, g2, exact=True)
            for name in OUTS:
                RS.assert_same_bits(cut[name], want[name][a:b], (total, a, b, name, "_dev"))
                RS.assert_same_bits(host[name], want[name][a:b], (total, a, b, name, "host"))
    finally:
        d_ps.free()


@gpu
@pytest.mark.parametrize("n1,n2", [(1024, 1024), (4096, 4096), (4096, 3), (3, 4096)])
def test_large_groups(ctx, n1, n2):
    """the workgroup kernel's largest sizes and most lopsided lists, a handful of rows each"""
    ps, g1, g2, _ = KF.table(n1, n2, 2, KF.LARGE_KINDS)
    ref = KF.reference(n1, n2, 2, KF.LARGE_KINDS)
    assert ref["tested"].sum() >= 8
    check(ctx.ks(ps, g1, g2, exact=True), ref, f"{n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))


@gpu
def test_swapping_the_groups_keeps_d_and_p(ctx):
    for total in (7, 16, 40, 64, 65, 129):
        n1, n2 = KF.split(total)
        ps, g1, g2, _ = KF.table(n1, n2)
        got, swapped = ctx.ks(ps, g1, g2, exact=True), ctx.ks(ps, g2, g1, exact=True)
        for name in ("tested", "p", "d", "exact"):
            RS.assert_same_bits(swapped[name], got[name], (total, name))
        assert np.all(same_f32(swapped["med1"], got["med2"])) and np.all(same_f32(swapped["mean2"], got["mean1"]))


@gpu
def test_the_hand_case_and_tiny_calls(ctx):
    """x = [1, 1, 1], y = [1, 1, 1, 2]: M = 3, D = 0.25 (a mid-run evaluation would report 1); lists too short for any row
    to be tested give zeros; n = 0 is a no-op"""
    row = np.array([[1, 1, 1, 1, 1, 1, 2, 9]], np.float32)
    for exact in (False, True):
        got = ctx.ks(row, [0, 1, 2], [3, 4, 5, 6], exact=exact)
        assert got["tested"][0] == 1 and got["d"][0] == 0.25 and got["exact"][0] == int(exact)
        want = 1.0 if exact else KR.asymptotic_p(3, 3, 4)
        assert abs(got["p"][0] - want) <= RS.P_RTOL * want
    ps = np.tile(np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], np.float32), (5, 1))
    for g1, g2 in (([0, 1], [2, 3, 4]), ([0], [1]), ([0, 1, 2, 3], [4, 5])):
        for exact in (False, True):
            got = ctx.ks(ps, g1, g2, exact=exact)
            assert not any(got[name].any() for name in OUTS)
    got = ctx.ks(ps, [0, 1, 2], [3, 4, 5], exact=True)
    assert got["tested"].tolist() == [1] * 5 and got["d"].tolist() == [1.0] * 5 and got["p"].tolist() == [0.1] * 5
    empty = ctx.ks(np.zeros((0, 7), np.float32), [0, 1, 2], [3, 4, 5])
    assert all(empty[name].shape == (0,) for name in OUTS)


ERROR_CASES = ("n1 0", "n2 0", "n1 4097", "column in both lists", "column twice in one list", "index equal to s",
               "negative index", "more columns than the table", "exact asked for without its array")
DEV_CASES = ("n1 0", "n2 0", "n1 4097", "more columns than the table", "exact asked for without its array")


def _error_call(ctx, case, dev):
    """-> (return code, outputs after, outputs before)"""
    n, s = 3, 12
    g1, g2 = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6, 7], np.int32)
    n1, n2, want_exact = 4, 4, 1
    if case == "n1 0":
        n1 = 0
    elif case == "n2 0":
        n2 = 0
    elif case == "n1 4097":
        n1, s = GROUP_LIMIT + 1, GROUP_LIMIT + 1 + 8
        g1 = np.arange(8, 8 + n1, dtype=np.int32)
    elif case == "column in both lists":
        g2[2] = g1[0]
    elif case == "column twice in one list":
        g1[3] = g1[1]
    elif case == "index equal to s":
        g2[3] = s
    elif case == "negative index":
        g1[0] = -1
    elif case == "more columns than the table":
        s = 7
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(KR.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    null_exact = case == "exact asked for without its array"
    if not dev:
        held = [np.ascontiguousarray(ps), g1, g2]
        ptr = lambda a: a.ctypes.data                          # noqa: E731
        rc = ctx.lib.sdice_ks(ctx.h, n, s, ptr(held[0]), ptr(g1), n1, ptr(g2), n2, want_exact,
                              *[None if (x == "exact" and null_exact) else ptr(outs[x]) for x in OUTS])
        return rc, outs, before
    held = [ctx.to_device(v, v.dtype) for v in (ps, g1, g2)] + [ctx.to_device(outs[x], outs[x].dtype) for x in OUTS]
    try:
        rc = ctx.lib.sdice_ks_dev(ctx.h, n, s, held[0].ptr, held[1].ptr, n1, held[2].ptr, n2, want_exact,
                                  *[None if (x == "exact" and null_exact) else a.ptr for x, a in zip(OUTS, held[3:])])
        ctx.sync()
        return rc, {x: a.to_host() for x, a in zip(OUTS, held[3:])}, before
    finally:
        for a in held:
            a.free()


@gpu
@pytest.mark.parametrize("case", ERROR_CASES)
def test_errors_leave_the_outputs_untouched(ctx, case):
    """SDICE_ERR_ARG before any launch, a message, outputs untouched, through the host call; through the _dev call the
    cases it can see (the counts: the lists are device memory there)"""
    rc, outs, before = _error_call(ctx, case, dev=False)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    message = ctx.lib.sdice_last_error()
    assert message and b"sdice_ks" in message
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "n1 4097":
        assert b"4096" in message and b"4097" in message
    if case in DEV_CASES:
        rc, outs, before = _error_call(ctx, case, dev=True)
        assert rc == -1 and ctx.lib.sdice_last_error(), case
        for x in outs:
            assert np.array_equal(outs[x], before[x]), (case, x, "dev")
    # the context still works
    ok = ctx.ks(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5])
    assert ok["tested"].tolist() == [1, 1] and ok["d"].tolist() == [0.0, 0.0] and ok["p"].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    """60 rows x (8 v 9) samples + 2 samples outside the manifests; the manifests' order is not the table's.  Shifted rows,
    rows switched on in a part of set 1 (equal medians, D large), heavy ties, all-equal rows, rows with a starved set"""
    rng = np.random.default_rng(1933)
    n, s = 60, 19
    samples, _ = RS.ps_names(n, s)
    set1 = np.array([0, 2, 4, 6, 8, 10, 12, 14])
    set2 = np.array([1, 3, 5, 7, 9, 11, 13, 15, 16])
    v = 0.05 + 0.1 * rng.random((n, s))
    v[:, set1] += 0.1 * rng.standard_normal((n, 1))
    v[20:40][:, set1[:3]] += 0.8                                                          # switched on in three samples of set 1
    v = np.clip(v, 0, 1)
    v[:10] = np.round(v[:10] * 5) / 5                                                    # heavy ties
    text = np.where(rng.random((n, s)) < 0.08, "nan", np.char.mod("%.3f", v))
    text[10:13] = "0.500"                                                                 # all-equal rows stay in the table
    text[13:16][:, set2[1:]] = "nan"                                                      # one value left in set 2: rows dropped
    path, (m1, m2), names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in set1[::-1]], "A"),
                                                             ([samples[j] for j in rng.permutation(set2)], "B")])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, m1, m2, names, matrix, set1.astype(np.int32), set2.astype(np.int32)


@gpu
@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("exact", [False, True])
def test_cli_ks_byte_for_byte(ctx, golden_dir, tmp_path, exact, gtf):
    """compare_sample_sets --ks (with and without --exact, with and without -a) on 60 rows of 8 v 9: the file equals, byte
    for byte, the table formatted here from the referee's values (numpy's float32 cells, the referee's D and p, the
    oracle's BH of that p over the tested rows) with the writer's rules"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, names, matrix, g1, g2 = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(argparse.Namespace(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=False,
                                    exact=exact, strata=None, trend=False, ks=True, annotation=anno, outputFile=out), ctx=ctx)
    ref = KR.table_reference(matrix, g1, g2, exact)
    keep = np.flatnonzero(ref["tested"])
    assert 50 <= keep.size < 60 and {10, 11, 12} <= set(keep.tolist()) and not {13, 14, 15} & set(keep.tolist())
    assert ref["exact"][keep].all() == exact and (ref["p"][keep] >= RS.P_FLOOR).all()
    switched = [r for r in range(20, 40) if ref["tested"][r]]
    assert sum(abs(ref["delta"][r]) < 0.1 and ref["d"][r] >= 0.3 for r in switched) > 8      # what the D column is for
    q = O.bh_fdr(ref["p"][keep])
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    lines = ["event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tD\tp-value\tcorrected" + ("\tgene\toverlapping\ttranscript_id" if gtf else "")]
    for i, r in enumerate(keep):
        cells = [ref["mean1"][r], ref["mean2"][r], ref["med1"][r], ref["med2"][r], ref["delta"][r], np.float64(ref["d"][r]),
                 np.float64(ref["p"][r]), np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + sfx[i])
    want = "\n".join(lines) + "\n"
    got = open(out).read()
    diff = [(g, w) for g, w in zip(got.split("\n"), want.split("\n")) if g != w]
    print(f"exact={exact} gtf={gtf}: lines that differ {len(diff)} of {want.count(chr(10))}")
    for g, w in diff[:5]:
        print("got ", g, "\nwant", w)
    assert got == want


@gpu
def test_cli_on_an_empty_table_and_without_the_flag(ctx, golden_dir, tmp_path):
    """a table without rows gives the header alone; the golden two-set run with ks=False is what it is with the flag
    absent"""
    from splicedice_amd import compare_sample_sets as css
    samples, _ = RS.ps_names(0, 8)
    table = tmp_path / "empty_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(samples) + "\n")
    m = []
    for i, group in enumerate((samples[:4], samples[4:])):
        m.append(tmp_path / f"e{i}.tsv")
        m[-1].write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    out = str(tmp_path / "empty_out.tsv")
    css.run_with(argparse.Namespace(psiSPLICEDICE=str(table), manifest1=str(m[0]), manifest2=str(m[1]), ks=True, annotation="",
                                    outputFile=out), ctx=ctx)
    assert open(out).read() == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tD\tp-value\tcorrected\n"
    d = os.path.join(golden_dir, "compare")
    outs = []
    for extra in ({}, dict(ks=False)):
        outs.append(str(tmp_path / f"cmp{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "in_allPS.tsv"), manifest1=os.path.join(d, "m1.tsv"),
                                        manifest2=os.path.join(d, "m2.tsv"), annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    recorded = open(os.path.join(d, "expected_out_device.tsv"), "rb").read()
    assert open(outs[0], "rb").read() == recorded and open(outs[1], "rb").read() == recorded
