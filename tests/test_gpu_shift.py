"""sdice_shift (the Hodges-Lehmann shift with its confidence interval) and compare_sample_sets --shift against the referee
(tests/shift_referee.py: brute force over all differences, integers on the 3-decimal grid and float64 subtractions off it,
the rank from mpmath at 40 digits) and the rank-sum call.

Bars, without a tolerance anywhere: shift, lo and hi equal the referee's as float64 BITS, NaN where the referee has NaN;
rank equal as an integer; tested equal to the referee's and to ctx.ranksum's on the same lists; every slot of a row that
is not tested all-zero bits, also where the output held something else before the call.

The tables (tests/shift_fixtures.py) hold every row kind on 3-decimal values, off the grid and mixed, at every total
column count that changes the kernel or its lane-group width; tests/test_shift_cpu.py checks on the CPU that they are
what they claim and that no rank of theirs hangs on a rounding."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import shift_fixtures as SF  # noqa: E402
import shift_referee as SR  # noqa: E402
from shift_referee import OUTS  # noqa: E402

gpu = pytest.mark.gpu
GROUP_LIMIT = 4096                  # columns of one group (include/sdice.h)
F64 = ("shift", "lo", "hi")


def check(got, ref, label, plain=None):
    """asserts every bar -> dict(tested, nan, grid): the numbers of tested rows, of NaN triples and of tested grid rows"""
    assert got["tested"].dtype == np.uint8 and got["rank"].dtype == np.int32, label
    bad = np.flatnonzero(got["tested"] != ref["tested"])
    assert bad.size == 0, (label, "tested", bad[:5].tolist())
    if plain is not None:
        assert np.array_equal(got["tested"], plain["tested"]), (label, "tested unlike the rank-sum call's")
    t = ref["tested"].astype(bool)
    assert np.array_equal(got["rank"], ref["rank"]), (label, "rank", np.flatnonzero(got["rank"] != ref["rank"])[:5].tolist())
    nan = np.isnan(ref["shift"])
    for name in F64:
        assert got[name].dtype == np.float64, (label, name)
        assert np.array_equal(np.isnan(got[name]), nan) and np.array_equal(np.isnan(ref[name]), nan), (label, name, "NaN rows")
        RS.assert_same_bits(got[name][~nan], ref[name][~nan], (label, name), where=lambda r: np.flatnonzero(~nan)[r].tolist())
    for name in OUTS:
        assert not RS.bits(got[name][~t]).any(), (label, name, "a slot of a row that is not tested")
    return dict(tested=int(t.sum()), nan=int(nan.sum()), grid=int((ref["grid"].astype(bool) & t).sum()))


def dev_call(ctx, d_ps, g1, g2, n, conf=0.95):
    """the _dev entry point on a resident table (or a view of it), every output holding 0xA5 bytes before the call -> host
    copies of the outputs"""
    from splicedice_amd.engine import SHIFT_FIELDS, field_shapes
    held = [ctx.to_device(v, np.int32) for v in (g1, g2)]
    out = {name: ctx.empty(*sd).memset(0xA5) for name, sd in field_shapes(SHIFT_FIELDS, n).items()}
    try:
        ctx.shift_dev(d_ps, *held, out, conf)
        ctx.sync()
        return {name: a.to_host() for name, a in out.items()}
    finally:
        for a in (*held, *out.values()):
            a.free()


def dev_table(ctx, ps, g1, g2, conf=0.95):
    d_ps = ctx.to_device(ps, np.float32)
    try:
        return dev_call(ctx, d_ps, g1, g2, ps.shape[0], conf)
    finally:
        d_ps.free()


def call(ctx, entry, ps, g1, g2, conf=0.95):
    return ctx.shift(ps, g1, g2, conf) if entry == "host" else dev_table(ctx, ps, g1, g2, conf)


# ---------------------------------------------------------------- the library
@gpu
@pytest.mark.parametrize("flavour", SF.FLAVOURS)
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_shift_parity(ctx, entry, flavour):
    """every row kind at every total: both kernels, every lane-group width, 64 | 65; tables on the grid (the integer
    paths), off it and mixed"""
    total = dict(tested=0, nan=0, grid=0)
    for cols in SF.TOTALS:
        n1, n2 = SF.split(cols)
        ps, g1, g2, _ = SF.table(n1, n2, flavour)
        out = check(call(ctx, entry, ps, g1, g2), SF.reference(n1, n2, flavour), f"total={cols} {flavour} {entry}",
                    plain=ctx.ranksum(ps, g1, g2))
        for k in total:
            total[k] += out[k]
    print(f"{entry} {flavour}: {len(SF.TOTALS)} tables, {total}")
    assert total["tested"] > 400
    assert (total["grid"] == total["tested"]) if flavour == "grid" else (total["nan"] >= len(SF.TOTALS))
    assert flavour != "off" or total["grid"] == 0


@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_lists_of_unlike_lengths(ctx, entry):
    """3 v 61 and 61 v 3 (a lane group's longest list beside the shortest), 3 v 13 and 13 v 3, and 3 v 62 and 62 v 3 in the
    workgroup kernel"""
    for n1, n2 in SF.LOPSIDED:
        ps, g1, g2, _ = SF.table(n1, n2)
        out = check(call(ctx, entry, ps, g1, g2), SF.reference(n1, n2), f"{n1} v {n2} {entry}", plain=ctx.ranksum(ps, g1, g2))
        assert out["tested"] >= 15 and out["grid"] >= 5 and out["nan"] == 1


@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_levels(ctx, entry):
    """conf 0.5, 0.9, 0.95 and 0.99 in both kernels: the rank moves, the shift does not"""
    for cols in SF.LEVEL_TOTALS:
        n1, n2 = SF.split(cols)
        ps, g1, g2, _ = SF.table(n1, n2)
        ranks = []
        for conf in SF.LEVELS:
            ref = SF.reference(n1, n2, "mixed", 1, None, conf)
            check(call(ctx, entry, ps, g1, g2, conf), ref, f"total={cols} conf={conf} {entry}")
            ranks.append(ref["rank"][ref["tested"] == 1].astype(np.int64))
        assert all((a >= b).all() for a, b in zip(ranks, ranks[1:])) and (cols < 16 or (ranks[0] > ranks[-1]).any())
    with pytest.raises(ValueError):
        ctx.shift(ps, g1, g2, conf=1.0)


@gpu
@pytest.mark.parametrize("total", SF.SLICE_TOTALS)
def test_row_slices(ctx, total):
    """views ps[a:b] of a resident table at odd a and b, and the host call on the same slices"""
    n1, n2 = SF.split(total)
    ps, g1, g2, _ = SF.table(n1, n2, "mixed", 4)
    rows, width = ps.shape
    want = ctx.shift(ps, g1, g2)
    check(want, SF.reference(n1, n2, "mixed", 4), f"total={total} 4 per kind")
    d_ps = ctx.to_device(ps, np.float32)
    try:
        for a, b in ((1, rows), (3, 70), (65, rows - 1), (rows - 1, rows)):
            cut = dev_call(ctx, d_ps.offset(a * width, (b - a, width)), g1, g2, b - a)
            host = ctx.shift(ps[a:b], g1, g2)
            for name in OUTS:
                RS.assert_same_bits(cut[name], want[name][a:b], (total, a, b, name, "_dev"))
                RS.assert_same_bits(host[name], want[name][a:b], (total, a, b, name, "host"))
    finally:
        d_ps.free()


@gpu
@pytest.mark.parametrize("n1,n2", SF.LARGE)
def test_large_groups(ctx, n1, n2):
    """the workgroup kernel's largest sizes and most lopsided lists, a handful of rows on the grid and off it"""
    ps, g1, g2, what = SF.table(n1, n2, "mixed", 1, SF.LARGE_KINDS)
    ref = SF.reference(n1, n2, "mixed", 1, SF.LARGE_KINDS)
    out = check(ctx.shift(ps, g1, g2), ref, f"{n1} v {n2}", plain=ctx.ranksum(ps, g1, g2))
    assert out["tested"] >= len(what) - 2 and 3 <= out["grid"] <= out["tested"] - 3      # (6 % NaN can starve a group of 3)
    assert ref["rank"].max() > (1000 if n1 == n2 else 1)


@gpu
def test_swapping_the_groups_negates_and_swaps(ctx):
    for total in (6, 7, 16, 40, 64, 65, 129):
        n1, n2 = SF.split(total)
        ps, g1, g2, _ = SF.table(n1, n2)
        got, swapped = ctx.shift(ps, g1, g2), ctx.shift(ps, g2, g1)
        nan = np.isnan(got["shift"])
        assert np.array_equal(swapped["tested"], got["tested"]) and np.array_equal(swapped["rank"], got["rank"])
        for a, b in (("shift", "shift"), ("lo", "hi"), ("hi", "lo")):
            assert np.array_equal(np.isnan(swapped[a]), nan)
            RS.assert_same_bits(swapped[a][~nan], (-got[b] + 0.0)[~nan], (total, a, "is not minus", b))


@gpu
def test_the_hand_case_and_tiny_calls(ctx):
    """keys 100 200 300 400 v 50 100 150 at 95 %: (0.15, -0.05, 0.35), rank 1; 3 v 3 at 95 %: the clamp, the interval is
    the whole range; lists too short for any row to be tested give zeros; n = 0 is a no-op"""
    row = np.array([[0.1, 0.2, 0.3, 0.4, 0.05, 0.1, 0.15, 9]], np.float32)
    got = ctx.shift(row, [0, 1, 2, 3], [4, 5, 6])
    assert [got[k][0] for k in OUTS] == [1, 0.15, -0.05, 0.35, 1]
    got = ctx.shift(np.array([[0.3, 0.2, 0.3, 0.2, 0.1, 0.2]], np.float32), [0, 1, 2], [3, 4, 5])
    assert [got[k][0] for k in OUTS] == [1, 0.1, 0.0, 0.2, 1]            # (equal printed differences tie; 3 v 3: c = 1)
    got = ctx.shift(np.array([[0.3, 0.2, 0.3, 0.2, 0.1, 0.2]], np.float32), [0, 1, 2], [3, 4, 5], conf=0.5)
    assert got["rank"][0] == SR.rank_and_margin(3, 3, SR.zq_of(0.5))[0] == 2 and got["lo"][0] == 0.0 and got["hi"][0] == 0.2
    ps = np.tile(np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], np.float32), (5, 1))
    for g1, g2 in (([0, 1], [2, 3, 4]), ([0], [1]), ([0, 1, 2, 3], [4, 5])):
        for entry in ("host", "dev"):
            got = call(ctx, entry, ps, np.array(g1, np.int32), np.array(g2, np.int32))
            assert not any(RS.bits(got[name]).any() for name in OUTS)
    empty = ctx.shift(np.zeros((0, 7), np.float32), [0, 1, 2], [3, 4, 5])
    assert all(empty[name].shape == (0,) for name in OUTS)


ERROR_CASES = ("n1 0", "n2 0", "n1 4097", "column in both lists", "column twice in one list", "index equal to s",
               "negative index", "more columns than the table", "zq 0", "zq negative", "zq NaN", "zq infinite")
DEV_CASES = ("n1 0", "n2 0", "n1 4097", "more columns than the table", "zq 0", "zq negative", "zq NaN", "zq infinite")


def _error_call(ctx, case, dev):
    """-> (return code, outputs after, outputs before)"""
    import ctypes as C
    n, s = 3, 12
    g1, g2 = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6, 7], np.int32)
    n1, n2, zq = 4, 4, 1.959963984540054
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
    elif case.startswith("zq"):
        zq = {"0": 0.0, "negative": -1.96, "NaN": float("nan"), "infinite": float("inf")}[case[3:]]
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(SR.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    if not dev:
        held = [np.ascontiguousarray(ps), g1, g2]
        ptr = lambda a: a.ctypes.data                          # noqa: E731
        rc = ctx.lib.sdice_shift(ctx.h, n, s, ptr(held[0]), ptr(g1), n1, ptr(g2), n2, C.c_double(zq), *[ptr(outs[x]) for x in OUTS])
        return rc, outs, before
    held = [ctx.to_device(v, v.dtype) for v in (ps, g1, g2)] + [ctx.to_device(outs[x], outs[x].dtype) for x in OUTS]
    try:
        rc = ctx.lib.sdice_shift_dev(ctx.h, n, s, held[0].ptr, held[1].ptr, n1, held[2].ptr, n2, C.c_double(zq),
                                     *[a.ptr for a in held[3:]])
        ctx.sync()
        return rc, {x: a.to_host() for x, a in zip(OUTS, held[3:])}, before
    finally:
        for a in held:
            a.free()


@gpu
@pytest.mark.parametrize("case", ERROR_CASES)
def test_errors_leave_the_outputs_untouched(ctx, case):
    """SDICE_ERR_ARG before any launch, a message, outputs untouched, through the host call; through the _dev call the
    cases it can see (the counts and zq: the lists are device memory there)"""
    rc, outs, before = _error_call(ctx, case, dev=False)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    message = ctx.lib.sdice_last_error()
    assert message and b"sdice_shift" in message
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "n1 4097":
        assert b"4096" in message and b"4097" in message
    if case.startswith("zq"):
        assert b"zq" in message
    if case in DEV_CASES:
        rc, outs, before = _error_call(ctx, case, dev=True)
        assert rc == -1 and ctx.lib.sdice_last_error(), case
        for x in outs:
            assert np.array_equal(outs[x], before[x]), (case, x, "dev")
    # the context still works
    ok = ctx.shift(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5])
    assert ok["tested"].tolist() == [1, 1] and ok["shift"].tolist() == [0.0, 0.0] and ok["rank"].tolist() == [1, 1]


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    """60 rows x (8 v 9) samples + 2 samples outside the manifests; the manifests' order is not the table's.  Shifted rows,
    rows where the medians agree and the shift does not, heavy ties, all-equal rows, rows with a starved set"""
    rng = np.random.default_rng(2040)
    n, s = 60, 19
    samples, _ = RS.ps_names(n, s)
    set1 = np.array([0, 2, 4, 6, 8, 10, 12, 14])
    set2 = np.array([1, 3, 5, 7, 9, 11, 13, 15, 16])
    v = 0.3 + 0.2 * rng.random((n, s))
    v[:, set1] += 0.1 * rng.standard_normal((n, 1))
    v = np.clip(v, 0, 1)
    v[:10] = np.round(v[:10] * 5) / 5                                                    # heavy ties
    text = np.where(rng.random((n, s)) < 0.08, "nan", np.char.mod("%.3f", v))
    text[10:13] = "0.500"                                                                 # all-equal rows stay in the table
    text[13:16][:, set2[1:]] = "nan"                                                      # one value left in set 2: rows dropped
    path, (m1, m2), names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in set1[::-1]], "A"),
                                                             ([samples[j] for j in rng.permutation(set2)], "B")])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, m1, m2, names, matrix, set1.astype(np.int32), set2.astype(np.int32)


def _ns(table_path, m1, m2, out, **extra):
    base = dict(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=False, exact=False,
                strata=None, trend=False, ks=False, shift=True, conf=None, annotation="", outputFile=out)
    base.update(extra)
    return argparse.Namespace(**base)


@gpu
@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("exact", [False, True])
def test_cli_shift_byte_for_byte(ctx, golden_dir, tmp_path, exact, gtf):
    """compare_sample_sets --shift (with and without --exact, with and without -a) on 60 rows of 8 v 9: the file equals,
    byte for byte, the table the referee formats from ITS shift, lo and hi and from the fields, the p and the BH of the
    rank-sum call the command makes without the flag -- and the same command without the flag writes that table less the
    three columns"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, names, matrix, g1, g2 = _write_cli_inputs(tmp_path)
    out, bare = str(tmp_path / "out.tsv"), str(tmp_path / "bare.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(_ns(table_path, m1, m2, out, exact=exact, annotation=anno), ctx=ctx)
    css.run_with(_ns(table_path, m1, m2, bare, exact=exact, annotation=anno, shift=False), ctx=ctx)
    ref = SR.table_reference(matrix, g1, g2, SR.zq_of(0.95))
    plain = (ctx.ranksum_exact if exact else ctx.ranksum)(matrix, g1, g2)
    keep = np.flatnonzero(ref["tested"])
    assert np.array_equal(plain["tested"], ref["tested"])
    assert 50 <= keep.size < 60 and {10, 11, 12} <= set(keep.tolist()) and not {13, 14, 15} & set(keep.tolist())
    assert ref["grid"][keep].all() and (ref["rank"][keep] > 1).any()
    apart = sum(abs(ref["shift"][r] - float(plain["delta"][r])) > 0.01 for r in keep)
    assert apart > 10                                        # what the column is for: the estimate is not delta
    q = ctx.bh(plain["p"][keep])
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else None
    want = SR.format_table(names, keep, plain, ref, q, sfx, gtf)
    got = open(out).read()
    diff = [(g, w) for g, w in zip(got.split("\n"), want.split("\n")) if g != w]
    print(f"exact={exact} gtf={gtf}: lines that differ {len(diff)} of {want.count(chr(10))}")
    for g, w in diff[:5]:
        print("got ", g, "\nwant", w)
    assert got == want
    less = ["\t".join(c for i, c in enumerate(line.split("\t")) if i not in (6, 7, 8)) for line in got.split("\n")]
    assert open(bare).read() == "\n".join(less)
    # another level moves the interval's columns alone
    css.run_with(_ns(table_path, m1, m2, out, exact=exact, annotation=anno, conf=0.5), ctx=ctx)
    half = SR.table_reference(matrix, g1, g2, SR.zq_of(0.5))
    assert open(out).read() == SR.format_table(names, keep, plain, half, q, sfx, gtf)
    assert (half["rank"][keep] > ref["rank"][keep]).any()


@gpu
def test_cli_refusals_with_a_live_context(ctx, tmp_path, capsys):
    """the refusals' text and status with the engine at hand: one line on stderr, status 1, no output file"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, *_ = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "refused.tsv")
    for extra, words in ((dict(paired=True), "compare_sample_sets --shift: cannot be combined with --paired ("),
                         (dict(ks=True), "compare_sample_sets --shift: cannot be combined with --ks ("),
                         (dict(trend=True), "compare_sample_sets --shift: cannot be combined with --trend ("),
                         (dict(moreManifests=[m2]), "compare_sample_sets --shift: cannot be combined with -mx/--moreManifests ("),
                         (dict(strata=m1), "compare_sample_sets --shift: cannot be combined with --strata ("),
                         (dict(shift=False, conf=0.9), "compare_sample_sets --conf: needs --shift ("),
                         (dict(conf=1.5), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 1.5)")):
        with pytest.raises(SystemExit) as e:
            css.run_with(_ns(table_path, m1, m2, out, **extra), ctx=ctx)
        err = capsys.readouterr().err
        assert e.value.code == 1 and err.count("\n") == 1 and err.startswith(words) and err.endswith(". Exit.\n"), err
        assert not os.path.exists(out)


def _cells(path):
    return [line.rstrip("\n").split("\t") for line in open(path)]


@gpu
def test_cli_on_an_empty_table_and_without_the_flag(ctx, golden_dir, tmp_path):
    """a table without rows gives the header alone; the golden two-set run with the flags absent and with shift=False,
    conf=None: every byte of tests/golden/compare/expected_out_device.tsv, what the command wrote for these inputs on an
    MI355X before it had any of its added flags.  expected_out.tsv beside it holds scipy's p-values and statsmodels' BH,
    an ulp or two from the device's on most lines before this flag as after, so its cells are held by the rule of
    tests/test_gpu_cli.py: text and float32 cells as strings, p-value and corrected to 1e-6 relative."""
    from splicedice_amd import compare_sample_sets as css
    samples, _ = RS.ps_names(0, 8)
    table = tmp_path / "empty_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(samples) + "\n")
    m = []
    for i, group in enumerate((samples[:4], samples[4:])):
        m.append(tmp_path / f"e{i}.tsv")
        m[-1].write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    out = str(tmp_path / "empty_out.tsv")
    css.run_with(_ns(str(table), str(m[0]), str(m[1]), out), ctx=ctx)
    assert open(out).read() == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tshift\tshift_lo\tshift_hi\tp-value\tcorrected\n"
    d = os.path.join(golden_dir, "compare")
    outs = []
    for extra in ({}, dict(shift=False, conf=None)):
        outs.append(str(tmp_path / f"cmp{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "in_allPS.tsv"), manifest1=os.path.join(d, "m1.tsv"),
                                        manifest2=os.path.join(d, "m2.tsv"), annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    recorded = open(os.path.join(d, "expected_out_device.tsv"), "rb").read()
    assert open(outs[0], "rb").read() == recorded and open(outs[1], "rb").read() == recorded
    got, want = _cells(outs[1]), _cells(os.path.join(d, "expected_out.tsv"))
    assert len(got) == len(want) and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert g[:6] == w[:6]
        np.testing.assert_allclose([float(x) for x in g[6:]], [float(x) for x in w[6:]], rtol=1e-6)
