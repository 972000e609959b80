"""sdice_walsh (the paired shift -- the median of the Walsh averages -- with its confidence interval) and compare_sample_sets
--paired --pseudomedian against the referee (tests/walsh_referee.py: brute force over all Walsh sums, integers on the
3-decimal grid, float32 differences and float64 sums off it, the rank from mpmath at 40 digits) and the signed-rank call.

Bars, without a tolerance anywhere: shift, lo and hi equal the referee's as float64 BITS, NaN where the referee has NaN;
rank equal as an integer; tested equal to the referee's and to ctx.signedrank's on the same pairs; every slot of a row that
is not tested all-zero bits, also where the output held something else before the call.

The tables (tests/walsh_fixtures.py) hold every row kind on 3-decimal values, off the grid and mixed, at every pair count that
changes the kernel or its lane-group width; tests/test_walsh_cpu.py checks on the CPU that they are what they claim and that
no rank of theirs hangs on a rounding."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import walsh_fixtures as WF  # noqa: E402
import walsh_referee as WR  # noqa: E402
from walsh_referee import OUTS  # noqa: E402

gpu = pytest.mark.gpu
PAIR_LIMIT = 4096                   # pairs a call takes (include/sdice.h)
F64 = ("shift", "lo", "hi")


def check(got, ref, label, plain=None):
    """asserts every bar -> dict(tested, nan, grid): the numbers of tested rows, of NaN triples and of tested grid rows"""
    assert got["tested"].dtype == np.uint8 and got["rank"].dtype == np.int32, label
    bad = np.flatnonzero(got["tested"] != ref["tested"])
    assert bad.size == 0, (label, "tested", bad[:5].tolist())
    if plain is not None:
        assert np.array_equal(got["tested"], plain["tested"]), (label, "tested unlike the signed-rank call's")
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


def dev_call(ctx, d_ps, a, b, n, conf=0.95):
    """the resident entry point on a resident table (or a view of it), every output holding 0xA5 bytes before the call ->
    host copies of the outputs"""
    from splicedice_amd.engine import WALSH_FIELDS, field_shapes
    held = [ctx.to_device(v, np.int32) for v in (a, b)]
    out = {name: ctx.empty(*sd).memset(0xA5) for name, sd in field_shapes(WALSH_FIELDS, n).items()}
    try:
        ctx.walsh_resident(d_ps, *held, out, conf)
        ctx.sync()
        return {name: d.to_host() for name, d in out.items()}
    finally:
        for d in (*held, *out.values()):
            d.free()


def dev_table(ctx, ps, a, b, conf=0.95):
    d_ps = ctx.to_device(ps, np.float32)
    try:
        return dev_call(ctx, d_ps, a, b, ps.shape[0], conf)
    finally:
        d_ps.free()


def call(ctx, entry, ps, a, b, conf=0.95):
    return ctx.walsh(ps, a, b, conf) if entry == "host" else dev_table(ctx, ps, a, b, conf)


# ---------------------------------------------------------------- the library
@gpu
@pytest.mark.parametrize("flavour", WF.FLAVOURS)
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_walsh_parity(ctx, entry, flavour):
    """every row kind at every pair count 3..66, 127..129, 255..257: both kernels, every lane-group width, 64 | 65; tables
    on the grid (the integer paths), off it and mixed (grid and off-grid rows side by side in a wave)"""
    total = dict(tested=0, nan=0, grid=0)
    for m in WF.PAIRS:
        ps, a, b, _ = WF.table(m, flavour)
        out = check(call(ctx, entry, ps, a, b), WF.reference(m, flavour), f"pairs={m} {flavour} {entry}",
                    plain=ctx.signedrank(ps, a, b))
        for k in total:
            total[k] += out[k]
    print(f"{entry} {flavour}: {len(WF.PAIRS)} tables, {total}")
    assert total["tested"] > 8 * len(WF.PAIRS)
    assert (total["grid"] == total["tested"] and total["nan"] == 0) if flavour == "grid" else (total["nan"] >= 2 * len(WF.PAIRS) - 4)
    assert flavour != "off" or total["grid"] == 0


@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_levels(ctx, entry):
    """conf 0.5, 0.8, 0.9, 0.95 and 0.99 in both kernels: the rank moves, the shift does not"""
    for m in WF.LEVEL_PAIRS:
        ps, a, b, _ = WF.table(m)
        ranks, shifts = [], []
        for conf in WF.LEVELS:
            ref = WF.reference(m, "mixed", 1, None, conf)
            check(call(ctx, entry, ps, a, b, conf), ref, f"pairs={m} conf={conf} {entry}")
            ranks.append(ref["rank"][ref["tested"] == 1].astype(np.int64))
            shifts.append(ref["shift"])
        assert all((x >= y).all() for x, y in zip(ranks, ranks[1:])) and (m < 7 or (ranks[0] > ranks[-1]).any())
        assert all(np.array_equal(RS.bits(s), RS.bits(shifts[0])) for s in shifts)
    with pytest.raises(ValueError):
        ctx.walsh(ps, a, b, conf=1.0)


@gpu
@pytest.mark.parametrize("m", WF.SLICE_PAIRS)
def test_row_slices(ctx, m):
    """views ps[a:b] of a resident table at odd a and b, and the host call on the same slices"""
    ps, a, b, _ = WF.table(m, "mixed", 4)
    rows, width = ps.shape
    want = ctx.walsh(ps, a, b)
    check(want, WF.reference(m, "mixed", 4), f"pairs={m} 4 per kind")
    d_ps = ctx.to_device(ps, np.float32)
    try:
        for lo, hi in ((1, rows), (3, 70), (65, rows - 1), (rows - 1, rows)):
            cut = dev_call(ctx, d_ps.offset(lo * width, (hi - lo, width)), a, b, hi - lo)
            host = ctx.walsh(ps[lo:hi], a, b)
            for name in OUTS:
                RS.assert_same_bits(cut[name], want[name][lo:hi], (m, lo, hi, name, "resident"))
                RS.assert_same_bits(host[name], want[name][lo:hi], (m, lo, hi, name, "host"))
    finally:
        d_ps.free()


@gpu
def test_the_most_pairs(ctx):
    """4096 pairs, two rows only (the referee orders 8.4 M sums a row): one on the grid, one off it, 6 % NaN each, through
    both entry points"""
    ps, a, b, what = WF.table(WF.LARGE, "mixed", 1, WF.LARGE_KINDS)
    assert [g for _, g in what] == [True, False]
    ref = WF.reference(WF.LARGE, "mixed", 1, WF.LARGE_KINDS)
    assert (ref["m"] > 3000).all() and (ref["m"] < WF.LARGE).all()
    assert all(WR.rank_and_margin(int(m), WR.zq_of(0.95))[1] >= 1e-6 for m in ref["m"])
    for entry in ("host", "dev"):
        out = check(call(ctx, entry, ps, a, b), ref, f"{WF.LARGE} pairs {entry}", plain=ctx.signedrank(ps, a, b))
        assert out == dict(tested=2, nan=0, grid=1)
    assert ref["rank"].min() > 1000000 and (ref["lo"] < ref["shift"]).all() and (ref["shift"] < ref["hi"]).all()


@gpu
def test_swapping_the_sides_negates_and_swaps(ctx):
    for m in (3, 4, 7, 16, 40, 64, 65, 129):
        ps, a, b, _ = WF.table(m)
        got, swapped = ctx.walsh(ps, a, b), ctx.walsh(ps, b, a)
        nan = np.isnan(got["shift"])
        assert np.array_equal(swapped["tested"], got["tested"]) and np.array_equal(swapped["rank"], got["rank"])
        for x, y in (("shift", "shift"), ("lo", "hi"), ("hi", "lo")):
            assert np.array_equal(np.isnan(swapped[x]), nan)
            RS.assert_same_bits(swapped[x][~nan], (-got[y] + 0.0)[~nan], (m, x, "is not minus", y))


@gpu
def test_the_hand_cases_and_tiny_calls(ctx):
    """the hand cases of tests/test_walsh_cpu.py; one or two pairs give zeros; n = 0 is a no-op"""
    row = np.array([[0.3, 0.5, 0.9, 0.2, 0.1, 0.4, 9]], np.float32)
    got = ctx.walsh(row, [0, 1, 2], [3, 4, 5])
    assert [got[k][0] for k in OUTS] == [1, 0.35, 0.1, 0.5, 1]
    row = np.array([[0.1, 0.2, 0.4, 0.5, 0.2, 0.2, 0.2, 0.2]], np.float32)          # d = -100 0 200 300: the zero is kept
    got = ctx.walsh(row, [0, 1, 2, 3], [4, 5, 6, 7])
    assert [got[k][0] for k in OUTS] == [1, 0.1, -0.1, 0.3, 1]
    got = ctx.walsh(row, [0, 1, 2, 3], [4, 5, 6, 7], conf=0.5)
    assert [got[k][0] for k in OUTS] == [1, 0.1, 0.0, 0.2, 3]
    got = ctx.walsh(np.array([[0.3, 0.2, 0.3, 0.2, 0.1, 0.2]], np.float32), [0, 1, 2], [3, 4, 5])
    assert [got[k][0] for k in OUTS] == [1, 0.1, 0.1, 0.1, 1]            # (equal printed differences tie)
    got = ctx.walsh(np.full((1, 8), 0.5, np.float32), [0, 1, 2, 3], [4, 5, 6, 7])
    assert got["tested"][0] == 1 and not any(RS.bits(got[k]).any() for k in F64)      # all differences zero: +0.0 thrice
    ps = np.tile(np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], np.float32), (5, 1))
    for a, b in (([0, 1], [2, 3]), ([0], [1])):
        for entry in ("host", "dev"):
            got = call(ctx, entry, ps, np.array(a, np.int32), np.array(b, np.int32))
            assert not any(RS.bits(got[name]).any() for name in OUTS)
    empty = ctx.walsh(np.zeros((0, 7), np.float32), [0, 1, 2], [3, 4, 5])
    assert all(empty[name].shape == (0,) for name in OUTS)
    with pytest.raises(ValueError):
        ctx.walsh(ps, [0, 1, 2], [3, 4])


ERROR_CASES = ("m 0", "m 4097", "column in both lists", "column twice in one list", "index equal to s", "negative index",
               "more columns than the table", "zq 0", "zq negative", "zq NaN", "zq infinite")
DEV_CASES = ("m 0", "m 4097", "more columns than the table", "zq 0", "zq negative", "zq NaN", "zq infinite")


def _error_call(ctx, case, dev):
    """-> (return code, outputs after, outputs before)"""
    import ctypes as C
    n, s = 3, 12
    a, b = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6, 7], np.int32)
    m, zq = 4, 1.959963984540054
    if case == "m 0":
        m = 0
    elif case == "m 4097":
        m, s = PAIR_LIMIT + 1, 2 * (PAIR_LIMIT + 1) + 8
        a, b = np.arange(8, 8 + m, dtype=np.int32), np.arange(8 + m, 8 + 2 * m, dtype=np.int32)
    elif case == "column in both lists":
        b[2] = a[0]
    elif case == "column twice in one list":
        a[3] = a[1]
    elif case == "index equal to s":
        b[3] = s
    elif case == "negative index":
        a[0] = -1
    elif case == "more columns than the table":
        s = 7
    elif case.startswith("zq"):
        zq = {"0": 0.0, "negative": -1.96, "NaN": float("nan"), "infinite": float("inf")}[case[3:]]
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(WR.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    if not dev:
        ptr = lambda v: v.ctypes.data                          # noqa: E731
        rc = ctx.lib.sdice_walsh(ctx.h, n, s, ptr(ps), ptr(a), ptr(b), m, C.c_double(zq), *[ptr(outs[x]) for x in OUTS])
        return rc, outs, before
    held = [ctx.to_device(v, v.dtype) for v in (ps, a, b)] + [ctx.to_device(outs[x], outs[x].dtype) for x in OUTS]
    try:
        rc = ctx.lib.sdice_walsh_dev(ctx.h, n, s, held[0].ptr, held[1].ptr, held[2].ptr, m, C.c_double(zq),
                                     *[d.ptr for d in held[3:]])
        ctx.sync()
        return rc, {x: d.to_host() for x, d in zip(OUTS, held[3:])}, before
    finally:
        for d in held:
            d.free()


@gpu
@pytest.mark.parametrize("case", ERROR_CASES)
def test_errors_leave_the_outputs_untouched(ctx, case):
    """SDICE_ERR_ARG before any launch, a message, outputs untouched, through the host call; through the resident call the
    cases it can see (the count and zq: the lists are device memory there)"""
    rc, outs, before = _error_call(ctx, case, dev=False)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    message = ctx.lib.sdice_last_error()
    assert message and b"sdice_walsh" in message
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "m 4097":
        assert b"4096" in message and b"4097" in message
    if case.startswith("zq"):
        assert b"zq" in message
    if case in DEV_CASES:
        rc, outs, before = _error_call(ctx, case, dev=True)
        assert rc == -1 and ctx.lib.sdice_last_error(), case
        for x in outs:
            assert np.array_equal(outs[x], before[x]), (case, x, "dev")
    # the context still works: d = -200 100 100, the sums -400 -100 -100 200 200 200, the median (-100 + 200) / 4000
    ok = ctx.walsh(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5])
    assert ok["tested"].tolist() == [1, 1] and ok["shift"].tolist() == [0.025, 0.025] and ok["rank"].tolist() == [1, 1]
    assert ok["lo"].tolist() == [-0.2, -0.2] and ok["hi"].tolist() == [0.1, 0.1]


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    """60 rows x 9 pairs + 2 samples outside the manifests; the manifests' order is not the table's.  Rows whose pairs move
    together, rows where the medians agree and the pairs' change does not, heavy ties with equal pairs, all-equal rows, rows
    with two kept pairs"""
    rng = np.random.default_rng(2140)
    n, s, m = 60, 20, 9
    samples, _ = RS.ps_names(n, s)
    v = rng.random((n, s))
    v[:, :m] = np.clip(v[:, m:2 * m] + 0.06 * rng.standard_normal((n, m)) + 0.1 * rng.standard_normal((n, 1)), 0, 1)
    v[:10] = np.round(v[:10] * 5) / 5                                                    # heavy ties, equal pairs
    text = np.where(rng.random((n, s)) < 0.05, "nan", np.char.mod("%.3f", v))
    text[10:13] = "0.500"                                                                 # all-equal rows stay in the table
    text[13:16, 0:7] = "nan"                                                              # two kept pairs: rows dropped
    order = [3, 0, 8, 5, 1, 7, 4, 2, 6]
    path, (m1, m2), names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in order], "A"),
                                                             ([samples[j + m] for j in order], "B")])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, m1, m2, names, matrix, np.array(order, np.int32), np.array(order, np.int32) + m


def _ns(table_path, m1, m2, out, **extra):
    base = dict(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=True, exact=False,
                strata=None, trend=False, ks=False, shift=False, conf=None, pseudomedian=True, annotation="", outputFile=out)
    base.update(extra)
    return argparse.Namespace(**base)


@gpu
@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("exact", [False, True])
def test_cli_pseudomedian_byte_for_byte(ctx, golden_dir, tmp_path, exact, gtf):
    """compare_sample_sets --paired --pseudomedian (with and without --exact, with and without -a) on 60 rows of 9 pairs: the
    file equals, byte for byte, the table the referee formats from ITS shift, lo and hi and from the fields, the p and the
    BH of the signed-rank call the command makes without the flag -- and the same command without the flag writes that
    table less the three columns"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, names, matrix, a, b = _write_cli_inputs(tmp_path)
    out, bare = str(tmp_path / "out.tsv"), str(tmp_path / "bare.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(_ns(table_path, m1, m2, out, exact=exact, annotation=anno), ctx=ctx)
    css.run_with(_ns(table_path, m1, m2, bare, exact=exact, annotation=anno, pseudomedian=False), ctx=ctx)
    ref = WR.table_reference(matrix, a, b, WR.zq_of(0.95))
    plain = (ctx.signedrank_exact if exact else ctx.signedrank)(matrix, a, b)
    keep = np.flatnonzero(ref["tested"])
    assert np.array_equal(plain["tested"], ref["tested"])
    assert 50 <= keep.size < 60 and {10, 11, 12} <= set(keep.tolist()) and not {13, 14, 15} & set(keep.tolist())
    assert ref["grid"][keep].all() and (ref["rank"][keep] > 1).any() and (ref["rank"][keep] == 1).any()
    apart = sum(abs(ref["shift"][r] - float(plain["delta"][r])) > 0.01 for r in keep)
    assert apart > 10                                        # what the column is for: the estimate is not delta
    q = ctx.bh(plain["p"][keep])
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else None
    want = WR.format_table(names, keep, plain, ref, q, sfx, gtf)
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
    half = WR.table_reference(matrix, a, b, WR.zq_of(0.5))
    assert open(out).read() == WR.format_table(names, keep, plain, half, q, sfx, gtf)
    assert (half["rank"][keep] > ref["rank"][keep]).any()


@gpu
def test_cli_refusals_and_an_empty_table_with_a_live_context(ctx, tmp_path, capsys):
    """the refusals' text and status with the engine at hand: one line on stderr, status 1, no output file; a table without
    rows gives the header alone"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, *_ = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "refused.tsv")
    for extra, words in ((dict(paired=False), "compare_sample_sets --pseudomedian: needs --paired ("),
                         (dict(shift=True), "compare_sample_sets --shift: cannot be combined with --paired ("),
                         (dict(ks=True), "compare_sample_sets --ks: cannot be combined with --paired ("),
                         (dict(moreManifests=[m2]), "compare_sample_sets --paired: cannot be combined with -mx/--moreManifests ("),
                         (dict(pseudomedian=False, conf=0.9), "compare_sample_sets --conf: needs --shift ("),
                         (dict(conf=1.5), "compare_sample_sets --conf: LEVEL must satisfy 0 < LEVEL < 1 (got 1.5)")):
        with pytest.raises(SystemExit) as e:
            css.run_with(_ns(table_path, m1, m2, out, **extra), ctx=ctx)
        err = capsys.readouterr().err
        assert e.value.code == 1 and err.count("\n") == 1 and err.startswith(words) and err.endswith(". Exit.\n"), err
        assert not os.path.exists(out)
    samples, _ = RS.ps_names(0, 8)
    table = tmp_path / "empty_allPS.tsv"
    table.write_text("cluster\t" + "\t".join(samples) + "\n")
    m = []
    for i, group in enumerate((samples[:4], samples[4:])):
        m.append(tmp_path / f"e{i}.tsv")
        m[-1].write_text("".join(f"{x}\tpath\tmeta\tA\n" for x in group))
    css.run_with(_ns(str(table), str(m[0]), str(m[1]), out), ctx=ctx)
    assert open(out).read() == "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tshift\tshift_lo\tshift_hi\tp-value\tcorrected\n"
