"""GPU: sdice_friedman and sdice_page (Friedman's test and Page's L test over k matched sets) and compare_sample_sets
--repeated against the exact referee (tests/friedman_referee.py) and numpy.

Bars: tested, blocks, medians, means, delta, Q, W and L equal as bits (Q and W: the correctly rounded
rational); z within 2 ulp of the correctly rounded A / sqrt(B) and bit-equal to -z of the call on the reversed sets; p
within 1e-9 relative of the referee's 50-digit value where that is >= 1e-280, below 2e-280 under it, 0 past the float64
range.  Every test prints the worst figures it saw per band before it ends."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friedman_fixtures as FF  # noqa: E402
import friedman_referee as FR  # noqa: E402
import rank_support as RS  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

pytestmark = pytest.mark.gpu

TESTS = ("friedman", "page")


def _host(ctx, test, ps, sets):
    return getattr(ctx, test)(ps, list(sets))


@pytest.mark.parametrize("k", FF.KS)
def test_shapes_and_row_kinds(ctx, k):
    """every m of the issue for k sets (the limits 64 x 256 and 4 x 4096 and both sides of the planner's boundary among
    them), a row of every kind per table, the flavours (grid, off it, mixed) taking turns; both tests, both entry points"""
    rng = np.random.default_rng(2100 + k)
    worst = {t: FF.Worst() for t in TESTS}
    forms = set()
    for turn, m in enumerate(FF.shapes(k)):
        sets, s = FF.draw_sets(rng, k, m)
        ps, kinds = FF.table(rng, sets, s, turn)
        ref = FR.table_reference(ps, sets)
        forms.add(FF.staged(k, m) <= FF.WAVE_MAX)
        if m >= 3:
            r = FF.SAME_ORDER
            assert ref["tested"][r] and ref["w"][r] == 1.0 and ref["q"][r] == m * (k - 1), (k, m)
            assert ref["tested"][:3].tolist() == [1, 0, 1] and ref["blocks"][2] == 3
        else:
            assert not ref["tested"].any()
        for test in TESTS:
            got = _host(ctx, test, ps, sets)
            FF.check(test, got, ref, f"{test} k={k} m={m}", worst[test])
            dev = FF.resident(ctx, test, ps, sets)
            for name in FF.TEST_OUTS[test]:
                RS.assert_same_bits(dev[name], got[name], (test, k, m, name, "resident v host"))
    assert forms == {True, False}            # the wave form and the workgroup form
    for test in TESTS:
        print(worst[test].line(f"{test} k={k}"))


@pytest.mark.parametrize("test", TESTS)
def test_optional_outputs_absent_and_prefilled(ctx, test):
    """q, w / l and blocks are optional: absent (NULL) in any combination, the other fields are what they are with all of
    them present, on both entry points; the outputs are pre-filled (0xA5 on the device, 7 on the host) and every slot is
    written"""
    rng = np.random.default_rng(31)
    from splicedice_amd import engine
    optional = engine.ROW_TESTS[test][1]
    for k, m in ((3, 5), (5, 300)):
        sets, s = FF.draw_sets(rng, k, m)
        ps, _ = FF.table(rng, sets, s)
        full = _host(ctx, test, ps, sets)
        for fill in (0x00, 0xA5, 0xFF):
            dev = FF.resident(ctx, test, ps, sets, fill=fill)
            for name in FF.TEST_OUTS[test]:
                RS.assert_same_bits(dev[name], full[name], (test, k, m, name, fill))
        for at in range(1, 1 << len(optional)):
            skip = [f for i, f in enumerate(optional) if at >> i & 1]
            dev = FF.resident(ctx, test, ps, sets, skip=skip)
            assert set(dev) == set(FF.TEST_OUTS[test]) - set(skip)
            outs = {name: np.full(v.shape, 7, v.dtype) for name, v in full.items()}
            rc = RS.raw_call(ctx, "sdice_" + test, ps, (engine.friedman_columns(sets, s), k, m),
                             {name: None if name in skip else a for name, a in outs.items()}, FF.TEST_OUTS[test])
            assert rc == 0
            for name in set(FF.TEST_OUTS[test]) - set(skip):
                RS.assert_same_bits(dev[name], full[name], (test, k, m, name, skip))
                RS.assert_same_bits(outs[name], full[name], (test, k, m, name, skip, "host"))
            for name in skip:
                assert np.all(outs[name] == 7)


def test_row_slices(ctx):
    """a call on rows r0..r1 of a resident table gives those rows of the call on the whole table"""
    rng = np.random.default_rng(32)
    for k, m in ((4, 8), (3, 700)):
        sets, s = FF.draw_sets(rng, k, m)
        ps = np.concatenate([FF.table(rng, sets, s, t)[0] for t in range(6)])
        n = ps.shape[0]
        d_ps = ctx.to_device(ps, np.float32)
        try:
            for test in TESTS:
                whole = FF.resident(ctx, test, None, sets, d_ps=d_ps)
                for r0, r1 in ((0, 1), (5, 41), (n - 13, n)):
                    part = FF.resident(ctx, test, None, sets, d_ps=d_ps.offset(r0 * s, (r1 - r0, s)))
                    for name in FF.TEST_OUTS[test]:
                        RS.assert_same_bits(part[name], whole[name][..., r0:r1], (test, k, m, name, r0, r1))
        finally:
            d_ps.free()


@pytest.mark.parametrize("form,n", [("wave", 1_000_000), ("workgroup", 100_000)])
def test_more_rows_than_one_grid_pass(ctx, form, n):
    """3 x 3 over more rows than the kernel's grid holds at once (the workgroup form by friedman.wave_max = 0): the rows are
    a palette of 480 rows of every kind, the reference is the palette's, scattered"""
    rng = np.random.default_rng(33)
    sets, s = FF.draw_sets(rng, 3, 3)
    palette = np.concatenate([FF.table(rng, sets, s, t)[0] for t in range(40)])
    idx = RS.palette_index(n, palette.shape[0])
    ps = np.ascontiguousarray(palette[idx])
    ref = RS.scatter(FR.table_reference(palette, sets), idx)
    assert 0.3 * n < ref["tested"].sum() < n
    with ctx.params({"friedman.wave_max": FF.WAVE_MAX if form == "wave" else 0}):
        for test in TESTS:
            worst = FF.Worst()
            FF.check(test, FF.resident(ctx, test, ps, sets), ref, f"{test} {form} n={n}", worst)
            print(worst.line(f"{test} {form} 3 x 3 x {n}"))


def test_every_knob_value(ctx):
    """friedman.wave_max moves the boundary between the two forms: every value gives the default's results bit for bit, on
    shapes on both sides of every value (at 32768 a wave takes 4 x 4096 and 64 x 256 alone in its workgroup)"""
    rng = np.random.default_rng(34)
    worst = {t: FF.Worst() for t in TESTS}
    assert ctx.get_param("friedman.wave_max") == FF.WAVE_MAX
    for k, m in ((3, 3), (4, 8), (8, 8), (3, 16), (2, 31), (4, 256), (4, 257), (63, 17), (64, 256), (4, 4096), (2, 4096)):
        sets, s = FF.draw_sets(rng, k, m)
        ps, _ = FF.table(rng, sets, s, k)
        ref = FR.table_reference(ps, sets)
        for test in TESTS:
            base = _host(ctx, test, ps, sets)
            FF.check(test, base, ref, f"{test} {k} x {m}", worst[test])
            for value in FF.KNOB_VALUES:
                with ctx.params({"friedman.wave_max": value}):
                    got = _host(ctx, test, ps, sets)
                for name in FF.TEST_OUTS[test]:
                    RS.assert_same_bits(got[name], base[name], (test, k, m, value, name))
    assert ctx.get_param("friedman.wave_max") == FF.WAVE_MAX
    for test in TESTS:
        print(worst[test].line(test))


def test_permuted_sets_and_subjects(ctx):
    """permuting the sets permutes med / mean and leaves tested, blocks, delta, Q, W, both p and |z| bit for bit -- reversing
    them negates z and nothing else; permuting the subjects leaves all of these and the medians bit for bit (a mean may
    move in its last bit: another order of the same sum)"""
    rng = np.random.default_rng(35)
    for k, m in ((3, 7), (5, 40), (8, 129), (4, 1500)):
        sets, s = FF.draw_sets(rng, k, m)
        ps = np.concatenate([FF.table(rng, sets, s, t)[0] for t in range(3)])
        fr, pg = _host(ctx, "friedman", ps, sets), _host(ctx, "page", ps, sets)
        order = rng.permutation(k)
        fr2, pg2 = _host(ctx, "friedman", ps, sets[order]), _host(ctx, "page", ps, sets[order])
        for name in ("tested", "blocks", "delta", "q", "w", "p"):
            RS.assert_same_bits(fr2[name], fr[name], ("sets permuted", k, m, name))
        for name in ("med", "mean"):
            RS.assert_same_bits(fr2[name], fr[name][order], ("sets permuted", k, m, name))
            RS.assert_same_bits(pg2[name], pg[name][order], ("sets permuted, page", k, m, name))
        rev = _host(ctx, "page", ps, sets[::-1])
        t = pg["tested"].astype(bool)
        assert np.any(pg["z"][t] != 0)
        RS.assert_same_bits(rev["z"], np.where(pg["z"] == 0, 0.0, -pg["z"]), ("sets reversed", k, m, "z"))
        RS.assert_same_bits(rev["l"][t], (pg["blocks"] * (k * (k + 1.0) ** 2 / 2) - pg["l"])[t], ("sets reversed", k, m, "l"))
        for name in ("tested", "blocks", "delta", "p"):
            RS.assert_same_bits(rev[name], pg[name], ("sets reversed", k, m, name))
        subjects = rng.permutation(m)
        fr3, pg3 = _host(ctx, "friedman", ps, sets[:, subjects]), _host(ctx, "page", ps, sets[:, subjects])
        for name in ("tested", "blocks", "delta", "q", "w", "p", "med"):
            RS.assert_same_bits(fr3[name], fr[name], ("subjects permuted", k, m, name))
        for name in ("tested", "blocks", "delta", "z", "l", "p", "med"):
            RS.assert_same_bits(pg3[name], pg[name], ("subjects permuted", k, m, name))


@pytest.mark.parametrize("k,m", [(4, 4096), (64, 256)])
def test_p_ladder(ctx, k, m):
    """p from 1 down to 0: a growing share of the blocks orders the sets the same way, the others at random"""
    rng = np.random.default_rng(36 + k)
    sets, s = FF.draw_sets(rng, k, m, spare=0)
    shares = np.concatenate([[0.0], np.geomspace(0.002, 0.05, 12), np.geomspace(0.05, 1.0, 150)])
    ps = np.empty((shares.size, s), np.float32)
    for r, share in enumerate(shares):
        X = rng.random((k, m)).astype(np.float32)
        same = rng.random(m) < share
        X[:, same] = np.sort(X[:, same], axis=0)
        ps[r, sets.reshape(-1)] = X.reshape(-1)
    ref = FR.table_reference(ps, sets)
    for test in TESTS:
        worst = FF.Worst()
        FF.check(test, _host(ctx, test, ps, sets), ref, f"{test} ladder {k} x {m}", worst)
        p = ref["p_" + test]
        assert p.max() > 0.05 and np.sum((p > 1e-280) & (p < 1e-6)) >= 3 and np.sum((p < 1e-280) & (p > 0)) >= 1 and p.min() == 0.0, p
        print(worst.line(f"{test} ladder {k} x {m}"))


ERRORS = ("k=1", "k=65", "m=0", "m=4097", "km=16385", "km>s", "repeated column", "index out of range", "index negative",
          "NULL tested", "NULL p", "NULL med", "NULL mean", "NULL delta", "NULL z")


@pytest.mark.parametrize("test,case", [(t, c) for t in TESTS for c in ERRORS if (t, c) != ("friedman", "NULL z")])  # (q is optional)
def test_errors_leave_the_outputs_untouched(ctx, test, case):
    n, k, m, s = 3, 3, 4, 20
    cols = None
    if case == "k=1":
        k = 1
    elif case == "k=65":
        k, m, s = 65, 3, 200
    elif case == "m=0":
        m = 0
    elif case == "m=4097":
        k, m, s = 2, 4097, 8200
    elif case == "km=16385":
        k, m, s = 5, 3277, 16390
    elif case == "km>s":
        s = 11
    cols = np.arange(max(k * m, 1), dtype=np.int32)
    if case == "repeated column":
        cols[7] = cols[2]
    elif case == "index out of range":
        cols[5] = s
    elif case == "index negative":
        cols[0] = -1
    ps = np.full((n, s), 0.5, np.float32)
    kk = max(k, 2)
    order = FF.TEST_OUTS[test]
    outs = {name: np.full((kk, n) if name in ("med", "mean") else n, 5, dt)
            for name, dt in (("tested", np.uint8), ("p", np.float64), (order[2], np.float64), (order[3], np.float64),
                             ("blocks", np.int32), ("med", np.float32), ("mean", np.float32), ("delta", np.float32))}
    before = {x: v.copy() for x, v in outs.items()}
    handed = dict(outs)
    if case.startswith("NULL"):
        handed[case.split()[1]] = None
    rc = RS.raw_call(ctx, "sdice_" + test, ps, (cols, k, m), handed, order)
    assert rc == -1, case
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "km=16385":
        assert b"16384" in ctx.lib.sdice_last_error()
    # the resident call checks the counts and the required outputs (the lists are on the device)
    if case in ("k=1", "k=65", "m=0", "m=4097", "km=16385", "km>s") or case.startswith("NULL"):
        d_ps, d_cols = ctx.to_device(ps), ctx.to_device(cols)
        d_out = {name: ctx.to_device(v) for name, v in outs.items()}
        try:
            rc = getattr(ctx.lib, f"sdice_{test}_dev")(ctx.h, n, s, d_ps.ptr, d_cols.ptr, k, m,
                                                       *[None if handed[x] is None else d_out[x].ptr for x in order])
            assert rc == -1, case
            ctx.sync()
            for x in outs:
                assert np.array_equal(d_out[x].to_host(), before[x]), (case, x, "resident")
        finally:
            for a in (d_ps, d_cols, *d_out.values()):
                a.free()
    # the context still works
    ok = getattr(ctx, test)(np.tile(np.float32([0.1, 0.2, 0.3, 0.2, 0.3, 0.4, 0.3, 0.4, 0.6]), (2, 1)), [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    assert ok["tested"].tolist() == [1, 1] and ok["blocks"].tolist() == [3, 3]


def test_engine_refuses_bad_sets_before_any_launch(ctx):
    ps = np.zeros((2, 9), np.float32)
    with pytest.raises(ValueError, match="differ in length"):
        ctx.friedman(ps, [[0, 1, 2], [3, 4, 5], [6, 7]])
    with pytest.raises(ValueError, match="more than once"):
        ctx.page(ps, [[0, 1, 2], [3, 4, 5], [6, 7, 0]])
    with pytest.raises(ValueError, match="outside"):
        ctx.friedman(ps, [[0, 1, 2], [3, 4, 5], [6, 7, 9]])


# ---------------------------------------------------------------- command line
def _write_cli_inputs(tmp_path):
    rng = np.random.default_rng(4343)
    n, k, m = 200, 4, 6
    s = k * m + 2
    samples, _ = RS.ps_names(n, s)
    sets = rng.permutation(s)[: k * m].reshape(k, m)
    v = rng.integers(0, 1001, size=(n, s)) / 1000.0
    v[:, sets[3]] = np.clip(v[:, sets[0]] * 0.6 + 0.3, 0, 1)              # the last set follows the first
    v[:30] = np.round(v[:30] * 2) / 2                                     # heavy ties
    text = np.where(rng.random((n, s)) < 0.04, "nan", np.char.mod("%.3f", v))
    text[40:50] = "0.500"                                                 # fully tied rows stay in the table
    text[60:70, sets[1, :4]] = "nan"                                      # two complete subjects: rows dropped
    table, manifests, names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in g], "A") for g in sets])
    return table, manifests, sets, names


@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("trend", [False, True])
def test_cli_repeated(ctx, golden_dir, tmp_path, trend, gtf):
    """compare_sample_sets --repeated [--trend] on a synthesised 200 x 26 table and four manifests in an order that is not the
    table's: the file against the referee's table -- event, means, medians, delta, Q and W (and the GTF columns) byte for
    byte; z, p-value and corrected are float64 whose last bits are held to bars, not to equality (z 2 ulp, p and BH 1e-9
    relative), so those cells are parsed, held to their bars and must be repr round-trips"""
    from splicedice_amd import compare_sample_sets as css
    table, manifests, sets, names = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1], moreManifests=manifests[2:],
                                    repeated=True, trend=trend, annotation=anno, outputFile=out), ctx=ctx)
    _, _, matrix = css.read_ps_table(table)
    ref = FR.table_reference(matrix, sets)
    p = ref["p_page" if trend else "p_friedman"]
    keep, want = FR.command_table(ref, names, trend, O.bh_fdr(p[ref["tested"].astype(bool)]))
    assert 150 < keep.size < 200 and set(range(40, 50)) <= set(keep.tolist()) and not set(range(60, 70)) & set(keep.tolist())
    lines = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert lines[0] == FR.command_header(4, trend, gtf) and len(lines) == keep.size + 1
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else None
    exact = 10 if trend else 12            # event, 4 means, 4 medians, delta (, Q, W)
    for i, (got, cells) in enumerate(zip(lines[1:], want)):
        assert got[:exact] == cells[:exact], (keep[i], got, cells)
        for at in range(exact, len(cells)):
            field, val = got[at], float(cells[at])
            assert str(np.float64(float(field))) == field
            if trend and at == exact:                                  # (z)
                assert abs(float(field) - val) <= 2 * np.spacing(abs(val)), (keep[i], field, val)
            else:
                assert abs(float(field) - val) <= RS.P_RTOL * abs(val), (keep[i], field, val)
        assert ("\t" + "\t".join(got[len(cells):]) == sfx[i]) if gtf else len(got) == len(cells)


def test_cli_without_the_flag_is_the_mx_command(ctx, tmp_path):
    """without --repeated every byte is as before: a Namespace without the attribute and one with repeated=False give the
    Kruskal-Wallis table"""
    from splicedice_amd import compare_sample_sets as css
    table, manifests, sets, names = _write_cli_inputs(tmp_path)
    outs = []
    for extra in ({}, dict(repeated=False)):
        outs.append(str(tmp_path / f"out{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1],
                                        moreManifests=manifests[2:], annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    a, b = (open(x, "rb").read() for x in outs)
    assert a == b and a.split(b"\n")[0].split(b"\t")[9:] == [b"delta", b"H", b"p-value", b"corrected"]
