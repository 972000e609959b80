"""GPU: sdice_kruskal_dunn (Kruskal-Wallis with Dunn's test for every pair of sets) and compare_sample_sets -mx --posthoc
against the exact referee (tests/dunn_referee.py: the pair numerators and z^2 as integers and Fractions, z correctly
rounded from them, p and Holm's step-down from mpmath at 50 digits) and against sdice_kruskal on the same arguments.

Bars, on every row of every fixture:
  tested, p, h, med, mean, delta   sdice_kruskal's on the same input, bit for bit
  pair_z                           within Z_ROUNDINGS ulps (tests/dunn_fixtures.py) of the referee's correctly rounded z -- the
                                   rounding count that the header of csrc/kruskal.hip states for its z form
                                   (tests/test_dunn_cpu.py reads it there), and never more than 8; exactly +-0 where the
                                   referee's z is 0
  pair_p, pair_padj                within 1e-9 relative of the referee where that is >= 1e-280, below 2e-280 under it
  pair_padj                        >= pair_p, <= 1, and exactly min(1, m * p) in float64 for the row's smallest p
  a row that is not tested         0 in every pair slot
The fixtures are those of tests/dunn_fixtures.py, whose rows keep their pair p-values apart (tests/test_dunn_cpu.py)."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dunn_fixtures as DF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import rank_support as RS  # noqa: E402
from dunn_fixtures import PAIR, check_pairs  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

pytestmark = pytest.mark.gpu

K12 = ("tested", "p", "h", "med", "mean", "delta")
H_RTOL = 1e-12


def check(ctx, ps, sets, ref, label):
    """the host call against sdice_kruskal on the same arguments and against the referee -> the call's result"""
    got = ctx.kruskal_dunn(ps, sets)
    kw = ctx.kruskal(ps, sets)
    assert list(got) == list(K12 + PAIR)
    for name in K12:
        assert got[name].dtype == kw[name].dtype
        RS.assert_same_bits(got[name], kw[name], (label, name, "against sdice_kruskal"))
    check_pairs(got, ref, label)
    return got


# ------------------------------------------------------------------------------ set counts, sizes, row kinds
@pytest.mark.parametrize("flavour", DF.FLAVOURS)
@pytest.mark.parametrize("k", DF.KS)
def test_set_counts(ctx, k, flavour):
    """k = 2, 3, 4, 5, 10, 11 (m = 1 .. 55 pairs: the last lane in use, and the pair (0, k - 1) whose sets sit in the first
    and the last set lane), sets of 3..8 columns, every value shape, NaNs, a starved set"""
    name = f"set count k={k} {flavour}"
    ps, sets, label = DF.fixture(name)
    ref = DF.reference(name)
    assert len(sets) == k and 0 < ref["tested"].sum() < ref["tested"].size
    got = check(ctx, ps, sets, ref, label)
    assert got["pair_z"].shape[0] == k * (k - 1) // 2 and np.any(got["pair_z"][k - 2] != 0) and np.any(got["pair_z"][-1] != 0)


@pytest.mark.parametrize("flavour", DF.FLAVOURS)
@pytest.mark.parametrize("big_first", [False, True], ids=["3v3v64", "4096v3v3"])
def test_unequal_sets(ctx, big_first, flavour):
    name = f"unequal {'4096v3v3' if big_first else '3v3v64'} {flavour}"
    ps, sets, label = DF.fixture(name)
    check(ctx, ps, sets, DF.reference(name), label)


@pytest.mark.parametrize("flavour", DF.FLAVOURS)
def test_row_kinds(ctx, flavour):
    """NaNs scattered, a set left with 2 kept values (untested: every pair slot 0), all values equal (z = 0, p = padj = 1),
    one set fully separated, heavy ties, two sets identical (z = 0 for that pair): on the grid, off it and mixed"""
    name = f"row kinds {flavour}"
    ps, sets, label = DF.fixture(name)
    ref = DF.reference(name)
    got = check(ctx, ps, sets, ref, label)
    equal = DF._kind_rows()[1] == DF.KINDS.index("all values equal")
    assert np.all(got["pair_p"][:, equal] == 1.0) and np.all(got["pair_padj"][:, equal] == 1.0)
    assert not RS.bits(got["pair_z"][:, equal]).any() and not got["h"][equal].any() and np.all(got["p"][equal] == 1.0)
    if flavour != "grid":                                # both kernels finish from the same integers
        base = ctx.kruskal_dunn(*DF.fixture("row kinds grid")[:2])
        for field in ("h", "p") + PAIR:
            RS.assert_same_bits(got[field], base[field], (label, field, "against the grid rows"))


def test_block_path_edge_values(ctx):
    """signed zeros (one tie group), subnormals (distinct values) and +-FLT_MAX through the sorting kernel"""
    ps, sets, label = DF.fixture("block edges")
    check(ctx, ps, sets, DF.reference("block edges"), label)


# ------------------------------------------------------------------------------ refusals
def _raw(ctx, symbol, ps, sets, outs):
    from splicedice_amd.engine import kruskal_sets
    cols, set_ptr = kruskal_sets(sets, ps.shape[1])
    return RS.raw_call(ctx, symbol, ps, [cols, set_ptr, len(sets)], outs, K12 + PAIR)


def _host_outs(n, k):
    from splicedice_amd.engine import KRUSKAL_DUNN_FIELDS, field_shapes
    outs = {name: np.empty(shape, dt) for name, (shape, dt) in field_shapes(KRUSKAL_DUNN_FIELDS, n, k).items()}
    for a in outs.values():
        a.view(np.uint8)[...] = 0x5A
    return outs


def test_twelve_sets_and_a_null_pair_z_are_refused_by_both_entry_points(ctx):
    """k = 12 (66 pairs) and a NULL pair_z: SDICE_ERR_ARG from the host and the device entry point, outputs untouched;
    k = 11 on the same table passes, and the context still works"""
    from splicedice_amd.engine import KRUSKAL_DUNN_FIELDS, SdiceError, field_shapes, kruskal_sets
    rng = np.random.default_rng(7600)
    ps = (rng.integers(0, 1001, size=(5, 36)) / 1000.0).astype(np.float32)
    sets12 = [np.arange(3 * i, 3 * i + 3) for i in range(12)]
    with pytest.raises(SdiceError):
        ctx.kruskal_dunn(ps, sets12)
    assert b"sdice_kruskal_dunn" in ctx.lib.sdice_last_error() and b"2..11" in ctx.lib.sdice_last_error()
    outs = _host_outs(5, 12)
    assert _raw(ctx, "sdice_kruskal_dunn", ps, sets12, outs) == -1
    assert all(np.all(RS.bits(a).view(np.uint8) == 0x5A) for a in outs.values())
    outs = _host_outs(5, 11)
    assert _raw(ctx, "sdice_kruskal_dunn", ps, sets12[:11], dict(outs, pair_z=None)) == -1
    assert b"NULL output" in ctx.lib.sdice_last_error()
    assert all(np.all(RS.bits(a).view(np.uint8) == 0x5A) for a in outs.values())
    d_ps = ctx.to_device(ps)
    for sets, drop in ((sets12, ()), (sets12[:11], ("pair_z",))):
        cols, set_ptr = kruskal_sets(sets, 36)
        d_cols = ctx.to_device(cols)
        out = {name: ctx.empty(shape, dt).memset(0x5A) for name, (shape, dt) in
               field_shapes(KRUSKAL_DUNN_FIELDS, 5, len(sets)).items()}
        handed = {name: d for name, d in out.items() if name not in drop}
        if drop:                                             # (the engine wants the key: hand the library its NULL directly)
            import ctypes as C
            args = [None if name in drop else C.c_void_p(out[name].ptr) for name in out]
            rc = ctx.lib.sdice_kruskal_dunn_dev(ctx.h, 5, 36, C.c_void_p(d_ps.ptr), C.c_void_p(d_cols.ptr),
                                                set_ptr.ctypes.data_as(C.c_void_p), len(sets), *args)
            assert rc == -1 and b"NULL output" in ctx.lib.sdice_last_error()
        else:
            with pytest.raises(SdiceError):
                ctx.kruskal_dunn_dev(d_ps, d_cols, set_ptr, handed)
        for name, d in out.items():
            assert np.all(d.to_host().view(np.uint8) == 0x5A), (len(sets), name)
            d.free()
        d_cols.free()
    d_ps.free()
    ok = ctx.kruskal_dunn(ps, sets12[:11])
    assert ok["tested"].all() and ok["pair_z"].shape == (55, 5)
    with pytest.raises(ValueError, match="one set only"):
        ctx.kruskal_dunn(ps, [[0, 1, 2], [3, 4, 5], [6, 7, 0]])


# ------------------------------------------------------------------------------ command line
def _write_cli_inputs(tmp_path, k):
    """90 rows x (6 k + 2) samples, k manifests (the second in another order and with a sample the table lacks, two columns
    in no set): sets shifted against each other, heavy ties, all-equal rows, rows with a starved set"""
    rng = np.random.default_rng(7700 + k)
    n, s = 90, 6 * k + 2
    samples, _ = RS.ps_names(n, s)
    member = np.array([j % k for j in range(6 * k)] + [-1, -1])
    shift = rng.uniform(-0.2, 0.2, size=(n, k)) * (np.arange(n)[:, None] % 3 != 0)
    v = np.clip(0.5 + np.where(member[None, :] >= 0, shift[:, member], 0.0) + 0.1 * rng.standard_normal((n, s)), 0, 1)
    v[:15] = np.round(v[:15] * 4) / 4                                      # heavy ties
    text = np.where(rng.random((n, s)) < 0.07, "nan", np.char.mod("%.3f", v))
    text[15:20] = "0.500"                                                  # all-equal rows stay in the table
    text[25:30][:, np.flatnonzero(member == 1)[1:]] = "nan"                # the second set keeps one value: rows dropped
    groups = [[samples[j] for j in np.flatnonzero(member == i)] for i in range(k)]
    groups[1] = groups[1][::-1] + ["not_in_the_table"]
    path, manifests, names = RS.write_ps_inputs(tmp_path, text, [(g, "A") for g in groups])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, manifests, [np.flatnonzero(member == i) for i in range(k)], names, matrix


@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("k", [3, 4])
def test_cli_posthoc(ctx, golden_dir, tmp_path, k, gtf):
    """compare_sample_sets -mx --posthoc against the referee's table (tests/dunn_referee.py, command_table): the header and
    every text cell -- event, means, medians, delta, every z (the engine's z is the correctly rounded one) and the GTF
    cells -- byte for byte; H, padj, p-value and corrected are float64 whose last bits the engine may miss (as in
    tests/test_gpu_kruskal.py), so those cells are parsed, held to the parity bars (H 1e-12, the others 1e-9 relative) and
    must be repr round-trips.  With the new columns cut out the file is the plain -mx file byte for byte."""
    from splicedice_amd import compare_sample_sets as css
    table, manifests, sets, names, matrix = _write_cli_inputs(tmp_path, k)
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    outs = {}
    for posthoc in (True, False):
        outs[posthoc] = str(tmp_path / f"out{int(posthoc)}.tsv")
        css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1],
                                        moreManifests=manifests[2:], posthoc=posthoc, annotation=anno, outputFile=outs[posthoc]),
                     ctx=ctx)
    ref = DR.table_reference(matrix, sets, True)
    keep = np.flatnonzero(ref["tested"])
    assert 75 < keep.size < 90 and set(range(15, 20)) <= set(keep.tolist()) and not set(range(25, 30)) & set(keep.tolist())
    assert (np.abs(ref["pair_z"][:, keep]) > 2).sum() > 10 and (ref["pair_padj"][:, keep] == 1.0).sum() > 10
    header, keep2, want = DR.command_table(ref, names, k, O.bh_fdr(ref["p"][keep]))
    assert np.array_equal(keep, keep2)
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    got = open(outs[True], "rb").read().decode()
    lines = got[:-1].split("\n")
    assert got.endswith("\n") and lines[0].split("\t") == DR.command_header(k, gtf) and len(lines) == keep.size + 1
    z_at, padj_at = DR.pair_cells(k)
    h_at, p_at = z_at[0] - 1, padj_at[-1] + 1
    for line, cells, tail in zip(lines[1:], want, sfx):
        f = line.split("\t")
        assert "\t" + "\t".join(f[len(cells):]) == tail if gtf else len(f) == len(cells)
        for at, cell in enumerate(cells):
            if isinstance(cell, str):
                assert f[at] == cell, (f[0], header[at], f[at], cell)
            else:
                assert str(np.float64(float(f[at]))) == f[at], (f[0], header[at])
                assert abs(float(f[at]) - cell) <= (H_RTOL if at == h_at else RS.P_RTOL) * abs(cell), (f[0], header[at], f[at], cell)
    # the new columns cut out: the plain -mx file
    plain = open(outs[False], "rb").read().decode()
    cut = "\n".join("\t".join(c for at, c in enumerate(line.split("\t")) if not h_at < at < p_at) for line in lines) + "\n"
    assert cut == plain
