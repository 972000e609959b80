"""Dunn's-test sweeps: sdice_kruskal_dunn at the column counts, table shapes and call patterns that the fixtures of
tests/test_gpu_dunn.py do not reach, under that file's bars (check, check_pairs).

- column counts: three sets over every total of 9..66 and 127..129 selected columns, on the grid, off it and mixed;
- rows per wave: tables of 64 x compute_units x ch rows for ch = 64, 32, 8, 2 from the palette of row kinds of the
  Kruskal-Wallis sweeps (tests/kset_fixtures.py), reached as tests/test_gpu_kruskal_sweeps.py reaches them: more rows than
  one grid pass of either kernel, KW_REDO rows among tested, untested and grid rows.  The ch = 64 table also goes through
  sdice_kruskal_dunn_dev on outputs filled with 0x5A, once with every output and once with h, pair_p and pair_padj absent;
- row slices of one table equal the slices of the whole table's result;
- the sets in another order: the z's permute and negate, p and padj permute, all bit for bit;
- a ladder that takes one pair's z from 0 to 45.8, so that its p runs through every band down to 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dunn_fixtures as DF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import rank_support as RS  # noqa: E402
from kset_fixtures import CHS, PALETTE_S, palette, palette_index  # noqa: E402
from rank_support import chunk_table_rows  # noqa: E402
from test_gpu_dunn import K12, PAIR, check, check_pairs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flavour", DF.FLAVOURS)
def test_column_counts(ctx, flavour):
    """every total column count 9..66 and 127..129 (the staging loop's rounds of 64 lanes, the compaction's rounds, the
    sort lengths 16..256 of the sorting kernel)"""
    tested = 0
    for (ps, sets, label), ref in zip(DF.column_count_fixtures(flavour), DF.column_count_references(flavour)):
        got = check(ctx, ps, sets, ref, label)
        tested += int(got["tested"].sum())
    assert tested > 300


@pytest.mark.parametrize("ch", CHS)
def test_rows_per_wave(ctx, ch):
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    rows, sets, _ = palette()
    idx = palette_index(n)
    ps = np.ascontiguousarray(rows[idx])
    ref = RS.scatter({name: v for name, v in DF.palette_reference().items() if name != "exact"}, idx)
    got = check(ctx, ps, sets, ref, f"ch={ch} n={n} on {cus} CUs")
    if ch != 64:
        return
    assert n > 256 * 8 * cus
    from splicedice_amd.engine import KRUSKAL_DUNN_FIELDS, field_shapes, kruskal_sets
    cols, set_ptr = kruskal_sets(sets, PALETTE_S)
    d_ps, d_cols = ctx.to_device(ps), ctx.to_device(cols)
    try:
        for absent in ((), ("h", "pair_p", "pair_padj")):
            out = {name: ctx.empty(shape, dtype).memset(0x5A) for name, (shape, dtype) in
                   field_shapes(KRUSKAL_DUNN_FIELDS, n, 3).items() if name not in absent}
            try:
                ctx.kruskal_dunn_dev(d_ps, d_cols, set_ptr, out)
                for name, d in out.items():
                    RS.assert_same_bits(d.to_host(), got[name], ("sdice_kruskal_dunn_dev without", absent, name))
            finally:
                for d in out.values():
                    d.free()
    finally:
        d_ps.free()
        d_cols.free()


def test_optional_outputs_absent_in_the_host_call(ctx):
    """pair_p and / or pair_padj NULL: every other output is what it is with them"""
    ps, sets, label = DF.fixture("set count k=5 mixed")
    full = ctx.kruskal_dunn(ps, sets)
    for want_p, want_padj in ((False, True), (True, False), (False, False)):
        got = ctx.kruskal_dunn(ps, sets, pair_p=want_p, pair_padj=want_padj)
        assert ("pair_p" in got) == want_p and ("pair_padj" in got) == want_padj
        for name, v in got.items():
            RS.assert_same_bits(v, full[name], (label, name, want_p, want_padj))
        check_pairs(got, DF.reference("set count k=5 mixed"), label)


def test_row_slices(ctx):
    ps, sets, label = DF.fixture("set count k=4 mixed")
    full = ctx.kruskal_dunn(ps, sets)
    for a, b in ((0, 1), (1, 4), (3, 8), (7, 8), (2, 2)):
        got = ctx.kruskal_dunn(np.ascontiguousarray(ps[a:b]), sets)
        for name in K12 + PAIR:
            RS.assert_same_bits(got[name], full[name][..., a:b], (label, name, a, b))


@pytest.mark.parametrize("name", ["set count k=5 grid", "set count k=5 off", "set count k=11 mixed", "row kinds mixed"])
def test_sets_in_another_order(ctx, name):
    """a permutation of the sets: pair (a, b) of the new order holds the old sets perm[a], perm[b]; its z is the old pair's,
    negated where the pair turned round, bit for bit (+0.0 stays +0.0); p and padj are the old pair's bit for bit; H and
    the K12 p are unchanged, med and mean permute"""
    ps, sets, label = DF.fixture(name)
    k = len(sets)
    base = ctx.kruskal_dunn(ps, sets)
    perm = np.random.default_rng(k).permutation(k)
    assert not np.array_equal(perm, np.arange(k))
    got = ctx.kruskal_dunn(ps, [sets[i] for i in perm])
    for field in ("tested", "p", "h", "delta"):
        RS.assert_same_bits(got[field], base[field], (label, field))
    for field in ("med", "mean"):
        RS.assert_same_bits(got[field], base[field][perm], (label, field))
    where = {pr: q for q, pr in enumerate(DR.pairs(k))}
    turned = 0
    for q, (a, b) in enumerate(DR.pairs(k)):
        i, j = int(perm[a]), int(perm[b])
        old = where[(min(i, j), max(i, j))]
        zo = base["pair_z"][old]
        RS.assert_same_bits(got["pair_z"][q], zo if i < j else np.where(zo == 0, zo, -zo), (label, "z of pair", q))
        RS.assert_same_bits(got["pair_p"][q], base["pair_p"][old], (label, "p of pair", q))
        RS.assert_same_bits(got["pair_padj"][q], base["pair_padj"][old], (label, "padj of pair", q))
        turned += i > j
    assert turned > 0


@pytest.mark.parametrize("flavour", ["grid", "off"])
def test_p_ladder(ctx, flavour):
    """z of the first pair from 0 to sqrt(3 * 1400 / 2) = 45.8: p within 1e-9 of mpmath's down to 1e-280, under 2e-280 below
    that and 0 at the end; padj follows"""
    name = f"ladder {flavour}"
    ps, sets, label = DF.fixture(name)
    ref = DF.reference(name)
    got = check(ctx, ps, sets, ref, label)
    assert got["pair_z"][0, 0] == 0 and got["pair_p"][0, 0] == 1.0
    assert got["pair_z"][0, -1] > 38 and got["pair_p"][0, -1] == 0.0 and got["pair_padj"][0, -1] == 0.0
    assert np.any((got["pair_p"][0] > 0) & (got["pair_p"][0] < 1e-200))
