"""The host code that the entry points share (rowsum.h: zero_two_sample, stage_two_sample; common.h: the result block of
HostStaging; engine.py: the pointer list of a _dev call), through the engine, at the smallest shapes where it can go wrong:
n = 131 rows (no multiple of 64; a field of 131 bytes or 524 ends off every alignment) and, for the result block, n = 1.

* Nothing testable (2 v 5 columns, 2 pairs): the _dev call leaves every field, `exact` included, all zero bytes on buffers
  that held 0xAA, with z passed and without; a z buffer that is not passed keeps its 0xAA.
* The host form gives the _dev form's bytes in every field: 3-decimal values with about 10 % NaN, a row of NaNs and an
  off-grid row, at 3 v 4 columns (3 pairs: the lane and lane-group kernels) and at 40 v 30 columns (70 pairs: the
  workgroup-per-row kernels of signedrank.hip, strata.hip and ks.hip, the 64-lane rank-sum path).  Stratum ids are
  column % 3.  sdice_ks (`ks`, and `ks_exact` = exact=True): d rides in the z slot, `exact` is an output of both.
* The same for the entry points with fields of their own, at 131 rows and at 1: kruskal and jonckheere over the three sets
  of call_order_fixtures.SETS (med and mean are [3, n]), spearman at 7 and 70 columns, shift at 3 v 4 and 40 v 30,
  sample_gram and rowstats (float32, float64) at 5 columns, similarity at 8 samples.
* An optional output (z, h, j, rho, d, sdice_ks's exact) passed as NULL to the C entry point: status 0, and every other
  field has the bytes of the call that passed it."""
import functools

import numpy as np
import pytest

import rank_support as RS
from call_order_fixtures import SETS
from splicedice_amd.engine import (GRAM_FIELDS, JONCKHEERE_FIELDS, KRUSKAL_FIELDS, KS_FIELDS, RANKSUM_EXACT_FIELDS,
                                   RANKSUM_FIELDS, SHIFT_FIELDS, SPEARMAN_FIELDS, field_shapes, kruskal_sets, spearman_order)

gpu = pytest.mark.gpu

N = 131
ENTRIES = ("ranksum", "ranksum_exact", "ranksum_strata", "signedrank", "signedrank_exact", "ks", "ks_exact")
SHAPES = ((3, 4, 3), (40, 30, 70))          # group 1, group 2, pairs


def fields_of(entry):
    if entry.startswith("ks"):
        return KS_FIELDS
    return RANKSUM_EXACT_FIELDS if entry.endswith("_exact") else RANKSUM_FIELDS


def lists_of(entry, n1, n2, m):
    """the column lists of an entry point: two groups (+ their stratum ids) or the two sides of m pairs"""
    if entry.startswith("signedrank"):
        return [np.arange(m, dtype=np.int32), np.arange(m, 2 * m, dtype=np.int32)]
    g1, g2 = np.arange(n1, dtype=np.int32), np.arange(n1, n1 + n2, dtype=np.int32)
    return [g1, g2, g1 % 3, g2 % 3] if entry == "ranksum_strata" else [g1, g2]


def call_dev(ctx, entry, d_ps, d_lists, out):
    if entry == "ranksum_strata":
        ctx.ranksum_strata_dev(d_ps, *d_lists, 3, out)
    elif entry.startswith("ks"):
        ctx.ks_dev(d_ps, *d_lists, out, exact=entry == "ks_exact")
    else:
        getattr(ctx, entry + "_dev")(d_ps, *d_lists, out)


def call_host(ctx, entry, ps, lists):
    if entry.startswith("ks"):
        return ctx.ks(ps, *lists, exact=entry == "ks_exact")
    return getattr(ctx, entry)(ps, *lists)


def device_fields(ctx, entry, byte):
    return {f[0]: ctx.empty(N, f[1]).memset(byte) for f in fields_of(entry)}


def make_table(n1, n2, m, n=N):
    """n rows (a table of fewer than 65 rows has no off-grid row, of fewer than 18 no row of NaNs either)"""
    s = max(n1 + n2, 2 * m) + 1
    rng = np.random.default_rng(1000 * n1 + n2)
    ps = (rng.integers(0, 1001, size=(n, s)) / 1000.0).astype(np.float32)
    ps[rng.random((n, s)) < 0.10] = np.nan
    ps[17:18] = np.nan
    ps[64:65] = rng.random(s, dtype=np.float32) * np.float32(0.999) + np.float32(1e-4)    # off the 3-decimal grid
    return ps


@gpu
@pytest.mark.parametrize("with_z", (True, False), ids=("z", "no z"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_nothing_testable_zeroes_every_field(ctx, entry, with_z):
    ps = make_table(2, 5, 2)                 # 131 x 8
    d_ps = ctx.to_device(ps)
    d_lists = [ctx.to_device(v) for v in lists_of(entry, 2, 5, 2)]
    out = device_fields(ctx, entry, 0xAA)
    z = "d" if entry.startswith("ks") else "z"
    d_z = out[z]
    if not with_z:
        del out[z]
    call_dev(ctx, entry, d_ps, d_lists, out)
    for name, d in out.items():
        assert not np.frombuffer(d.to_host().tobytes(), np.uint8).any(), name
    if not with_z:
        assert (np.frombuffer(d_z.to_host().tobytes(), np.uint8) == 0xAA).all()
    for d in [d_ps, d_z, *d_lists, *out.values()]:
        d.free()


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dv%d_%dpairs" % v)
@pytest.mark.parametrize("entry", ENTRIES)
def test_host_form_gives_the_dev_form_bytes(ctx, entry, shape):
    ps = make_table(*shape)
    lists = lists_of(entry, *shape)
    host = call_host(ctx, entry, ps, lists)
    d_ps = ctx.to_device(ps)
    d_lists = [ctx.to_device(v) for v in lists]
    out = device_fields(ctx, entry, 0xAA)
    call_dev(ctx, entry, d_ps, d_lists, out)
    assert list(host) == [f[0] for f in fields_of(entry)]
    for name, d in out.items():
        dev = d.to_host()
        assert host[name].dtype == dev.dtype and host[name].shape == dev.shape, name
        assert host[name].tobytes() == dev.tobytes(), name
    assert host["tested"].any() and not host["tested"].all()       # the table has rows of both kinds
    for d in [d_ps, *d_lists, *out.values()]:
        d.free()


# ------------------------------------------------------------------------------ the entry points with fields of their own
ROWS = (N, 1)
SET_COLS = 40                    # the columns SETS reach into


def _on_device(ctx, arrays, shapes):
    """-> (device copies of `arrays`, sentinel-filled device fields of `shapes` = name: (shape, dtype))"""
    return [ctx.to_device(a) for a in arrays], {k: ctx.empty(sh, dt).memset(0xAA) for k, (sh, dt) in shapes.items()}


def _sets(entry, fields, ctx, n):
    ps = make_table(SET_COLS, 0, 0, n)
    host = getattr(ctx, entry)(ps, SETS)
    cols, set_ptr = kruskal_sets(SETS, ps.shape[1])
    held, out = _on_device(ctx, [ps, cols], field_shapes(fields, n, len(SETS)))
    getattr(ctx, entry + "_dev")(*held, set_ptr, out)
    return host, out, held


def _spearman(m, ctx, n):
    ps = make_table(m, 0, 0, n)
    cols, x = np.arange(m)[::-1], (np.arange(m) % 5).astype(np.float64)      # a tied covariate
    host = ctx.spearman(ps, cols, x)
    held, out = _on_device(ctx, [ps, *spearman_order(cols, x)], field_shapes(SPEARMAN_FIELDS, n))
    ctx.spearman_dev(*held, out)
    return host, out, held


def _shift(n1, n2, ctx, n):
    ps = make_table(n1, n2, 0, n)
    g1, g2 = lists_of("shift", n1, n2, 0)
    host = ctx.shift(ps, g1, g2)
    held, out = _on_device(ctx, [ps, g1, g2], field_shapes(SHIFT_FIELDS, n))
    ctx.shift_dev(*held, out)
    return host, out, held


def _gram(ctx, n):
    ps = make_table(10, 0, 0, n)
    ps[64:65] = np.float32(0.25)                              # (sample_gram refuses a value off the grid)
    cols = np.array([4, 9, 0, 7, 2], np.int32)
    host = ctx.sample_gram(ps, cols)
    held, out = _on_device(ctx, [ps, cols], field_shapes(GRAM_FIELDS, (5, 5)))
    ctx.sample_gram_dev(*held, out)
    return host, out, held


def _rowstats(dtype, ctx, n):
    data = make_table(10, 0, 0, n).astype(dtype)
    idx = np.array([4, 9, 0, 7, 2], np.int32)
    host = dict(zip(("mean", "std", "n_nan"), ctx.rowstats(data, idx)))
    held, out = _on_device(ctx, [data, idx], dict(mean=(n, dtype), std=(n, dtype), n_nan=(n, np.int32)))
    ctx.rowstats_dev(*held, out["mean"], out["std"], out["n_nan"])
    return host, out, held


def _similarity(ctx, n):
    ps = make_table(7, 0, 0, n).astype(np.float64)            # s = 8
    rng = np.random.default_rng(8)
    mid, sign = np.round(rng.random(n), 3), rng.integers(-1, 2, size=n).astype(np.int8)
    host = dict(zip(("scores", "counts"), ctx.similarity(ps, mid, sign)))
    held, out = _on_device(ctx, [ps, mid, sign], dict(scores=(8, np.int64), counts=(8, np.int64)))
    ctx.similarity_dev(*held, out["scores"], out["counts"])
    return host, out, held


OWN_FIELDS = {
    "kruskal": functools.partial(_sets, "kruskal", KRUSKAL_FIELDS),
    "jonckheere": functools.partial(_sets, "jonckheere", JONCKHEERE_FIELDS),
    "spearman_7": functools.partial(_spearman, 7),
    "spearman_70": functools.partial(_spearman, 70),
    "shift_3v4": functools.partial(_shift, 3, 4),
    "shift_40v30": functools.partial(_shift, 40, 30),
    "sample_gram": _gram,
    "rowstats_float32": functools.partial(_rowstats, np.float32),
    "rowstats_float64": functools.partial(_rowstats, np.float64),
    "similarity": _similarity,
}


@gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("entry", OWN_FIELDS)
def test_host_form_gives_the_dev_form_bytes_in_fields_of_its_own(ctx, entry, n):
    host, out, held = OWN_FIELDS[entry](ctx, n)
    assert list(host) == list(out)
    for name, d in out.items():
        dev = d.to_host()
        assert host[name].dtype == dev.dtype and host[name].shape == dev.shape, name
        assert host[name].tobytes() == dev.tobytes(), name
    if "tested" in host and n == N:
        assert host["tested"].any() and not host["tested"].all()   # the table has rows of both kinds
    for d in [*held, *out.values()]:
        d.free()


def _names(fields):
    return [f[0] for f in fields]


def _two_groups(extra=()):
    g1, g2 = lists_of("ranksum", 3, 4, 3)
    return make_table(3, 4, 3), (g1, 3, g2, 4, *extra)


def _pairs():
    a, b = lists_of("signedrank", 3, 4, 3)
    return make_table(3, 4, 3), (a, b, 3)


def _k_sets():
    cols, set_ptr = kruskal_sets(SETS, SET_COLS + 1)
    return make_table(SET_COLS, 0, 0), (cols, set_ptr, len(SETS))


def _covariate():
    cols, xg = spearman_order(np.arange(7)[::-1], (np.arange(7) % 5).astype(np.float64))
    return make_table(7, 0, 0), (cols, xg, 7)


# symbol, the optional output, (table, arguments), the field table
OPTIONAL = [
    ("sdice_ranksum", "z", _two_groups, RANKSUM_FIELDS),
    ("sdice_ranksum_exact", "z", _two_groups, RANKSUM_EXACT_FIELDS),
    ("sdice_ranksum_strata", "z", lambda: _two_groups((np.arange(3) % 3, np.arange(3, 7) % 3, 3)), RANKSUM_FIELDS),
    ("sdice_signedrank", "z", _pairs, RANKSUM_FIELDS),
    ("sdice_signedrank_exact", "z", _pairs, RANKSUM_EXACT_FIELDS),
    ("sdice_ks", "d", lambda: _two_groups((0,)), KS_FIELDS),
    ("sdice_ks", "exact", lambda: _two_groups((0,)), KS_FIELDS),
    ("sdice_kruskal", "h", _k_sets, KRUSKAL_FIELDS),
    ("sdice_jonckheere", "j", _k_sets, JONCKHEERE_FIELDS),
    ("sdice_spearman", "rho", _covariate, SPEARMAN_FIELDS),
]


@gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("symbol,optional,inputs,fields", OPTIONAL, ids=[f"{c[0]}-{c[1]}" for c in OPTIONAL])
def test_an_optional_output_left_out_changes_no_other(ctx, symbol, optional, inputs, fields, n):
    ps, args = inputs()
    ps = ps[:n]
    k = len(SETS) if symbol in ("sdice_kruskal", "sdice_jonckheere") else None
    got = []
    for leave_out in (False, True):
        outs = {name: np.full(sh, 0x55, dt) for name, (sh, dt) in field_shapes(fields, n, k).items()}
        if leave_out:
            outs[optional] = None
        assert RS.raw_call(ctx, symbol, ps, args, outs, _names(fields)) == 0, (leave_out, ctx.lib.sdice_last_error())
        got.append(outs)
    full, partial = got
    for name in _names(fields):
        if name != optional:
            assert partial[name].tobytes() == full[name].tobytes(), name
    if n == N:
        assert full["tested"].any() and not full["tested"].all()
