"""The host code that the two-sample entry points share (rowsum.h: zero_two_sample, TwoSampleStaging; engine.py: the
pointer list of a _dev call), through the engine, at the smallest shapes where it can go wrong: n = 131 rows (no
multiple of 64).

* Nothing testable (2 v 5 columns, 2 pairs): the _dev call leaves every field, `exact` included, all zero bytes on buffers
  that held 0xAA, with z passed and without; a z buffer that is not passed keeps its 0xAA.
* The host form gives the _dev form's bytes in every field: 3-decimal values with about 10 % NaN, a row of NaNs and an
  off-grid row, at 3 v 4 columns (3 pairs: the lane and lane-group kernels) and at 40 v 30 columns (70 pairs: the
  workgroup-per-row kernels of signedrank.hip, strata.hip and ks.hip, the 64-lane rank-sum path).  Stratum ids are
  column % 3.  sdice_ks (`ks`, and `ks_exact` = exact=True): d rides in the z slot, `exact` is an output of both."""
import numpy as np
import pytest

from splicedice_amd.engine import KS_FIELDS, RANKSUM_EXACT_FIELDS, RANKSUM_FIELDS

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


def make_table(n1, n2, m):
    s = max(n1 + n2, 2 * m) + 1
    rng = np.random.default_rng(1000 * n1 + n2)
    ps = (rng.integers(0, 1001, size=(N, s)) / 1000.0).astype(np.float32)
    ps[rng.random((N, s)) < 0.10] = np.nan
    ps[17] = np.nan
    ps[64] = rng.random(s, dtype=np.float32) * np.float32(0.999) + np.float32(1e-4)       # off the 3-decimal grid
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
