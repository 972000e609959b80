"""The shift call under the rules of tests/test_gpu_call_order.py: its result must not depend on what the context held
before the call.  Context.shift_resident (sdice_shift_dev) is run on the row table of tests/call_order_fixtures.py, 18 v 19
columns on outputs filled with 0x5A first,

  b. after every case of that catalogue on the shared context, against a run alone on a context of its own;
  c. on scratch regions filled with 0x5A, 0xFF and 0x00 over their whole length.

The comparison with the referee (tests/shift_referee.py) is bit for bit on every field, as in tests/test_gpu_shift.py; two
runs are compared on their bit patterns.  The call resets the arena and takes nothing from it (arena=False), like the
other row tests of the catalogue.  The first test needs no GPU: the case has a reference that says something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import rank_support as RS  # noqa: E402
import shift_referee as SH  # noqa: E402
from splicedice_amd.engine import SHIFT_FIELDS, Context, field_shapes  # noqa: E402

gpu = pytest.mark.gpu
FILLS = (0x5A, 0xFF, 0x00)


def _run(ctx, x):
    d_ps, d_g1, d_g2 = ctx.to_device(x["ps"]), ctx.to_device(CF.G1), ctx.to_device(CF.G2)
    out = {name: ctx.empty(shape, dtype).memset(CF.FILL) for name, (shape, dtype) in field_shapes(SHIFT_FIELDS, CF.ROWS).items()}
    ctx.shift_resident(d_ps, d_g1, d_g2, out)
    got = {name: d.to_host() for name, d in out.items()}
    for d in (*out.values(), d_ps, d_g1, d_g2):
        d.free()
    return got


def _check(got, want, label):
    for name in SH.OUTS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name)
        assert np.array_equal(RS.bits(got[name]), RS.bits(want[name])), (label, name)


# (a Case of its own, not an entry of CF.CASES: the catalogue's tests keep their parameters)
CASE = CF.Case("shift", lambda: dict(ps=CF.row_table()), _run,
               lambda x: SH.table_reference(x["ps"], CF.G1, CF.G2, SH.zq_of(0.95)), _check, SH.OUTS, arena=False)


def _same_run(got, base, label):
    assert list(got) == list(base), label
    for name in base:
        assert np.array_equal(RS.bits(got[name]), RS.bits(base[name])), (label, name, "differs from the other run")


def test_the_case_has_a_reference_that_says_something():
    """tests/test_call_order_fixtures_cpu.py's conditions: tested takes both values, no output is all zero, no NaN triple
    (the table keeps no infinity), rows on the grid and off it; and every rank is far from a rounding"""
    want = CASE.want
    t = want["tested"].astype(bool)
    assert set(np.unique(want["tested"]).tolist()) == {0, 1}
    assert all(np.any(want[name] != 0) and not np.isnan(want[name]).any() for name in SH.OUTS)
    assert want["grid"][t].any() and not want["grid"][t].all()
    assert np.unique(want["rank"][t]).size > 10
    for n1, n2 in {(int(a), int(b)) for a, b in zip(want["n1"][t], want["n2"][t])}:
        assert SH.rank_and_margin(n1, n2, SH.zq_of(0.95))[1] >= 1e-6, (n1, n2)
    assert CASE.want is want


@gpu
def test_result_ignores_what_the_call_before_left(ctx):
    with Context(ctx.device) as own:
        base = CASE.run(own)
    CASE.check(base, "alone on a context of its own")
    for other in CF.CASES:
        CF.CASES[other].run(ctx)
        _same_run(CASE.run(ctx), base, f"shift after {other}")


@gpu
@pytest.mark.parametrize("fill", FILLS, ids=lambda b: f"fill_{b:02X}")
def test_result_ignores_scratch_contents(ctx, fill):
    CF.CASES["bh vector radix"].run(ctx)                     # (so that there is an arena to fill)
    first = CASE.run(ctx)
    CASE.check(first, "first run")
    filled = ctx.scratch_regions()
    assert filled
    for _, d in filled:
        d.memset(fill)
    got = CASE.run(ctx)
    _same_run(got, first, f"shift on scratch filled with {fill:#04x}")
    CASE.check(got, f"scratch filled with {fill:#04x}")
