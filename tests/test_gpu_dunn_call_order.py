"""The Dunn call under the rules of tests/test_gpu_call_order.py: its result must not depend on what the context held before
the call.  Context.kruskal_dunn_resident (sdice_kruskal_dunn_dev) is run on the row table of tests/call_order_fixtures.py
with its three sets (12, 13 and 13 columns; rows on the grid and off it, so both kernels run) on outputs filled with 0x5A
first,

  b. after every case of that catalogue on the shared context, against a run alone on a context of its own;
  c. on scratch regions filled with 0x5A, 0xFF and 0x00 over their whole length.

The comparison with the referee (tests/dunn_referee.py) is that of tests/test_gpu_dunn.py (check_pairs), the K12 fields
against the catalogue's own kruskal case; two runs are compared on their bit patterns.  The call resets the arena and takes
nothing from it (arena=False), like the other row tests of the catalogue.  The first test needs no GPU: the case has a
reference that says something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import rank_support as RS  # noqa: E402
from splicedice_amd.engine import KRUSKAL_DUNN_FIELDS, Context, field_shapes, kruskal_sets  # noqa: E402
from test_gpu_dunn import PAIR, check_pairs  # noqa: E402

gpu = pytest.mark.gpu
FILLS = (0x5A, 0xFF, 0x00)
OUTS = tuple(f[0] for f in KRUSKAL_DUNN_FIELDS)


def _run(ctx, x):
    cols, set_ptr = kruskal_sets(CF.SETS, CF.ROW_COLS)
    d_ps, d_cols = ctx.to_device(x["ps"]), ctx.to_device(cols)
    out = {name: ctx.empty(shape, dtype).memset(CF.FILL) for name, (shape, dtype) in
           field_shapes(KRUSKAL_DUNN_FIELDS, CF.ROWS, len(CF.SETS)).items()}
    ctx.kruskal_dunn_resident(d_ps, d_cols, set_ptr, out)
    got = {name: d.to_host() for name, d in out.items()}
    for d in (*out.values(), d_ps, d_cols):
        d.free()
    return got


def _check(got, want, label):
    CF.CASES["kruskal"].check({name: got[name] for name in CF.CASES["kruskal"].outputs}, label)
    check_pairs(got, want, label)


# (a Case of its own, not an entry of CF.CASES: the catalogue's tests keep their parameters)
CASE = CF.Case("kruskal_dunn", lambda: dict(ps=CF.row_table()), _run, lambda x: DR.table_reference(x["ps"], CF.SETS, False),
               _check, OUTS, arena=False)


def _same_run(got, base, label):
    assert list(got) == list(base), label
    for name in base:
        assert np.array_equal(RS.bits(got[name]), RS.bits(base[name])), (label, name, "differs from the other run")


def test_the_case_has_a_reference_that_says_something():
    """tests/test_call_order_fixtures_cpu.py's conditions: tested takes both values, no pair output is all zero, tested
    rows on the grid and off it; and no Holm order of a row hangs on a rounding"""
    want = CASE.want
    t = want["tested"].astype(bool)
    assert set(np.unique(want["tested"]).tolist()) == {0, 1}
    assert all(np.any(want[name] != 0) and not np.isnan(want[name]).any() for name in PAIR)
    grid = RS.on_grid(CF.row_table()).all(axis=1)
    assert (t & grid).sum() >= 50 and (t & ~grid).sum() >= 15 and (~t).sum() >= 10
    assert DR.close_pairs(want, 1e-6) == []
    assert (want["pair_padj"][:, t] == 1.0).any() and (want["pair_padj"][:, t] < 0.05).any()
    assert CASE.want is want


@gpu
def test_result_ignores_what_the_call_before_left(ctx):
    with Context(ctx.device) as own:
        base = CASE.run(own)
    CASE.check(base, "alone on a context of its own")
    for other in CF.CASES:
        CF.CASES[other].run(ctx)
        _same_run(CASE.run(ctx), base, f"kruskal_dunn after {other}")


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
    _same_run(got, first, f"kruskal_dunn on scratch filled with {fill:#04x}")
    CASE.check(got, f"scratch filled with {fill:#04x}")
