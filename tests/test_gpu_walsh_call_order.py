"""GPU: the paired-shift calls give, bit for bit, the results of a fresh context after every case of the call-order catalogue
(tests/call_order_fixtures.py, imported as it is) and on scratch regions filled with any byte.  The catalogue lists every
`_dev` method of Context; walsh_resident stays out of it until it is next open for change, and this file is the coverage it
would have given it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import rank_support as RS  # noqa: E402
import test_gpu_walsh as T  # noqa: E402
import walsh_fixtures as WF  # noqa: E402
from splicedice_amd.engine import WALSH_FIELDS, Context, field_shapes  # noqa: E402
from walsh_referee import OUTS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (16, 129)                  # the lane-group form and the workgroup form
FILLS = (0x5A, 0xFF, 0x00)


def _resident(ctx, ps, a, b, fill):
    held = [ctx.to_device(ps, np.float32), ctx.to_device(a, np.int32), ctx.to_device(b, np.int32)]
    out = {name: ctx.empty(*sd).memset(fill) for name, sd in field_shapes(WALSH_FIELDS, ps.shape[0]).items()}
    try:
        ctx.walsh_resident(*held, out)
        ctx.sync()
        return {name: d.to_host() for name, d in out.items()}
    finally:
        for d in (*held, *out.values()):
            d.free()


def _run(ctx):
    """both entry points, both forms -> {label: array}"""
    out = {}
    for m in SHAPES:
        ps, a, b, _ = WF.table(m)
        for form, res in (("host", ctx.walsh(ps, a, b)), ("resident", _resident(ctx, ps, a, b, CF.FILL))):
            for name in OUTS:
                out[f"{m} pairs {form} {name}"] = res[name]
    return out


def _same(got, base, label):
    assert list(got) == list(base)
    for name in base:
        assert np.array_equal(RS.bits(got[name]), RS.bits(base[name])), (label, name)


@pytest.fixture(scope="module")
def fresh(ctx):
    with Context(ctx.device) as own:
        base = _run(own)
    for m in SHAPES:
        for form in ("host", "resident"):
            T.check({name: base[f"{m} pairs {form} {name}"] for name in OUTS}, WF.reference(m), (m, form))
    return base


@pytest.mark.parametrize("other", list(CF.CASES))
def test_results_after_every_case_of_the_catalogue(ctx, fresh, other):
    CF.CASES[other].run(ctx)
    _same(_run(ctx), fresh, f"after {other}")


@pytest.mark.parametrize("fill", FILLS, ids=lambda b: f"fill_{b:02X}")
def test_results_on_filled_scratch(ctx, fresh, fill):
    CF.CASES["bh vector radix"].run(ctx)            # (leaves an arena chunk to fill: these calls take nothing from it)
    filled = ctx.scratch_regions()
    assert filled
    for _, d in filled:
        d.memset(fill)
    _same(_run(ctx), fresh, f"scratch filled with {fill:#04x}")
