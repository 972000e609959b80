"""GPU: the Friedman and Page calls give, bit for bit, the results of a fresh context after every case of the call-order
catalogue (tests/call_order_fixtures.py, imported as it is) and on scratch regions filled with any byte.  The catalogue
lists every `_dev` method of Context; friedman_resident / page_resident stay out of it until it is next open for change,
and this file is the coverage it would have given them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import friedman_fixtures as FF  # noqa: E402
import friedman_referee as FR  # noqa: E402
import rank_support as RS  # noqa: E402
from splicedice_amd.engine import Context  # noqa: E402

pytestmark = pytest.mark.gpu

TESTS = ("friedman", "page")
SHAPES = ((3, 16), (5, 300))        # the wave form and the workgroup form
FILLS = (0x5A, 0xFF, 0x00)


def _inputs():
    rng = np.random.default_rng(4100)
    made = []
    for k, m in SHAPES:
        sets, s = FF.draw_sets(rng, k, m)
        made.append((sets, np.concatenate([FF.table(rng, sets, s, t)[0] for t in range(3)])))
    return made


INPUTS = _inputs()


def _run(ctx):
    """both tests, both entry points, both forms -> {label: array}"""
    out = {}
    for (k, m), (sets, ps) in zip(SHAPES, INPUTS):
        for test in TESTS:
            for form, res in (("host", getattr(ctx, test)(ps, list(sets))), ("resident", FF.resident(ctx, test, ps, sets, fill=CF.FILL))):
                for name in FF.TEST_OUTS[test]:
                    out[f"{test} {k}x{m} {form} {name}"] = res[name]
    return out


def _same(got, base, label):
    assert list(got) == list(base)
    for name in base:
        assert np.array_equal(RS.bits(got[name]), RS.bits(base[name])), (label, name)


@pytest.fixture(scope="module")
def fresh(ctx):
    with Context(ctx.device) as own:
        base = _run(own)
    worst = FF.Worst()
    for (k, m), (sets, ps) in zip(SHAPES, INPUTS):
        ref = FR.table_reference(ps, sets)
        for test in TESTS:
            FF.check(test, {name: base[f"{test} {k}x{m} host {name}"] for name in FF.TEST_OUTS[test]}, ref, (test, k, m), worst)
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
