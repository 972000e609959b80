"""similarity_kernel (K8, csrc/similarity.hip) against the referee (tests/scoring_referee.py): the column loop at and
around every pass of 256 lanes, row counts on both sides of the point where a block takes more than 16 rows, edge
values at full float64 precision, every kind of sign byte, the device entry point, the refusals, and the command on
the inputs whose reports the reference wrote (tests/golden/similarity_edge).

Every comparison is int64 equality of both vectors; there is no tolerance in this file.  The CPU check (not gpu-marked)
shows that the row counts pass the 16-row block on a part of 256 compute units; the GPU test asserts it for the device.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scoring_fixtures as SF  # noqa: E402
import scoring_referee as R  # noqa: E402
from rank_support import NOMINAL_CUS  # noqa: E402

gpu = pytest.mark.gpu
ERR_ARG = -1
SLICES = lambda n: ((0, 1), (7, 64), (100, 180), (n - 3, 3))     # noqa: E731  (start, length) of the row slices


def _table(n, s, seed):
    """3-decimal PS values (many equal to the 3-decimal midpoint), 10 % NaN, a third of the rows with sign 0"""
    rng = np.random.default_rng(seed)
    ps = np.round(rng.random((n, s)), 3)
    ps[rng.random((n, s)) < 0.1] = np.nan
    return ps, np.round(rng.random(n), 3), rng.integers(-1, 2, size=n).astype(np.int8)


def _check(ctx, ps, mid, sign, label):
    got, want = ctx.similarity(ps, mid, sign), R.similarity_counts(ps, mid, sign)
    for name, g, w in zip(("scores", "counts"), got, want):
        assert g.dtype == np.int64 and g.shape == w.shape
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (label, name, bad.size, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())
    return got


def rows_per_block(n, compute_units):
    """the launch rule of sdice_similarity_dev restated"""
    return max(16, -(-n // (8 * compute_units)))


def row_count_cases(compute_units):
    return [1, 15, 16, 17, 33, 128 * compute_units - 1, 128 * compute_units, 128 * compute_units + 1,
            3 * 128 * compute_units + 7]


def test_row_count_cases_pass_the_16_row_block_on_the_nominal_part():
    """(not gpu-marked) on 256 compute units the last two cases take 17 and 49 rows per block and end in a short block"""
    cases = row_count_cases(NOMINAL_CUS)
    assert [rows_per_block(n, NOMINAL_CUS) for n in cases] == [16] * 7 + [17, 49]
    assert all(n > 128 * NOMINAL_CUS and n % rows_per_block(n, NOMINAL_CUS) for n in cases[7:])


# ------------------------------------------------------------------------------ shapes
@gpu
@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000])
def test_column_counts(ctx, s):
    ps, mid, sign = _table(40, s, 100 + s)
    assert (sign == 0).any() and (sign < 0).any() and (sign > 0).any()
    _, counts = _check(ctx, ps, mid, sign, s)
    assert counts.max() > 0


@gpu
@pytest.mark.parametrize("which", range(9))
def test_row_counts(ctx, which):
    cu = ctx.device_info()["compute_units"]
    n = row_count_cases(cu)[which]
    if which >= 7:
        assert n > 128 * cu and rows_per_block(n, cu) == (17, 49)[which - 7]       # (and on 256 CUs a short final block)
    else:
        assert rows_per_block(n, cu) == 16
    ps, mid, sign = _table(n, 3, 200 + which)
    _check(ctx, ps, mid, sign, n)


# ------------------------------------------------------------------------------ values
@gpu
def test_edge_values(ctx):
    ps, mid, sign, kinds = SF.edge_table()
    assert ps.shape[1] == SF.EDGE_S and ps.dtype == np.float64
    scores, counts = _check(ctx, ps, mid, sign, "edge table")
    assert not counts[SF.EDGE_LIVE:].any() and not scores[SF.EDGE_LIVE:].any()     # NaN in every scored row
    # the first five kinds, each row alone, against what tests/scoring_fixtures.py writes out by hand
    for k, ((kind, values, m), (minus, plus)) in enumerate(zip(SF.edge_rows(), SF.edge_hand())):
        for sg, want in ((-1, minus), (1, plus)):
            got = ctx.similarity(values[None, :], np.array([m]), np.array([sg], np.int8))
            assert np.array_equal(got[0], want.astype(np.int64)), (k, kind, sg)
            assert np.array_equal(got[1], np.ones(SF.EDGE_LIVE, np.int64)), (k, kind, sg)
    # every row alone, so that a row kind cannot hide behind another one's counts
    for r in np.flatnonzero(sign != 0):
        _check(ctx, ps[r:r + 1], mid[r:r + 1], sign[r:r + 1], (int(r), kinds[r]))


@gpu
def test_sign_bytes(ctx):
    """the ABI reads sign < 0, sign == 0, anything else"""
    ps, mid, _ = _table(49, 70, 300)
    sign = np.tile(np.array([-128, -2, -1, 0, 1, 2, 127], np.int8), 7)
    got = _check(ctx, ps, mid, sign, "sign bytes")
    assert all(np.array_equal(a, b) for a, b in zip(got, ctx.similarity(ps, mid, np.sign(sign).astype(np.int8))))


# ------------------------------------------------------------------------------ device entry
def _filled(ctx, s, byte=0x5A):
    return ctx.empty(s, np.int64).memset(byte), ctx.empty(s, np.int64).memset(byte)


@gpu
def test_device_entry_zeroes_its_outputs_and_takes_row_slices(ctx):
    n, s = 300, 70
    ps, mid, sign = _table(n, s, 400)
    d_ps, d_mid, d_sign = ctx.to_device(ps), ctx.to_device(mid), ctx.to_device(sign)
    d_scores, d_counts = _filled(ctx, s)
    want = ctx.similarity(ps, mid, sign)
    for _ in range(2):                                  # the second call must not add to the first one's sums
        ctx.similarity_dev(d_ps, d_mid, d_sign, d_scores, d_counts)
        assert np.array_equal(d_scores.to_host(), want[0]) and np.array_equal(d_counts.to_host(), want[1])
    assert np.array_equal(want[0], R.similarity_counts(ps, mid, sign)[0])
    for start, length in SLICES(n):
        rows = slice(start, start + length)
        d_scores.memset(0x5A), d_counts.memset(0x5A)
        ctx.similarity_dev(d_ps.offset(start * s, (length, s)), d_mid.offset(start, length), d_sign.offset(start, length),
                           d_scores, d_counts)
        want = ctx.similarity(ps[rows], mid[rows], sign[rows])
        assert np.array_equal(d_scores.to_host(), want[0]) and np.array_equal(d_counts.to_host(), want[1]), (start, length)
        ref = R.similarity_counts(ps[rows], mid[rows], sign[rows])
        assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1]), (start, length)


@gpu
def test_device_entry_without_rows_or_columns(ctx):
    d_ps, d_mid, d_sign = ctx.to_device(np.ones((4, 5))), ctx.to_device(np.zeros(4)), ctx.to_device(np.ones(4, np.int8))
    d_scores, d_counts = _filled(ctx, 5)
    call = ctx.lib.sdice_similarity_dev
    assert call(ctx.h, 0, 5, d_ps.ptr, d_mid.ptr, d_sign.ptr, d_scores.ptr, d_counts.ptr) == 0      # n = 0: zeros
    assert not d_scores.to_host().any() and not d_counts.to_host().any()
    assert call(ctx.h, 0, 5, None, None, None, d_scores.ptr, d_counts.ptr) == 0
    d_scores.memset(0x5A), d_counts.memset(0x5A)
    assert call(ctx.h, 4, 0, d_ps.ptr, d_mid.ptr, d_sign.ptr, d_scores.ptr, d_counts.ptr) == 0      # s = 0: nothing written
    assert call(ctx.h, 4, 0, d_ps.ptr, d_mid.ptr, d_sign.ptr, None, None) == 0
    filled = np.full(5, 0x5A5A5A5A5A5A5A5A, np.int64)
    assert np.array_equal(d_scores.to_host(), filled) and np.array_equal(d_counts.to_host(), filled)


# ------------------------------------------------------------------------------ refusals
REFUSALS = ["NULL ctx", "negative n", "negative s", "NULL scores", "NULL counts", "NULL ps", "NULL mid", "NULL sign"]


@gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_the_outputs_untouched(ctx, case, entry):
    n, s = 6, 5
    ps, mid, sign = _table(n, s, 500)
    filled = np.full(s, 0x5A5A5A5A5A5A5A5A, np.int64)
    if entry == "host":
        scores, counts = filled.copy(), filled.copy()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
        held = [ps, mid, sign, scores, counts]
    else:
        held = [ctx.to_device(ps), ctx.to_device(mid), ctx.to_device(sign), *_filled(ctx, s)]
        ptr = lambda a: a.ptr                            # noqa: E731
    args = [ctx.h, n, s] + [ptr(a) for a in held]
    where = {"NULL ctx": 0, "NULL ps": 3, "NULL mid": 4, "NULL sign": 5, "NULL scores": 6, "NULL counts": 7}
    if case == "negative n":
        args[1] = -1
    elif case == "negative s":
        args[2] = -1
    else:
        args[where[case]] = None
    symbol = "sdice_similarity" + ("_dev" if entry == "dev" else "")
    assert getattr(ctx.lib, symbol)(*args) == ERR_ARG, case
    reason = b"ctx is NULL" if case == "NULL ctx" else b"negative size" if case.startswith("negative") else \
        b"NULL output" if case in ("NULL scores", "NULL counts") else b"NULL input"
    assert b"sdice_similarity" in ctx.lib.sdice_last_error() and reason in ctx.lib.sdice_last_error(), case
    after = held[3:] if entry == "host" else [a.to_host() for a in held[3:]]
    assert np.array_equal(after[0], filled) and np.array_equal(after[1], filled), case
    _check(ctx, ps, mid, sign, "the context still works")


# ------------------------------------------------------------------------------ the command
@gpu
@pytest.mark.parametrize("case", list(SF.SIMILARITY_CASES))
def test_command_writes_the_reference_report(ctx, golden_dir, tmp_path, case):
    """similarity.run_with on the real context reproduces what the reference wrote from the same inputs, the part before
    the exception included where it raised"""
    from splicedice_amd import similarity
    d = os.path.join(golden_dir, "similarity_edge")
    rec = json.load(open(os.path.join(d, f"expected_{case}.json")))
    out = tmp_path / "report.tsv"
    args = argparse.Namespace(comparison=os.path.join(d, rec["comparison"]), allps=os.path.join(d, rec["allps"]),
                              manifest=rec["manifest"] and os.path.join(d, rec["manifest"]), output=str(out))
    if rec["raises"]:
        assert rec["raises"] == "ZeroDivisionError"
        with pytest.raises(ZeroDivisionError):
            similarity.run_with(args, ctx=ctx)
    else:
        similarity.run_with(args, ctx=ctx)
    assert out.read_text() == open(os.path.join(d, f"expected_{case}.tsv")).read()
