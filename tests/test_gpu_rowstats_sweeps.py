"""rowstats_kernel (K9, csrc/rowstats.hip) against numpy row by row (tests/scoring_referee.py): more rows than one pass of
the capped grid takes, column lists in any order and with repeats, edge rows (signed zeros, inf, overflow, cancellation,
subnormals), the device entry point, the refusals, and the command on the matrices whose lines the reference printed
(tests/golden/outliers_edge).

Every comparison of a mean or a std is scoring_referee.same_bits, for float32 and float64: NaN where numpy has NaN, numpy's
bit pattern everywhere else, so the sign of a zero counts.  The CPU checks (not gpu-marked) show that the column-order
fixtures have sums that depend on the order.
"""
import argparse
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import scoring_referee as R  # noqa: E402
from rank_support import PLACEMENTS, _kept_positions  # noqa: E402

gpu = pytest.mark.gpu
ERR_ARG = -1
DTYPES = [np.float32, np.float64]
SLICES = lambda n: ((0, 1), (7, 64), (100, 180), (n - 3, 3))     # noqa: E731  (start, length) of the row slices
OUTSIDE = [np.nan, 1e30, -7.0]                                  # what the columns outside idx hold


def assert_rowstats(got, want, label, where=None):
    for name, g, w in zip(("mean", "std", "n_nan"), got, want):
        bad = np.flatnonzero(~R.same_bits(g, w))
        assert bad.size == 0, (label, name, f"{bad.size} rows differ", bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist(),
                               None if where is None else where(bad[:6]))


# ------------------------------------------------------------------------------ fixtures
def edge_rows(k, dtype, rng):
    """-> [(name, the k selected values)]; a kind that needs two values keeps what fits at k = 1"""
    big, tiny = np.finfo(dtype).max, np.finfo(dtype).smallest_subnormal
    at = lambda fill, put: np.r_[np.asarray(put, np.float64), np.full(k, fill, np.float64)][:k]     # noqa: E731
    mid = lambda row, v: (row.__setitem__(k // 2, v), row)[1]                                      # noqa: E731
    noise = rng.random(k)
    return [("all -0.0", np.full(k, -0.0)),
            ("-0.0 and one NaN", mid(np.full(k, -0.0), np.nan)),
            ("+0.0 and -0.0", np.where(np.arange(k) % 2 == 0, 0.0, -0.0)),
            ("-0.0 and +0.0", np.where(np.arange(k) % 3 == 0, -0.0, 0.0)),
            ("all NaN", np.full(k, np.nan)),
            ("one value", mid(np.full(k, np.nan), 0.3)),
            ("+inf", mid(noise.copy(), np.inf)),
            ("-inf", mid(noise.copy(), -np.inf)),
            ("+inf and -inf", at(0.5, [np.inf, -np.inf])),
            ("max twice", at(0.25, [big, big])),
            ("-max twice", at(0.25, [-big, 1.0, -big])),
            ("cancellation", np.resize([1e20, 1e20, -1e20, 3.0], k)),
            ("subnormals", tiny * rng.integers(1, 50, k)),
            ("subnormals and zeros", tiny * rng.integers(-2, 3, k)),
            ("constant 0.1", np.full(k, 0.1))]


def table(k, s, dtype, seed):
    """-> (palette of rows [m, s] of dtype, idx int32 [k] ascending, the name of every palette row): rows with
    0, 1, k/2, k-1 and k NaNs among the selected columns at four placements, 3-decimal and continuous values, and the
    edge rows; the columns outside idx hold values that would show if they were read"""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(s, k, replace=False)).astype(np.int32)
    rows, names = [], []
    for n_nan in sorted({0, 1, k // 2, k - 1, k}):
        for how in PLACEMENTS:
            for flavour in ("3 decimals", "continuous"):
                v = np.round(rng.random(k), 3) if flavour == "3 decimals" else rng.random(k) ** 2
                v[_kept_positions(k, n_nan, how, rng)] = np.nan           # (here the kept positions are the NaNs)
                rows.append(v)
                names.append(f"{n_nan} NaN {how} {flavour}")
    for name, v in edge_rows(k, dtype, rng):
        rows.append(v)
        names.append(name)
    data = rng.choice(OUTSIDE, size=(len(rows), s))
    data[:, idx] = np.array(rows)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(data.astype(dtype)), idx, names


def order_case(k, dtype, kind, seed=1):
    """100 rows of random() ** 2 -> (data [100, s], idx int32 [k]) with idx a random permutation of k columns, the same
    columns descending, or (k = 40) 40 draws with replacement from 25 columns"""
    rng = np.random.default_rng(seed * 1000 + k)
    s = k + 7
    data = (rng.random((100, s)) ** 2).astype(dtype)
    chosen = rng.choice(s, k, replace=False)
    if kind == "permuted":
        idx = chosen
    elif kind == "reversed":
        idx = np.sort(chosen)[::-1]
    else:
        idx = rng.choice(rng.choice(s, 25, replace=False), k, replace=True)
        assert np.unique(idx).size < k
    assert np.any(np.diff(idx) < 0)
    return data, np.ascontiguousarray(idx, np.int32)


ORDER_CASES = [(k, kind) for k in (9, 40, 130, 1024) for kind in ("permuted", "reversed")] + [(40, "repeated")]


# ------------------------------------------------------------------------------ CPU checks of the fixtures
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,kind", ORDER_CASES)
def test_order_cases_tell_the_column_order(k, kind, dtype):
    """at least 10 % of the rows have a mean that is another number when the same columns are summed in ascending order"""
    data, idx = order_case(k, dtype, kind)
    mean, _, _ = R.rowstats_rows(data, idx)
    mean_sorted, _, _ = R.rowstats_rows(data, np.sort(idx))
    share = float(np.mean(mean != mean_sorted))
    print(f"k {k} {kind} {np.dtype(dtype).name}: mean differs on {share:.0%} of the rows")
    assert share >= 0.10, (k, kind, share)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rows_hold_what_their_names_say(dtype):
    for k in (1, 7, 8, 9, 129, 1024):
        data, idx, names = table(k, k + 37, dtype, 7)
        assert len(set(names)) == len(names)
        mean, std, n_nan = R.rowstats_rows(data, idx)
        row = {name: i for i, name in enumerate(names)}
        assert mean[row["all -0.0"]] == 0 and not np.signbit(mean[row["all -0.0"]])        # np.sum starts from +0
        assert np.isnan(mean[row["all NaN"]]) and np.isnan(std[row["all NaN"]]) and n_nan[row["all NaN"]] == k
        assert mean[row["one value"]] == dtype(0.3) and std[row["one value"]] == 0 and n_nan[row["one value"]] == k - 1
        assert mean[row["+inf"]] == np.inf and np.isnan(std[row["+inf"]]) and mean[row["-inf"]] == -np.inf
        if k >= 2:
            assert np.isnan(mean[row["+inf and -inf"]]) and mean[row["max twice"]] == np.inf
        if k >= 4 and dtype == np.float32:
            assert std[row["cancellation"]] == np.inf
        assert mean[row["subnormals"]] > 0 and std[row["subnormals"]] == 0                 # d * d underflows


# ------------------------------------------------------------------------------ rows past the grid cap
CAP_SHAPES = [(2, 5, 7, 12), (2, 5, 130, 140), (1, 3, 1024, 1030)]      # (passes, extra rows, K, s)


def test_cap_shapes_on_the_nominal_part():
    """(not gpu-marked) on 256 compute units: more rows than the 8192 one pass takes, and the largest table is 34 MB"""
    per_pass = 32 * RS.NOMINAL_CUS
    assert all(passes * per_pass + extra > per_pass for passes, extra, _, _ in CAP_SHAPES)
    assert max((passes * per_pass + extra) * s * 8 for passes, extra, _, s in CAP_SHAPES) < 70e6


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CAP_SHAPES)
def test_rows_past_the_grid_cap(ctx, shape, dtype):
    """(passes, extra rows, K, s): the launch is capped at 8 blocks of 4 waves per compute unit, one row per wave and pass"""
    passes, extra, k, s = shape
    per_pass = 32 * ctx.device_info()["compute_units"]
    n = passes * per_pass + extra
    assert n > per_pass
    palette, idx, names = table(k, s, dtype, 31 * k + passes)
    pick = RS.palette_index(n, len(palette))
    assert 40 <= len(palette) <= 70 and np.unique(pick[per_pass if passes > 1 else 0:]).size == len(palette)
    data = np.ascontiguousarray(palette[pick])
    want = [v[pick] for v in R.rowstats_rows(palette, idx)]
    assert_rowstats(ctx.rowstats(data, idx), want, shape, lambda rows: [names[pick[r]] for r in rows])


# ------------------------------------------------------------------------------ idx in any order
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,kind", ORDER_CASES)
def test_columns_in_any_order(ctx, k, kind, dtype):
    data, idx = order_case(k, dtype, kind)
    assert_rowstats(ctx.rowstats(data, idx), R.rowstats_rows(data, idx), (k, kind))


# ------------------------------------------------------------------------------ edge rows
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 7, 8, 9, 129, 1024])
def test_edge_rows(ctx, k, dtype):
    data, idx, names = table(k, k + 37, dtype, 7)
    assert_rowstats(ctx.rowstats(data, idx), R.rowstats_rows(data, idx), k, lambda rows: [names[r] for r in rows])


# ------------------------------------------------------------------------------ device entry
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_entry_and_row_slices(ctx, dtype):
    k, s = 40, 50
    palette, idx, _ = table(k, s, dtype, 11)
    n = 300
    data = np.ascontiguousarray(palette[RS.palette_index(n, len(palette))])
    want = ctx.rowstats(data, idx)
    assert_rowstats(want, R.rowstats_rows(data, idx), "host call")
    d_data, d_idx = ctx.to_device(data), ctx.to_device(idx)
    outs = [ctx.empty(n, dtype), ctx.empty(n, dtype), ctx.empty(n, np.int32)]
    for d in outs:
        d.memset(0x5A)
    ctx.rowstats_dev(d_data, d_idx, *outs)
    assert_rowstats([d.to_host() for d in outs], want, "device call")
    for start, length in SLICES(n):
        for d in outs:
            d.memset(0x5A)
        ctx.rowstats_dev(d_data.offset(start * s, (length, s)), d_idx, *[d.offset(0, length) for d in outs])
        got = [d.to_host() for d in outs]
        assert_rowstats([g[:length] for g in got], [w[start:start + length] for w in want], (start, length))
        for g in got:                                    # nothing past the slice's rows is written
            assert (RS.bits(g[length:]) == (0x5A5A5A5A5A5A5A5A & (2 ** (8 * g.itemsize) - 1))).all(), (start, length)
    for d in outs:
        d.memset(0x5A)
    code = 0 if dtype == np.float32 else 1
    assert ctx.lib.sdice_rowstats_dev(ctx.h, 0, s, d_data.ptr, code, d_idx.ptr, k, *[d.ptr for d in outs]) == 0
    assert ctx.lib.sdice_rowstats_dev(ctx.h, 0, s, None, code, None, k, None, None, None) == 0
    for d in outs:
        assert (RS.bits(d.to_host()) == (0x5A5A5A5A5A5A5A5A & (2 ** (8 * d.dtype.itemsize) - 1))).all()


# ------------------------------------------------------------------------------ refusals
REFUSALS = ["NULL ctx", "dtype 2", "dtype -1", "k = 0", "k = 1025", "negative n", "negative s", "negative k",
            "NULL data", "NULL idx", "NULL mean", "NULL std", "NULL n_nan"]
HOST_ONLY = ["negative column", "column = s"]


@gpu
@pytest.mark.parametrize("entry,case", [(e, c) for e in ("host", "dev") for c in REFUSALS] + [("host", c) for c in HOST_ONLY])
def test_refusals_leave_the_outputs_untouched(ctx, entry, case):
    n, s, k = 6, 9, 4
    rng = np.random.default_rng(600)
    data = rng.random((n, s)).astype(np.float32)
    idx = np.array([1, 3, 4, 8], np.int32)
    if case == "k = 1025":
        idx, k = np.zeros(1025, np.int32), 1025
    elif case == "negative column":
        idx[2] = -1
    elif case == "column = s":
        idx[3] = s
    fill32, filli = np.full(n, 0x5A5A5A5A, np.uint32).view(np.float32), np.full(n, 0x5A5A5A5A, np.int32)
    if entry == "host":
        held = [data, idx, fill32.copy(), fill32.copy(), filli.copy()]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    else:
        held = [ctx.to_device(data), ctx.to_device(idx)] + [ctx.empty(n, t).memset(0x5A) for t in (np.float32, np.float32, np.int32)]
        ptr = lambda a: a.ptr                            # noqa: E731
    d, i, m, sd, nn = (ptr(a) for a in held)
    args = [ctx.h, n, s, d, 0, i, k, m, sd, nn]
    change = {"NULL ctx": (0, None), "dtype 2": (4, 2), "dtype -1": (4, -1), "k = 0": (6, 0), "negative n": (1, -1),
              "negative s": (2, -1), "negative k": (6, -1), "NULL data": (3, None), "NULL idx": (5, None), "NULL mean": (7, None),
              "NULL std": (8, None), "NULL n_nan": (9, None)}
    if case in change:
        args[change[case][0]] = change[case][1]
    symbol = "sdice_rowstats" + ("_dev" if entry == "dev" else "")
    assert getattr(ctx.lib, symbol)(*args) == ERR_ARG, case
    assert b"sdice_rowstats" in ctx.lib.sdice_last_error(), case
    after = held[2:] if entry == "host" else [a.to_host() for a in held[2:]]
    for a in after:
        assert (RS.bits(a) == 0x5A5A5A5A).all(), case
    good = np.array([1, 3, 4, 8], np.int32)
    assert_rowstats(ctx.rowstats(data, good), R.rowstats_rows(data, good), "the context still works")


# ------------------------------------------------------------------------------ the command
@gpu
@pytest.mark.parametrize("cutoff", [0, 2, 3])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_command_prints_the_reference_lines(ctx, golden_dir, capsys, tag, cutoff):
    """find_outliers.run_with on the real context prints what the reference printed from the same edge matrix"""
    from splicedice_amd import find_outliers
    d = os.path.join(golden_dir, "outliers_edge")
    args = argparse.Namespace(psiSPLICEDICE=os.path.join(d, f"matrix_{tag}.npz"), manifest=os.path.join(d, "samples.tsv"),
                              nullMan=os.path.join(d, "null.tsv"), outlierCutoff=cutoff, dpsiThrsh=0.1)
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        find_outliers.run_with(args, ctx=ctx)
    got, want = capsys.readouterr().out.splitlines(), open(os.path.join(d, f"expected_{tag}_cutoff{cutoff}.txt")).read().splitlines()
    if got != want:                                      # (the first line that differs; pytest's own diff takes minutes)
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((f"line {first} of {len(got)} / {len(want)}", got[first:first + 1], want[first:first + 1]))
