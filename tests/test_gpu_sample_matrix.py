"""sdice_sample_gram and the `sample_matrix` command on the GPU: edge values and every refusal of an off-grid value, the
argument errors, the host and the device entry against each other and called twice into the same buffers, and the command
byte for byte -- the four integer matrices compared for equality, whole, with tests/sample_matrix_referee.py."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_matrix_referee as SM  # noqa: E402

gpu = pytest.mark.gpu

NAMES = ("shared", "sum1", "sum2", "prod")
SDICE_ERR_ARG = -1
SENTINEL = -0x5A5A5A5A5A5A5A5B


def check(got, ps, cols, what=""):
    """every one of the four matrices equals the referee's, entry for entry"""
    want = SM.gram(ps, cols)
    for name in NAMES:
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, (what, name)
        if not np.array_equal(got[name], want[name]):
            bad = np.argwhere(got[name] != want[name])
            a, b = bad[0]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} of {want[name].size} entries, first [{a}, {b}]: "
                                 f"{got[name][a, b]} != {want[name][a, b]}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_call(ctx, ps, cols, m=None, outs=None, n=None, s=None):
    """sdice_sample_gram through ctypes with sentinel-filled outputs -> (return code, message, outputs)"""
    ps = np.ascontiguousarray(ps, dtype=np.float32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    m = cols.size if m is None else m
    side = max(cols.size, min(m, 8))
    if outs is None:
        outs = [np.full((side, side), SENTINEL, np.int64) for _ in NAMES]
    rc = ctx.lib.sdice_sample_gram(ctx.h, ps.shape[0] if n is None else n, ps.shape[1] if s is None else s, _p(ps), _p(cols),
                                   m, *[_p(o) for o in outs])
    return rc, ctx.lib.sdice_last_error().decode(), outs


def untouched(outs):
    return all(o is None or np.all(o == SENTINEL) for o in outs)


@gpu
def test_edge_values(ctx):
    """the six edge keys, -0.0 and NaNs of several payloads, in every pairing"""
    vals = [SM.GRID[k] for k in (0, 1, 499, 500, 999, 1000)] + [np.float32(-0.0)]
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    assert np.all(np.isnan(nans))
    pool = np.concatenate([np.array(vals, dtype=np.float32), nans])
    rng = np.random.default_rng(61)
    ps = pool[rng.integers(0, pool.size, size=(211, 13))]
    ps[:pool.size, 0] = pool                        # every value against every value in columns 0 and 1
    ps[:pool.size, 1] = pool[::-1]
    assert np.signbit(ps).any() and np.isnan(ps).any()
    cols = np.array([1, 0, 12, 5, 7, 3, 9], dtype=np.int32)
    check(ctx.sample_gram(ps, cols), ps, cols, "edge values")


BAD = {"0.0005": np.float32(0.0005), "1.001": np.float32(1.001), "-0.001": np.float32(-0.001), "+inf": np.float32(np.inf),
       "-inf": np.float32(-np.inf), "nextafter(0.1)": np.nextafter(np.float32(0.1), np.float32(1))}


@gpu
@pytest.mark.parametrize("where", ["first row, first selected", "last row, last selected"])
@pytest.mark.parametrize("bad", list(BAD))
def test_off_grid_values_are_refused(ctx, bad, where):
    rng = np.random.default_rng(67)
    n, s = 300, 11
    ps = SM.random_table(rng, n, s)
    cols = np.array([4, 9, 0, 7, 2], dtype=np.int32)
    r, c = (0, int(cols[0])) if where.startswith("first") else (n - 1, int(cols[-1]))
    ps[r, c] = BAD[bad]
    rc, msg, outs = raw_call(ctx, ps, cols)
    assert rc == SDICE_ERR_ARG and f"row {r}," in msg and f"column {c} " in msg, (rc, msg)
    assert untouched(outs)
    with pytest.raises(Exception, match=f"row {r}, column {c} "):
        ctx.sample_gram(ps, cols)
    # the same value where no selected column is: never looked at
    ps[r, c] = SM.GRID[250]
    for free in (1, 3, 5, 6, 8, 10):
        ps[r, free] = BAD[bad]
    check(ctx.sample_gram(ps, cols), np.where(np.isin(np.arange(s), cols), ps, np.float32(0.5)), cols, "unselected")


@gpu
def test_first_bad_value_is_named(ctx):
    """several off-grid cells: the message names the first in (row, position in cols) order"""
    rng = np.random.default_rng(68)
    ps = SM.random_table(rng, 500, 9)
    cols = np.array([8, 1, 6, 3], dtype=np.int32)
    ps[400, 8] = ps[77, 3] = ps[77, 6] = ps[300, 1] = np.float32(0.12345)
    rc, msg, outs = raw_call(ctx, ps, cols)
    assert rc == SDICE_ERR_ARG and "row 77, column 6 " in msg and untouched(outs), msg


@gpu
def test_argument_errors(ctx):
    rng = np.random.default_rng(71)
    ps = SM.random_table(rng, 6, 12)
    good = np.array([3, 0, 11, 5], dtype=np.int32)
    wide = SM.random_table(rng, 1, 4100)
    cases = {
        "m = 1": raw_call(ctx, ps, good[:1]),
        "m = 0": raw_call(ctx, ps, good[:0]),
        "m = 4097": raw_call(ctx, wide, np.arange(4097)),
        "m > s": raw_call(ctx, ps[:, :3], good, s=3),
        "a column equal to s": raw_call(ctx, ps, np.array([3, 12, 5])),
        "a negative column": raw_call(ctx, ps, np.array([3, -1, 5])),
        "a column listed twice": raw_call(ctx, ps, np.array([3, 0, 5, 3])),
    }
    for k in range(4):
        outs = [np.full((4, 4), SENTINEL, np.int64) for _ in NAMES]
        outs[k] = None
        cases[f"NULL output {k}"] = raw_call(ctx, ps, good, outs=outs)
    for what, (rc, msg, outs) in cases.items():
        assert rc == SDICE_ERR_ARG and msg and untouched(outs), (what, rc, msg)
    assert "4097 columns listed" in cases["m = 4097"][1] and "out of range" in cases["a column equal to s"][1]
    assert "once" in cases["a column listed twice"][1]
    # the _dev entry: sizes and pointers (the column list is on the device)
    d_ps, d_cols = ctx.to_device(ps, np.float32), ctx.to_device(good, np.int32)
    d_out = {k: ctx.to_device(np.full((4, 4), SENTINEL, np.int64)) for k in NAMES}
    lib = ctx.lib
    ptrs = [d_out[k].ptr for k in NAMES]
    assert lib.sdice_sample_gram_dev(ctx.h, 6, 12, d_ps.ptr, d_cols.ptr, 1, *ptrs) == SDICE_ERR_ARG
    assert lib.sdice_sample_gram_dev(ctx.h, 6, 12, d_ps.ptr, d_cols.ptr, 4097, *ptrs) == SDICE_ERR_ARG
    assert lib.sdice_sample_gram_dev(ctx.h, 6, 3, d_ps.ptr, d_cols.ptr, 4, *ptrs) == SDICE_ERR_ARG
    assert lib.sdice_sample_gram_dev(ctx.h, 6, 12, d_ps.ptr, d_cols.ptr, 4, ptrs[0], None, ptrs[2], ptrs[3]) == SDICE_ERR_ARG
    # a column index past the table on the device: met by the pre-pass, refused before any sum
    d_badcols = ctx.to_device(np.array([3, 0, 12, 5], dtype=np.int32))
    assert lib.sdice_sample_gram_dev(ctx.h, 6, 12, d_ps.ptr, d_badcols.ptr, 4, *ptrs) == SDICE_ERR_ARG
    assert "cols[2]" in lib.sdice_last_error().decode()
    ctx.sync()
    assert all(np.all(d_out[k].to_host() == SENTINEL) for k in NAMES)
    for a in (d_ps, d_cols, d_badcols, *d_out.values()):
        a.free()


@gpu
def test_no_rows_gives_zeros(ctx):
    rc, msg, outs = raw_call(ctx, np.zeros((0, 7), np.float32), np.array([2, 6, 0]))
    assert rc == 0 and all(np.all(o == 0) for o in outs), (rc, msg)
    d_ps, d_cols = ctx.empty((0, 7), np.float32), ctx.to_device(np.array([2, 6, 0], dtype=np.int32))
    d_out = {k: ctx.to_device(np.full((3, 3), SENTINEL, np.int64)) for k in NAMES}
    ctx.sample_gram_dev(d_ps, d_cols, d_out)
    ctx.sync()
    assert all(np.all(d_out[k].to_host() == 0) for k in NAMES)
    for a in (d_ps, d_cols, *d_out.values()):
        a.free()


@gpu
def test_host_and_device_entry_agree_and_outputs_are_rezeroed(ctx):
    rng = np.random.default_rng(73)
    n, s, m = 700, 90, 75
    ps = SM.random_table(rng, n, s)
    cols = rng.permutation(s)[:m].astype(np.int32)
    host = ctx.sample_gram(ps, cols)
    check(host, ps, cols, "host entry")
    d_ps, d_cols = ctx.to_device(ps, np.float32), ctx.to_device(cols, np.int32)
    d_out = {k: ctx.to_device(np.full((m, m), SENTINEL, np.int64)) for k in NAMES}
    for call in range(2):                           # the second call into the buffers that hold the first one's sums
        ctx.sample_gram_dev(d_ps, d_cols, d_out)
        ctx.sync()
        got = {k: d_out[k].to_host() for k in NAMES}
        for k in NAMES:
            assert np.array_equal(got[k], host[k]), (call, k)
    # another table into the same buffers: nothing of the first is left
    ps2 = SM.random_table(rng, n, s, nan_frac=0.8)
    d_ps.upload(ps2)
    ctx.sample_gram_dev(d_ps, d_cols, d_out)
    ctx.sync()
    check({k: d_out[k].to_host() for k in NAMES}, ps2, cols, "second table")
    for a in (d_ps, d_cols, *d_out.values()):
        a.free()


# ---------------------------------------------------------------- the command
def _write_table(path, names, ps):
    with open(path, "w") as f:
        f.write("cluster\t" + "\t".join(names) + "\n")
        for i, row in enumerate(ps):
            f.write(f"chr7:{1000 + 13 * i}-{5000 + 17 * i}:-\t" + "\t".join("nan" if np.isnan(v) else "%.3f" % v for v in row) + "\n")


def _square(names, data, fmt):
    return "sample\t" + "\t".join(names) + "\n" + "".join(
        name + "\t" + "\t".join(fmt(v) for v in row) + "\n" for name, row in zip(names, data))


@gpu
@pytest.mark.parametrize("with_list", [True, False])
def test_command_byte_for_byte(ctx, tmp_path, with_list):
    from splicedice_amd import sample_matrix
    from splicedice_amd.engine import sample_matrix_finish
    rng = np.random.default_rng(79)
    names = [f"lib{j:02d}" for j in range(9)]
    ps = SM.random_table(rng, 40, 9, nan_frac=0.35)
    ps[:, 3] = np.float32(0.5)                      # a constant sample: nan correlations, distances defined
    ps[4:, 8] = np.nan                              # shares at most 4 junctions: below --minShared 5
    table = str(tmp_path / "t_allPS.tsv")
    _write_table(table, names, ps)
    if with_list:
        order = [7, 2, 3, 0, 8, 5]
        listing = tmp_path / "samples.txt"
        listing.write_text("".join(f"{names[j]}\tbatch{j % 2}\n\n" for j in order))
        args = argparse.Namespace(psiSPLICEDICE=table, samples=str(listing), minShared=5, outputPrefix=str(tmp_path / "o"))
    else:
        order = list(range(9))
        args = argparse.Namespace(psiSPLICEDICE=table, samples="", minShared=3, outputPrefix=str(tmp_path / "o"))
    sample_matrix.run_with(args, ctx=ctx)
    g = SM.gram(ps, order)
    corr, rmsd = sample_matrix_finish(g["shared"], g["sum1"], g["sum2"], g["prod"], args.minShared)
    chosen = [names[j] for j in order]
    assert np.isnan(corr).any() and (~np.isnan(corr)).any()
    if with_list:
        assert np.all(np.isnan(rmsd[4, :4])) and not np.isnan(rmsd[0, 1])
    want = {"_sampleCorrelation.tsv": _square(chosen, corr, str), "_sampleDistance.tsv": _square(chosen, rmsd, str),
            "_sampleShared.tsv": _square(chosen, g["shared"], lambda v: "%.0f" % v)}
    for suffix, text in want.items():
        assert open(str(tmp_path / "o") + suffix).read() == text, suffix


@gpu
def test_command_off_grid_cell_exits_1(ctx, tmp_path, capsys):
    from splicedice_amd import sample_matrix
    rng = np.random.default_rng(83)
    names = [f"lib{j}" for j in range(5)]
    ps = SM.random_table(rng, 12, 5)
    table = str(tmp_path / "t_allPS.tsv")
    _write_table(table, names, ps)
    text = open(table).read().splitlines()
    cells = text[7].split("\t")
    cells[3] = "0.1234"                             # row 6, column 2
    text[7] = "\t".join(cells)
    open(table, "w").write("\n".join(text) + "\n")
    args = argparse.Namespace(psiSPLICEDICE=table, samples="", minShared=3, outputPrefix=str(tmp_path / "o"))
    with pytest.raises(SystemExit) as e:
        sample_matrix.run_with(args, ctx=ctx)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("sample_matrix: ") and "row 6, column 2 " in err and err.count("\n") == 1, err
    assert not [x for x in os.listdir(tmp_path) if x.startswith("o_")]
