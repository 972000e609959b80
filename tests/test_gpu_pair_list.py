"""GPU: the Fisher and chi2 pair kernels over a caller's LIST of sample pairs (sdice_fisher_pair_list / sdice_chi2_pair_list
and their _dev forms), and everything above them: engine, device pipeline of the sub-command, sharded pipeline.

The pair kernel walks a packed pair table q -> (i, j); with a list that table is the caller's.  Window (two registers of
64 entries), ring (512 slots) and pmf blocks (256 pairs) are indexed by q alone, so the lists here hit their ends:
m = 1, 63, 64, 65, 255, 256, 257, 512, 513, the full natural list, a random subset in random order, every pair reversed,
a list with repeats -- at s = 3, 24, 65 and 200, every p-value checked.

Reference and tolerances are those of tests/test_gpu_pair_sweeps.py, whose palette rows are reused: scipy once per
distinct 2x2 table ((j, i) is the table with its columns swapped, looked up as the ORDERED palette pair), 1e-9 relative,
1e-7 for totals above 5e4.  Command-line tables against the reference-written goldens: 1e-6 relative, identical
structure and row names (tests/test_gpu_cli.py).
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle_np as O  # noqa: E402
from pair_fixtures import MIX_WEIGHTS, SWEEP, TABLE_MAX_T, PaletteRef, _check_chi2, _check_fisher  # noqa: E402
from splicedice_amd.engine import SdiceError  # noqa: E402

gpu = pytest.mark.gpu
CLI_RTOL = 1e-6
EDGE_M = (1, 63, 64, 65, 255, 256, 257, 512, 513)


def natural(s):
    iu, ju = np.triu_indices(s, 1)
    return np.stack([iu, ju], axis=1).astype(np.int32)


def random_pairs(s, m, rng):
    """m ordered pairs (i, j), i != j, both orientations, repeats as they fall (at s = 3 there are six to draw from)"""
    i = rng.integers(0, s, m)
    j = (i + rng.integers(1, s, m)) % s
    return np.stack([i, j], axis=1).astype(np.int32)


def edge_lists(s, seed):
    rng = np.random.default_rng(seed)
    nat = natural(s)
    lists = {f"m={m}": random_pairs(s, m, rng) for m in EDGE_M}
    lists["natural"] = nat
    lists["reversed"] = nat[:, ::-1]
    k = max(1, len(nat) * 2 // 3)
    sub = nat[rng.permutation(len(nat))[:k]]
    flip = rng.random(k) < 0.5
    sub[flip] = sub[flip][:, ::-1]
    lists["subset"] = sub
    few = random_pairs(s, 5, rng)
    lists["repeats"] = few[rng.integers(0, 5, 300)]
    return lists


def list_ids(ref, pid, pi, pairs):
    """table id of every listed pair of every row: the ORDERED palette pair (entry of sample i, entry of sample j)"""
    return ref.ids[pid[:, None], pi[:, pairs[:, 0]], pi[:, pairs[:, 1]]]


def test_list_ids_are_the_per_pair_oracle_on_the_swapped_table():
    """(not gpu) the list scatter against scipy per listed table, reversed pairs included"""
    from scipy.stats import fisher_exact
    ref = PaletteRef(["zeros", "ties", "small"])
    incl, excl, pid, pi = ref.rows(7, seed=11)
    pairs = edge_lists(7, 1)["subset"]
    assert (pairs[:, 0] > pairs[:, 1]).any() and (pairs[:, 0] < pairs[:, 1]).any()
    want = ref.fisher()[0][list_ids(ref, pid, pi, pairs)]
    for r in range(incl.shape[0]):
        for q, (i, j) in enumerate(pairs):
            assert want[r, q] == fisher_exact([[incl[r, i], incl[r, j]], [excl[r, i], excl[r, j]]])[1]


# ------------------------------------------------------------------------------ kernels: every edge of the hand-out
@gpu
@pytest.mark.parametrize("s", [3, 24, 65, 200])
def test_pair_list_edges(ctx, s):
    """Fisher and chi2 on every list of edge_lists; the natural list bit for bit what the all-pairs call gives; and the
    count of values that differ bitwise from the matching all-pairs column for the other lists (printed, not asserted:
    lanes influence each other through power-of-two rescaling only, but the bar is the tolerance)"""
    ref = PaletteRef(SWEEP)
    incl, excl, pid, pi = ref.rows(s, reps=2, seed=21, weights={"mix": MIX_WEIGHTS})
    full_f = ctx.fisher_pairs(incl, excl)
    full_c, full_bad = ctx.chi2_pairs(incl, excl)
    col_of = {(int(i), int(j)): q for q, (i, j) in enumerate(natural(s))}
    n_same = n_diff = 0
    for name, pairs in edge_lists(s, 100 + s).items():
        what = f"s={s} list {name}"
        ids = list_ids(ref, pid, pi, pairs)
        got = ctx.fisher_pairs(incl, excl, pairs=pairs)
        assert got.shape == (incl.shape[0], len(pairs)), what
        _check_fisher(ref, got, ids, "fisher " + what)
        p, n_bad = ctx.chi2_pairs(incl, excl, pairs=pairs)
        _check_chi2(ref, p, n_bad, ids, "chi2 " + what)
        if name == "natural":
            assert np.array_equal(got.view(np.uint64), full_f.view(np.uint64)), what
            assert np.array_equal(p.view(np.uint64), full_c.view(np.uint64)) and n_bad == full_bad, what
        else:
            fwd = np.flatnonzero(pairs[:, 0] < pairs[:, 1])
            cols = [col_of[(int(i), int(j))] for i, j in pairs[fwd]]
            d = int((got[:, fwd].view(np.uint64) != full_f[:, cols].view(np.uint64)).sum())
            n_diff += d
            n_same += got[:, fwd].size - d
            assert np.array_equal(p[:, fwd].view(np.uint64), full_c[:, cols].view(np.uint64)), what     # (chi2: lanes are independent)
    print(f"pair-list sweep s={s}: {n_diff} of {n_same + n_diff} Fisher p-values differ bitwise from their all-pairs column")


@gpu
def test_pair_list_many_junctions_fill_every_slot(ctx):
    """20 000 junctions at s = 24 with a list of 257 pairs through the device entry points and a device-resident table:
    waves take junction after junction; the output starts as NaN (0xFF bytes) with one guard row behind it"""
    n, s, m = 20_000, 24, 257
    assert n > ctx.device_info()["compute_units"] * 32
    ref = PaletteRef(SWEEP)
    incl, excl, pid, pi = ref.rows(s, reps=-(-n // len(SWEEP)), seed=22, weights={"mix": MIX_WEIGHTS})
    perm = np.random.default_rng(22).permutation(len(pid))[:n]
    incl, excl, pid, pi = incl[perm], excl[perm], pid[perm], pi[perm]
    pairs = random_pairs(s, m, np.random.default_rng(23))
    ids = list_ids(ref, pid, pi, pairs)
    d_incl, d_excl, d_tab = ctx.to_device(incl), ctx.to_device(excl), ctx.pair_table(s, pairs)
    assert d_tab.shape == (m,) and np.array_equal(d_tab.to_host(), (pairs[:, 0].astype(np.uint32) << 16) | pairs[:, 1].astype(np.uint32))
    d_p = ctx.empty((n + 1, m), np.float64).memset(0xFF)
    for _ in range(2):                                           # (the table outlives a call)
        ctx.fisher_pairs_dev(d_incl, d_excl, d_p, pairs=d_tab)
    out = d_p.to_host()
    assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
    assert not np.isnan(out[:n]).any(), int(np.isnan(out[:n]).sum())
    _check_fisher(ref, out[:n], ids, "fisher list n=20000")
    d_p.memset(0xFF)
    d_bad = ctx.empty(1, np.int64).memset(0xFF)
    ctx.chi2_pairs_dev(d_incl, d_excl, d_p, d_bad, pairs=d_tab)
    out = d_p.to_host()
    assert (out[n].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard row written"
    n_bad = int(d_bad.to_host()[0])
    assert n_bad > 1000
    _check_chi2(ref, out[:n], n_bad, ids, "chi2 list n=20000")
    assert np.array_equal(np.isnan(out[:n]), np.isnan(ref.chi2()[0])[ids])


@gpu
def test_pair_list_table_max_boundary(ctx):
    """fisher.table_max = 256 with a list: totals of 256 leave the pair kernel as markers that the second kernel finishes,
    flagged rows beside unflagged ones"""
    ref = PaletteRef(["edge", "edge", "under", "edge", "under", "zeros"])
    incl, excl, pid, pi = ref.rows(200, reps=8, seed=24)
    pairs = random_pairs(200, 700, np.random.default_rng(25))
    ids = list_ids(ref, pid, pi, pairs)
    totals = ref.total[ids]
    assert (totals == TABLE_MAX_T).any(axis=1).sum() >= 24 and (totals.max(axis=1) < TABLE_MAX_T).sum() >= 16
    with ctx.params({"fisher.table_max": TABLE_MAX_T}):
        got = ctx.fisher_pairs(incl, excl, pairs=pairs)
    _check_fisher(ref, got, ids, f"fisher list table_max={TABLE_MAX_T}")
    _check_fisher(ref, ctx.fisher_pairs(incl, excl, pairs=pairs), ids, "fisher list table_max restored")


@gpu
@pytest.mark.parametrize("s", [24, 200])
def test_pair_list_launch_knob_corners(ctx, s):
    ref = PaletteRef(SWEEP)
    incl, excl, pid, pi = ref.rows(s, reps=1, seed=26, weights={"mix": MIX_WEIGHTS})
    pairs = random_pairs(s, 257, np.random.default_rng(27))
    ids = list_ids(ref, pid, pi, pairs)
    for unroll in (4, 24):
        for refill in (1, 64):
            with ctx.params({"fisher.unroll": unroll, "fisher.refill": refill}):
                got = ctx.fisher_pairs(incl, excl, pairs=pairs)
            _check_fisher(ref, got, ids, f"fisher list s={s} unroll={unroll} refill={refill}")


@gpu
def test_pair_list_arguments_are_checked(ctx):
    incl, excl = np.ones((2, 5), np.int32), np.ones((2, 5), np.int64)
    for bad, word in (([(0, 5)], "indices"), ([(1, 2), (-1, 2)], "indices"), ([(0, 1), (3, 3)], "itself")):
        for call in (ctx.fisher_pairs, ctx.chi2_pairs, lambda a, b, pairs: ctx.pair_table(5, pairs)):
            with pytest.raises(SdiceError, match=word):
                call(incl, excl, pairs=bad)
    with pytest.raises(ValueError):
        ctx.fisher_pairs(incl, excl, pairs=[])
    with pytest.raises(SdiceError, match="8192"):
        ctx.fisher_pairs(np.ones((1, 8193), np.int32), np.ones((1, 8193), np.int64), pairs=[(0, 1)])
    # the context is still usable, and a single reversed pair is the swapped table
    from scipy.stats import fisher_exact
    incl = np.array([[3, 40, 9]], np.int32)
    excl = np.array([[25, 4, 11]], np.int64)
    got = ctx.fisher_pairs(incl, excl, pairs=[(1, 0)])
    np.testing.assert_allclose(got, [[fisher_exact([[40, 3], [4, 25]])[1]]], rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------ the sub-command on the device pipeline
LISTED = [("p0", "p3"), ("p4", "p1"), ("p2", "p5")]          # the second pair reversed
MIRROR = ["p0_p3", "p1_p4", "p2_p5"]                         # the golden columns they equal


def _ns(d, out, mode="none", pairs=None, chi2=False, table="in_inclusionCounts.tsv", filt=None):
    return argparse.Namespace(inclusionSPLICEDICE=os.path.join(d, table) if not os.path.isabs(table) else table,
                              clusters=os.path.join(d, "in_allClusters.tsv"), chi2=chi2, multiple_test_correction=mode,
                              filter_list=filt, output=str(out), pairs=pairs)


def _quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*a, **k)
    return buf.getvalue()


def _read(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return rows[0], [r[0] for r in rows[1:]], np.array([[float(x) for x in r[1:]] for r in rows[1:]]).reshape(len(rows) - 1, -1)


def _pair_file(tmp_path, named):
    f = tmp_path / "pairs.txt"
    f.write_text("".join(f"{a}\t{b}\n" for a, b in named))
    return str(f)


def _assert_table(got_path, named, want_events, want):
    header, events, got = _read(got_path)
    assert header == ["clusterID"] + [f"{a}_{b}" for a, b in named]
    assert events == want_events and got.shape == want.shape
    ok = (got == want) | (np.abs(got - want) <= CLI_RTOL * np.abs(want))
    assert ok.all(), (int((~ok).sum()), float(np.nanmax(np.abs(got - want) / np.abs(want))))


def _golden_columns(path, cols):
    header, events, want = _read(path)
    return events, want[:, [header.index(c) - 1 for c in cols]]


@gpu
@pytest.mark.parametrize("mode", ["none", "pairwise", "all"])
def test_pairwise_cli_pair_list(ctx, golden_dir, tmp_path, mode, monkeypatch):
    """run_with(--pairs) on the device pipeline, streamed in row slabs of a few rows: the listed columns of the
    reference-written tables (the reversed pair against its mirror column); `all` = BH over the listed raw columns"""
    from splicedice_amd import pairwise
    monkeypatch.setattr(pairwise, "SLAB_BYTES", 512)
    d = os.path.join(golden_dir, "pairwise")
    out = tmp_path / "pw.tsv"
    text = _quiet(pairwise.run_with, _ns(d, out, mode, _pair_file(tmp_path, LISTED)), ctx=ctx)
    lines = text.splitlines()
    assert lines[lines.index("Analyzing pairs:") + 1] == "p0_p3,p4_p1,p2_p5"
    events, want = _golden_columns(os.path.join(d, "expected_pairwise.tsv" if mode == "pairwise" else "expected_none.tsv"), MIRROR)
    if mode == "all":
        want = O.bh_fdr(want.reshape(-1)).reshape(want.shape)
    _assert_table(out, LISTED, events, want)


@gpu
def test_pairwise_cli_pair_list_with_row_filter(ctx, golden_dir, tmp_path):
    from splicedice_amd import pairwise
    d = os.path.join(golden_dir, "pairwise")
    out = tmp_path / "pw.tsv"
    _quiet(pairwise.run_with, _ns(d, out, "none", _pair_file(tmp_path, LISTED), filt=os.path.join(d, "filter.txt")), ctx=ctx)
    events, want = _golden_columns(os.path.join(d, "expected_none_filtered.tsv"), MIRROR)
    assert 0 < len(events) < 48
    _assert_table(out, LISTED, events, want)


@gpu
@pytest.mark.parametrize("mode", ["none", "pairwise"])
def test_pairwise_cli_pair_list_fractional_counts(ctx, golden_dir, tmp_path, mode):
    from splicedice_amd import pairwise
    d = os.path.join(golden_dir, "pairwise_fractional")
    out = tmp_path / "pwf.tsv"
    named = [("p5", "p2"), ("p0", "p4")]
    _quiet(pairwise.run_with, _ns(d, out, mode, _pair_file(tmp_path, named)), ctx=ctx)
    events, want = _golden_columns(os.path.join(d, f"expected_{mode}.tsv"), ["p2_p5", "p0_p4"])
    _assert_table(out, named, events, want)


@gpu
@pytest.mark.parametrize("mode", ["none", "pairwise"])
def test_pairwise_cli_pair_list_chi2(ctx, golden_dir, tmp_path, mode):
    from splicedice_amd import pairwise
    d = os.path.join(golden_dir, "pairwise")
    out = tmp_path / "chi2.tsv"
    _quiet(pairwise.run_with, _ns(d, out, mode, _pair_file(tmp_path, LISTED), chi2=True, table="in_inclusionCounts_pos.tsv"), ctx=ctx)
    events, want = _golden_columns(os.path.join(d, f"expected_chi2_{mode}.tsv"), MIRROR)
    _assert_table(out, LISTED, events, want)


@gpu
def test_pairwise_cli_chi2_aborts_only_for_a_listed_sample(ctx, golden_dir, tmp_path):
    """the positive count table with sample p2 set to zero everywhere: p2 has no inclusion and no exclusion counts, so
    every table with p2 has a zero expected frequency and no other has.  A list without p2 runs and equals the
    reference's columns; a list with p2 dies with the reference's message and writes no file"""
    from splicedice_amd import pairwise
    d = os.path.join(golden_dir, "pairwise")
    rows = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(d, "in_inclusionCounts_pos.tsv"))]
    c = rows[0].index("p2")
    table = tmp_path / "counts.tsv"
    table.write_text("".join("\t".join(r[:c] + ([r[c]] if k == 0 else ["0"]) + r[c + 1:]) + "\n" for k, r in enumerate(rows)))
    named = [("p0", "p3"), ("p4", "p1"), ("p5", "p0")]
    out = tmp_path / "ok.tsv"
    _quiet(pairwise.run_with, _ns(d, out, "none", _pair_file(tmp_path, named), chi2=True, table=str(table)), ctx=ctx)
    events, want = _golden_columns(os.path.join(d, "expected_chi2_none.tsv"), ["p0_p3", "p1_p4", "p0_p5"])
    _assert_table(out, named, events, want)
    out = tmp_path / "dies.tsv"
    with pytest.raises(ValueError, match="expected frequencies has a zero element") as e:
        _quiet(pairwise.run_with, _ns(d, out, "none", _pair_file(tmp_path, named + [("p2", "p4")]), chi2=True, table=str(table)),
               ctx=ctx)
    assert f"({len(events)} of {len(events) * 4} " in str(e.value) and not out.exists()


# ------------------------------------------------------------------------------ the sharded pipeline, world 1
@gpu
def test_sharded_pair_list_on_engine(ctx):
    """pairwise_sharded(pairs=...) on the HIP engine: SingleComm and the library's RCCL communicator at world 1, one and
    several column groups, all three corrections and chi2 -- equal to the single-context calls"""
    from splicedice_amd import distributed, synth
    from splicedice_amd.engine import Context
    n, s = 700, 9
    cr, l, r, st = synth.make_junctions(n, 33, n_chrom=2)
    row_of, row_ptr, col = O.cluster_csr(cr, l, r, st)
    counts_in = synth.make_counts(n, s, 34, mean=20)
    counts = np.zeros_like(counts_in)
    counts[row_of] = counts_in
    pairs = np.array([(0, 8), (7, 1), (2, 3), (3, 2), (0, 8), (5, 4), (6, 0)], np.int32)
    excl = ctx.ps(counts, row_ptr, col, want_excl=True, want_ps=False)
    raw = ctx.fisher_pairs(counts, excl, pairs=pairs)
    where = {p: q for q, p in enumerate(O.pair_list(s))}
    full = O.fisher_pairs(counts[:40], excl[:40])
    np.testing.assert_allclose(raw[:40], full[:, [where[(min(i, j), max(i, j))] for i, j in pairs.tolist()]], rtol=1e-9, atol=0)
    want = {"none": raw, "pairwise": ctx.bh_columns(raw), "all": ctx.bh(raw.reshape(-1)).reshape(raw.shape)}
    single = {}
    for mode, w in want.items():
        out = distributed.pairwise_sharded(ctx, distributed.SingleComm(), counts, row_ptr, col, mode, pairs=pairs)
        assert out["own"] == (0, n) and out["p"].shape == (n, len(pairs))
        if mode == "none":
            assert np.array_equal(out["p"], w)
        else:
            np.testing.assert_allclose(out["p"], w, rtol=1e-12, atol=0)
        single[mode] = out["p"]
    np.testing.assert_allclose(single["pairwise"], O.bh_columns(raw), rtol=1e-12, atol=0)
    np.testing.assert_allclose(single["all"], O.bh_fdr(raw.reshape(-1)).reshape(raw.shape), rtol=1e-12, atol=0)
    # chi2: rows in overlapping pairs (2i <-> 2i + 1), counts >= 1, so that no table has an empty row or column
    c2 = np.random.default_rng(35).integers(1, 60, size=(40, s)).astype(np.int32)
    rp2, col2 = np.arange(41, dtype=np.int64), (np.arange(40) ^ 1).astype(np.int32)
    p2, bad = ctx.chi2_pairs(c2, ctx.ps(c2, rp2, col2, want_excl=True, want_ps=False), pairs=pairs)
    assert bad == 0
    out = distributed.pairwise_sharded(ctx, distributed.SingleComm(), c2, rp2, col2, "none", test="chi2", pairs=pairs)
    assert np.array_equal(out["p"], p2)
    with Context(0) as c:
        comm = distributed.RcclComm(c, 0, 1, lambda b, n_: b)
        for mode in want:
            out = distributed.pairwise_sharded(c, comm, counts, row_ptr, col, mode, pairs=pairs)
            assert np.array_equal(out["p"], single[mode]), mode
        out = distributed.pairwise_sharded(c, comm, c2, rp2, col2, "pairwise", test="chi2", pairs=pairs)
        np.testing.assert_allclose(out["p"], O.bh_columns(p2), rtol=1e-12, atol=0)
        for groups in (2, 7):
            out = distributed.pairwise_sharded(c, comm, counts, row_ptr, col, "pairwise", overlap_groups=groups, pairs=pairs)
            assert np.array_equal(out["p"], single["pairwise"]), groups
        # the shard object itself: the list is packed once in load(), two steps give the same rows
        plan = [dict(own_lo=0, own_hi=n, ext_lo=0, ext_hi=n)]
        sh = distributed.PairwiseShard(c, comm, n, s, plan, "none", "fisher", pair_list=pairs)
        try:
            sh.load(counts, row_ptr, col)
            sh.step()
            first = sh.result()
            sh.step()
            assert np.array_equal(first, raw) and np.array_equal(sh.result(), raw)
        finally:
            sh.free()
