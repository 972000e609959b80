"""CPU: `pairwise` over a chosen list of sample pairs -- everything above the kernels.

- the C ABI declares the pair-list entry points and the ctypes table binds them (the library must export them:
  tests/test_abi_and_host.py::test_library_exports_every_declared_symbol);
- `--pairs FILE`: default, parsing, every error before an engine exists, header and `Analyzing pairs:` line;
- pairwise.run_with on a host stand-in engine (scipy per listed table) with the reference-written goldens of
  tests/golden/pairwise: the listed columns of expected_none.tsv / expected_pairwise.tsv, `all` = BH over the listed
  p-values;
- distributed.pairwise_sharded(..., pairs=...) at world 2 (gloo), every rank holding its rows only, all three
  correction modes, equal to the single-process result; pairs=None unchanged;
- PairwiseShard with a list on a recording engine: the list is packed in load(), step() stays free of allocation and
  synchronisation and hands the device table to the kernel call.

The same checks on the real engine: tests/test_gpu_pair_list.py.
"""
import argparse
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle_np as O  # noqa: E402
from pair_fixtures import ListEngine, _IntoComm, _RecArray, _RecEngine, _args, _pair_file, _quiet  # noqa: E402

P_RTOL = 1e-9        # p-values against scipy (tests/test_gpu_parity.py)
LISTED = [("p0", "p3"), ("p4", "p1"), ("p2", "p5")]          # the second pair reversed
MIRROR = ["p0_p3", "p1_p4", "p2_p5"]                         # the golden columns they equal


def _read(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return rows[0], [r[0] for r in rows[1:]], np.array([[float(x) for x in r[1:]] for r in rows[1:]])


# ------------------------------------------------------------------------------ the ABI
def test_header_and_ctypes_table_name_the_pair_list_entry_points():
    from splicedice_amd import _ffi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdice.h")).read()
    for name in ("sdice_fisher_pair_list", "sdice_chi2_pair_list", "sdice_pair_list_pack_dev", "sdice_fisher_pair_list_dev",
                 "sdice_chi2_pair_list_dev"):
        assert f"int {name}(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(_ffi.load(), name), name
    assert "#define SDICE_ABI_VERSION 1\n" in header


def test_pair_array_normalises_and_refuses():
    from splicedice_amd.engine import pair_array
    a = pair_array([(0, 3), (4, 1)])
    assert a.dtype == np.int32 and a.shape == (2, 2) and a.flags.c_contiguous
    for bad in ([], [(0, 1, 2)], [0, 1], np.zeros((0, 2), np.int32)):
        with pytest.raises(ValueError):
            pair_array(bad)
    with pytest.raises(TypeError):
        pair_array([(0.5, 1.0)])


# ------------------------------------------------------------------------------ --pairs: parser and file
def test_pairs_flag_defaults_to_none():
    from splicedice_amd import pairwise
    p = argparse.ArgumentParser()
    pairwise.add_parser(p)
    ns = p.parse_args(["--inclusionSPLICEDICE", "a", "-c", "b"])
    assert ns.pairs is None
    assert p.parse_args(["--inclusionSPLICEDICE", "a", "-c", "b", "--pairs", "list.txt"]).pairs == "list.txt"


def test_read_pair_list_tabs_whitespace_blank_lines_and_order(tmp_path):
    from splicedice_amd import pairwise
    samples = ["p0", "p1", "with space", "p3"]
    f = _pair_file(tmp_path, "p0\tp3\n\n  \np3 p1\r\nwith space\tp0\n   p1   p0  \n")
    assert pairwise.read_pair_list(f, samples) == [(0, 3), (3, 1), (2, 0), (1, 0)]


@pytest.mark.parametrize("text,line,token", [
    ("p0\tp3\np0\tnope\n", 2, "nope"),                       # a name that is not in the header
    ("p0\tp3\np1\n", 2, "p1"),                               # one name
    ("p0 p1 p2\n", 1, "p0 p1 p2"),                           # three names
    ("p0\tp1\tp2\n", 1, "p0"),                               # three names, tab separated
    ("p0\tp3\n\np2\tp2\n", 3, "p2"),                         # a sample paired with itself
    ("p0\tp3\np3\tp0\np0 p3\n", 3, "p3"),                    # the same ordered pair twice (the reversed one is another pair)
])
def test_pair_list_errors_name_file_line_and_token_before_any_engine(tmp_path, golden_dir, monkeypatch, text, line, token):
    from splicedice_amd import pairwise
    f = _pair_file(tmp_path, text)
    with pytest.raises(ValueError) as e:
        pairwise.read_pair_list(f, ["p0", "p1", "p2", "p3"])
    assert f"{f}:{line}:" in str(e.value) and token in str(e.value)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the pair list was checked")
    monkeypatch.setattr(pairwise, "Context", no_engine)
    out = tmp_path / "o.tsv"
    with pytest.raises(ValueError) as e2:
        _quiet(pairwise.run_with, _args(golden_dir, out, pairs=f))
    assert f"{f}:{line}:" in str(e2.value) and not out.exists()


def test_empty_pair_list_is_refused_before_any_engine(tmp_path, golden_dir, monkeypatch):
    from splicedice_amd import pairwise
    f = _pair_file(tmp_path, "\n   \n")
    monkeypatch.setattr(pairwise, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("engine created")))
    with pytest.raises(ValueError, match="empty") as e:
        _quiet(pairwise.run_with, _args(golden_dir, tmp_path / "o.tsv", pairs=f))
    assert f in str(e.value)


# ------------------------------------------------------------------------------ run_with on the host stand-in
def _listed_file(tmp_path):
    return _pair_file(tmp_path, "".join(f"{a}\t{b}\n" for a, b in LISTED))


def test_header_and_analyzing_pairs_line_with_a_reversed_pair(tmp_path, golden_dir):
    from splicedice_amd import pairwise
    out = tmp_path / "o.tsv"
    eng = ListEngine()
    text = _quiet(pairwise.run_with, _args(golden_dir, out, pairs=_listed_file(tmp_path)), ctx=eng)
    lines = text.splitlines()
    assert lines[lines.index("Analyzing pairs:") + 1] == "p0_p3,p4_p1,p2_p5"
    header, events, _ = _read(out)
    assert header == ["clusterID", "p0_p3", "p4_p1", "p2_p5"]
    assert events == _read(os.path.join(golden_dir, "pairwise", "expected_none.tsv"))[1]
    assert eng.calls == [[[0, 3], [4, 1], [2, 5]]]


@pytest.mark.parametrize("mode", ["none", "pairwise", "all"])
def test_run_with_pair_list_equals_the_golden_columns(tmp_path, golden_dir, mode):
    """none / pairwise: columns p0_p3, p1_p4, p2_p5 of the reference-written tables (the reversed pair against its mirror
    column: the two-sided p is symmetric under the column swap); all: BH over the three selected raw columns"""
    from splicedice_amd import pairwise
    out = tmp_path / "o.tsv"
    _quiet(pairwise.run_with, _args(golden_dir, out, mode=mode, pairs=_listed_file(tmp_path)), ctx=ListEngine())
    _, events, got = _read(out)
    gdir = os.path.join(golden_dir, "pairwise")
    header, want_events, want = _read(os.path.join(gdir, "expected_pairwise.tsv" if mode == "pairwise" else "expected_none.tsv"))
    sel = want[:, [header.index(c) - 1 for c in MIRROR]]
    if mode == "all":
        sel = O.bh_fdr(sel.reshape(-1)).reshape(sel.shape)
    assert events == want_events and got.shape == sel.shape == (48, 3)
    assert (np.abs(got - sel) <= P_RTOL * sel).all(), float(np.max(np.abs(got - sel) / sel))


def test_run_with_pair_list_and_row_filter(tmp_path, golden_dir):
    from splicedice_amd import pairwise
    gdir = os.path.join(golden_dir, "pairwise")
    out = tmp_path / "o.tsv"
    _quiet(pairwise.run_with, _args(golden_dir, out, pairs=_listed_file(tmp_path), filt=os.path.join(gdir, "filter.txt")),
           ctx=ListEngine())
    _, events, got = _read(out)
    header, want_events, want = _read(os.path.join(gdir, "expected_none_filtered.tsv"))
    sel = want[:, [header.index(c) - 1 for c in MIRROR]]
    assert events == want_events and 0 < len(events) < 48
    assert (np.abs(got - sel) <= P_RTOL * sel).all()


def test_run_with_chi2_aborts_only_when_a_listed_pair_has_a_zero_expected_frequency(tmp_path, golden_dir):
    """in_inclusionCounts.tsv has rows where p1 and p2 are both zero (row 3): the all-pairs --chi2 run dies there
    (tests/golden/pairwise/chi2_on_zero_rows.json); a list that pairs neither with the other's zero runs or dies by its
    own tables alone"""
    from splicedice_amd import pairwise
    from splicedice_amd.distributed import CHI2_ZERO_MSG
    eng = ListEngine()
    out = tmp_path / "bad.tsv"
    with pytest.raises(ValueError, match=CHI2_ZERO_MSG):
        _quiet(pairwise.run_with, _args(golden_dir, out, chi2=True, pairs=_pair_file(tmp_path, "p1\tp2\n")), ctx=eng)
    assert not out.exists()
    # the positive table: the listed columns of the reference's chi2 table
    out = tmp_path / "good.tsv"
    _quiet(pairwise.run_with, _args(golden_dir, out, chi2=True, pairs=_listed_file(tmp_path), table="in_inclusionCounts_pos.tsv"),
           ctx=eng)
    header, _, want = _read(os.path.join(golden_dir, "pairwise", "expected_chi2_none.tsv"))
    got = _read(out)[2]
    sel = want[:, [header.index(c) - 1 for c in MIRROR]]
    assert (np.abs(got - sel) <= P_RTOL * sel).all()


def test_run_without_pairs_makes_the_calls_of_today(tmp_path, golden_dir):
    """no list: the engine methods are called without the keyword (an engine that does not know it keeps working) and
    the output is the all-pairs table"""
    from splicedice_amd import pairwise
    eng = ListEngine()
    out = tmp_path / "o.tsv"
    ns = _args(golden_dir, out)
    del ns.pairs                                               # (a caller's namespace from before the flag existed)
    _quiet(pairwise.run_with, ns, ctx=eng)
    assert eng.calls == [None]
    header, _, got = _read(out)
    want_header, _, want = _read(os.path.join(golden_dir, "pairwise", "expected_none.tsv"))
    assert header == want_header and (np.abs(got - want) <= P_RTOL * want).all()


# ------------------------------------------------------------------------------ pairwise_sharded, world 2 (gloo)
def _problem():
    from splicedice_amd import synth
    n, s = 260, 6
    cr, l, r, st = synth.make_junctions(n, 19, n_chrom=2)
    row_of, row_ptr, col = O.cluster_csr(cr, l, r, st)
    counts_in = synth.make_counts(n, s, 20, mean=15)
    counts = np.zeros_like(counts_in)
    counts[row_of] = counts_in
    return counts, row_ptr, col


def _chi2_problem():
    """40 rows in overlapping pairs (2i <-> 2i + 1), 6 samples, counts >= 1: every 2x2 table has positive margins"""
    n, s = 40, 6
    counts = np.random.default_rng(78).integers(1, 60, size=(n, s)).astype(np.int32)
    return counts, np.arange(n + 1, dtype=np.int64), (np.arange(n) ^ 1).astype(np.int32)


SHARD_LIST = np.array([(0, 3), (4, 1), (2, 5), (5, 0), (0, 3)], dtype=np.int32)      # reversed pairs and a repeat


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from splicedice_amd import distributed, shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        counts, row_ptr, col = _problem()
        part = shard.shard_plan(row_ptr, col, world)[rank]
        mine = counts[part["ext_lo"]:part["ext_hi"]].copy()      # a rank is handed ITS rows only
        del counts
        res = {}
        for mode in ("pairwise", "none", "all"):
            out = distributed.pairwise_sharded(ListEngine(), distributed.GlooComm(), mine, row_ptr, col, mode, pairs=SHARD_LIST)
            res[mode] = (out["own"], out["p"])
        c2, rp2, col2 = _chi2_problem()
        part2 = shard.shard_plan(rp2, col2, world)[rank]
        out = distributed.pairwise_sharded(ListEngine(), distributed.GlooComm(), c2[part2["ext_lo"]:part2["ext_hi"]].copy(), rp2,
                                           col2, "pairwise", test="chi2", pairs=SHARD_LIST[:3])
        res["chi2"] = (out["own"], out["p"])
        out = distributed.pairwise_sharded(ListEngine(), distributed.GlooComm(), mine, row_ptr, col, "pairwise")
        res["all_pairs"] = (out["own"], out["p"])
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_pair_list_equals_single_process():
    import torch.multiprocessing as mp
    from splicedice_amd import distributed
    world = 2
    counts, row_ptr, col = _problem()
    _, excl = O.calculate_psi_vectorised(counts, row_ptr, col)
    raw = ListEngine().fisher_pairs(counts, excl, pairs=SHARD_LIST)
    full = O.fisher_pairs(counts, excl)
    # the list against the all-pairs oracle: natural pairs equal their column, reversed ones their mirror column
    where = {p: q for q, p in enumerate(O.pair_list(6))}
    for q, (i, j) in enumerate(SHARD_LIST.tolist()):
        np.testing.assert_allclose(raw[:, q], full[:, where[(min(i, j), max(i, j))]], rtol=P_RTOL, atol=0)
    want = {"none": raw, "pairwise": O.bh_columns(raw), "all": O.bh_fdr(raw.reshape(-1)).reshape(raw.shape)}
    for mode in ("none", "pairwise", "all"):
        single = distributed.pairwise_sharded(ListEngine(), distributed.SingleComm(), counts, row_ptr, col, mode, pairs=SHARD_LIST)
        assert single["own"] == (0, counts.shape[0]) and np.array_equal(single["p"], want[mode]), mode
    c2, rp2, col2 = _chi2_problem()
    p2, bad2 = ListEngine().chi2_pairs(c2, O.calculate_psi_vectorised(c2, rp2, col2)[1], pairs=SHARD_LIST[:3])
    assert bad2 == 0
    want["chi2"] = O.bh_columns(p2)
    single = distributed.pairwise_sharded(ListEngine(), distributed.SingleComm(), c2, rp2, col2, "pairwise", test="chi2",
                                          pairs=SHARD_LIST[:3])
    assert np.array_equal(single["p"], want["chi2"])
    want["all_pairs"] = O.bh_columns(full)                       # pairs=None: what the existing world-2 test expects
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    covered = 0
    for rank, res in results:
        for mode, w in want.items():
            (lo, hi), got = res[mode]
            assert got.shape == (hi - lo, w.shape[1]), (rank, mode)
            assert np.array_equal(got, w[lo:hi]), (rank, mode)
        covered += res["none"][0][1] - res["none"][0][0]
    assert covered == counts.shape[0]


def test_sharded_chi2_counts_the_listed_tables_only():
    """one sample with zero counts in one row: a list without it runs, a list with it aborts"""
    from splicedice_amd import distributed
    c2, rp2, col2 = _chi2_problem()
    c2[6, 5] = c2[7, 5] = 0                                    # rows 6 and 7 are each other's exclusions: sample 5 is empty there
    run = lambda pairs: distributed.pairwise_sharded(ListEngine(), distributed.SingleComm(), c2, rp2, col2, "none", test="chi2",
                                                     pairs=pairs)
    assert run([(0, 3), (4, 1), (2, 4)])["p"].shape == (40, 3)
    with pytest.raises(ValueError, match=r"zero element \(2 of 80 "):
        run([(0, 1), (5, 4)])


def test_sharded_pair_list_is_checked():
    from splicedice_amd import distributed
    counts, row_ptr, col = _problem()
    for bad in ([(0, 6)], [(-1, 2)], [(3, 3)], []):
        with pytest.raises(ValueError):
            distributed.pairwise_sharded(ListEngine(), distributed.SingleComm(), counts, row_ptr, col, "none", pairs=bad)


# ------------------------------------------------------------------------------ the sub-command under a 2-rank launcher
def _cli_worker(rank, world, port, outdir, golden, pair_file):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from splicedice_amd import pairwise
    for mode in ("pairwise", "all", "none"):
        pairwise.run_with(_args(golden, os.path.join(outdir, f"{mode}.tsv"), mode=mode, pairs=pair_file), ctx=ListEngine())
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_pairs_flag_under_two_rank_launcher(tmp_path, golden_dir):
    """both ranks run `pairwise --pairs` on their rows through pairwise_sharded; ONE set of output files, equal to the
    listed columns of the reference-written goldens"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    pair_file = _listed_file(tmp_path)
    outdir = tmp_path / "out"
    outdir.mkdir()
    mpctx = mp.get_context("spawn")
    procs = [mpctx.Process(target=_cli_worker, args=(r, 2, port, str(outdir), golden_dir, pair_file)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    gdir = os.path.join(golden_dir, "pairwise")
    for mode in ("pairwise", "all", "none"):
        header, events, got = _read(outdir / f"{mode}.tsv")
        wh, want_events, want = _read(os.path.join(gdir, "expected_pairwise.tsv" if mode == "pairwise" else "expected_none.tsv"))
        sel = want[:, [wh.index(c) - 1 for c in MIRROR]]
        if mode == "all":
            sel = O.bh_fdr(sel.reshape(-1)).reshape(sel.shape)
        assert header == ["clusterID", "p0_p3", "p4_p1", "p2_p5"] and events == want_events
        assert (np.abs(got - sel) <= P_RTOL * sel).all(), mode
    assert not [f for f in os.listdir(outdir) if ".part" in f]


# ------------------------------------------------------------------------------ PairwiseShard with a list: load() and step()
@pytest.mark.parametrize("correction,test", [("pairwise", "fisher"), ("all", "fisher"), ("none", "chi2")])
def test_shard_packs_the_list_in_load_and_step_stays_device_work_only(correction, test):
    from splicedice_amd import distributed

    class Eng(_RecEngine):
        def pair_table(self, s, pairs):
            self.calls.append("pair_table")
            self.allocated.append(_RecArray(self, (len(pairs),), np.uint32, self._address(), owned=True))
            self.tab = self.allocated[-1]
            return self.tab

    seen = []
    for name in ("fisher_pairs_dev", "chi2_pairs_dev"):
        setattr(Eng, name, lambda self, *a, _n=name, **kw: (self.calls.append(_n), seen.append((_n, kw))))
    s, plan = 6, [dict(own_lo=0, own_hi=5, ext_lo=0, ext_hi=6), dict(own_lo=5, own_hi=9, ext_lo=4, ext_hi=9)]
    for rank in (0, 1):
        eng = Eng()
        eng.views = []
        rows = plan[rank]["ext_hi"] - plan[rank]["ext_lo"]
        sh = distributed.PairwiseShard(eng, _IntoComm(eng, rank, 2), 9, s, plan, correction, test, overlap_groups=1,
                                       pair_list=SHARD_LIST)
        assert sh.pairs == len(SHARD_LIST) and sh.ranges == distributed.pair_column_ranges(len(SHARD_LIST), 2)
        assert "pair_table" not in eng.calls
        sh.load(np.ones((rows, s), np.int32), np.arange(rows + 1, dtype=np.int64), np.zeros(rows, np.int32))
        assert eng.calls.count("pair_table") == 1
        for _ in range(2):
            eng.calls.clear()
            seen.clear()
            sh.step()
            assert not {"empty", "to_device", "sync", "pair_table"} & set(eng.calls), eng.calls
            assert len(seen) == 1 and seen[0][0] == f"{'chi2' if test == 'chi2' else 'fisher'}_pairs_dev"
            assert seen[0][1] == {"pairs": eng.tab}
        sh.free()
        assert all(a.free_calls == 1 and a.ptr is None for a in eng.allocated)
