"""CPU: the pieces of splicedice_amd/_cli.py that every sub-command goes through, and who closes the engine.

- engine_scope: a context it made is closed exactly once however the block ends; a context it was handed is left open and
  nothing is made;
- pairwise / similarity / find_outliers run_with on host doubles that record close(): the engine the command made is closed
  exactly once on every branch;
- columns_in_header: manifest order, dtype, the two refusal sentences;
- device_call / tested_rows on a context double whose arrays record free(): everything freed on success and when the
  launch raises; the compaction rule;
- the packed all-gather layout of distributed is the rank-sum field table;
- compare_sample_sets.run_with on every subset of the six flags that change the test: the refusal it prints, or that it
  goes on to read the table.
"""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle_np as O  # noqa: E402
from pair_fixtures import ListEngine, _args, _pair_file, _quiet  # noqa: E402
from splicedice_amd import _cli  # noqa: E402


# ------------------------------------------------------------------------------ engine_scope
class _Closable:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


@pytest.mark.parametrize("leave", [None, KeyError, SystemExit])
def test_engine_scope_closes_its_own_context_exactly_once(leave):
    made = []

    def make():
        made.append(_Closable())
        return made[-1]

    def body():
        with _cli.engine_scope(None, make) as c:
            assert c is made[0] and c.closed == 0
            if leave is not None:
                raise leave(1)

    if leave is None:
        body()
    else:
        with pytest.raises(leave):
            body()
    assert len(made) == 1 and made[0].closed == 1


@pytest.mark.parametrize("leave", [None, KeyError, SystemExit])
def test_engine_scope_leaves_a_passed_context_open_and_makes_none(leave):
    mine = _Closable()

    def make():
        raise AssertionError("make() was called although a context was passed")

    def body():
        with _cli.engine_scope(mine, make) as c:
            assert c is mine
            if leave is not None:
                raise leave(1)

    if leave is None:
        body()
    else:
        with pytest.raises(leave):
            body()
    assert mine.closed == 0


# ------------------------------------------------------------------------------ the commands close what they made
def _recording(base, monkeypatch, module):
    """module.Context -> a subclass of the host double `base` that counts close(); -> the list of the instances made"""
    made = []

    class Recording(base):
        def __init__(self, device=0):
            super().__init__()
            self.closed = 0
            made.append(self)

        def close(self):
            self.closed += 1

    monkeypatch.setattr(module, "Context", Recording)
    return made


def test_pairwise_closes_its_engine_once_on_the_host_engine_branch(tmp_path, golden_dir, monkeypatch):
    from splicedice_amd import pairwise
    made = _recording(ListEngine, monkeypatch, pairwise)
    out = tmp_path / "o.tsv"
    _quiet(pairwise.run_with, _args(golden_dir, out))
    assert [e.closed for e in made] == [1] and made[0].calls == [None]
    want = open(os.path.join(golden_dir, "pairwise", "expected_none.tsv")).readline()
    assert open(out).readline() == want


def test_pairwise_closes_its_engine_once_when_no_event_is_left(tmp_path, golden_dir, monkeypatch):
    """a filter that keeps no row: the table is the header alone, no engine method is called, the engine is closed"""
    from splicedice_amd import pairwise
    made = _recording(ListEngine, monkeypatch, pairwise)
    out = tmp_path / "o.tsv"
    _quiet(pairwise.run_with, _args(golden_dir, out, filt=_pair_file(tmp_path, "no_such_event\n", "filter.txt")))
    assert [e.closed for e in made] == [1] and made[0].calls == []
    assert open(out).read() == open(os.path.join(golden_dir, "pairwise", "expected_none.tsv")).readline()


def test_pairwise_closes_its_engine_once_when_chi2_aborts(tmp_path, golden_dir, monkeypatch):
    """the zero-expected-frequency case of tests/golden/pairwise/chi2_on_zero_rows.json: ValueError, no file, one close"""
    from splicedice_amd import pairwise
    from splicedice_amd.distributed import CHI2_ZERO_MSG
    made = _recording(ListEngine, monkeypatch, pairwise)
    out = tmp_path / "o.tsv"
    with pytest.raises(ValueError, match=CHI2_ZERO_MSG):
        _quiet(pairwise.run_with, _args(golden_dir, out, chi2=True))
    assert [e.closed for e in made] == [1] and not out.exists()


def test_pairwise_leaves_a_passed_engine_open(tmp_path, golden_dir, monkeypatch):
    from splicedice_amd import pairwise
    made = _recording(ListEngine, monkeypatch, pairwise)
    mine = pairwise.Context()
    _quiet(pairwise.run_with, _args(golden_dir, tmp_path / "o.tsv"), ctx=mine)
    assert made == [mine] and mine.closed == 0


class _SimilarityEngine:
    """engine.Context.similarity from the oracle"""

    def similarity(self, ps, mid, sign):
        return O.similarity_scores(ps, mid, sign)


def test_similarity_closes_the_engine_it_made(tmp_path, golden_dir, monkeypatch):
    from splicedice_amd import similarity
    made = _recording(_SimilarityEngine, monkeypatch, similarity)
    s, c = os.path.join(golden_dir, "similarity"), os.path.join(golden_dir, "compare")
    out = tmp_path / "scores.tsv"
    similarity.run_with(argparse.Namespace(comparison=os.path.join(c, "expected_out.tsv"), allps=os.path.join(c, "in_allPS.tsv"),
                                           manifest=None, output=str(out)))
    assert [e.closed for e in made] == [1]
    assert open(out).read() == open(os.path.join(s, "expected_scores.tsv")).read()


class _RowstatsEngine:
    """engine.Context.rowstats in plain numpy"""

    def rowstats(self, data, idx):
        sub = data[:, idx]
        with np.errstate(all="ignore"):
            return np.nanmean(sub, axis=1), np.nanstd(sub, axis=1), np.isnan(sub).sum(axis=1).astype(np.int32)


def test_find_outliers_closes_the_engine_it_made(golden_dir, monkeypatch, capsys):
    import warnings
    from splicedice_amd import find_outliers
    made = _recording(_RowstatsEngine, monkeypatch, find_outliers)
    d = os.path.join(golden_dir, "outliers")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # (numpy's "mean of empty slice" on an all-NaN row)
        find_outliers.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "matrix_f64.npz"), manifest=os.path.join(d, "samples.tsv"),
                                                  nullMan=None, outlierCutoff=3, dpsiThrsh=0.1))
    assert [e.closed for e in made] == [1]
    # (the double is plain numpy, not the library's bit-exact row statistics: the reported pairs are the golden's, the
    # printed floats are tests/test_gpu_cli.py's business)
    pairs = [line.split("\t")[:2] for line in capsys.readouterr().out.splitlines()]
    assert pairs and pairs == [line.split("\t")[:2] for line in open(os.path.join(d, "expected_f64_self.txt"))]


# ------------------------------------------------------------------------------ columns_in_header
class _Refused(Exception):
    pass


def _raise(why):
    raise _Refused(why)


def test_columns_in_header_keeps_the_order_of_the_names():
    header = ["s0", "s1", "s2", "s3"]
    idx = _cli.columns_in_header(["s3", "s0"], header, _raise)
    assert idx.dtype == np.int32 and idx.tolist() == [3, 0]
    empty = _cli.columns_in_header([], header, _raise)
    assert empty.dtype == np.int32 and empty.size == 0


def test_columns_in_header_refuses_a_missing_and_a_repeated_name():
    with pytest.raises(_Refused) as e:
        _cli.columns_in_header(["s1", "x"], ["s0", "s1"], _raise)
    assert str(e.value) == "sample 'x' is missing from the table header"
    with pytest.raises(_Refused) as e:
        _cli.columns_in_header(["s0", "s1"], ["s0", "s1", "s2", "s1", "s1"], _raise)
    assert str(e.value) == "sample 's1' appears 3 times in the table header"


def test_refusal_prints_prefix_reason_and_exits_with_status_1(capsys):
    with pytest.raises(SystemExit) as e:
        _cli.refusal("correlate")("sample 'x' is missing from the table header")
    assert e.value.code == 1
    assert capsys.readouterr().err == "correlate: sample 'x' is missing from the table header. Exit.\n"


# ------------------------------------------------------------------------------ device_call / tested_rows
class _FakeArray:
    def __init__(self, host):
        self.host, self.freed = host, 0

    def to_host(self):
        return self.host.copy()

    def free(self):
        self.freed += 1


class _FakeContext:
    """to_device / empty hand out host-backed arrays that count free(); bh_masked_dev is the oracle's BH over the tested
    entries, 0 elsewhere (as sdice_bh_masked_dev)"""

    def __init__(self):
        self.arrays, self.log = [], []

    def to_device(self, host, dtype=None):
        self.log.append("to_device")
        self.arrays.append(_FakeArray(np.array(host, dtype=dtype)))
        return self.arrays[-1]

    def empty(self, shape, dtype):
        self.log.append("empty")
        self.arrays.append(_FakeArray(np.full(shape, 99, dtype)))
        return self.arrays[-1]

    def sync(self):
        self.log.append("sync")

    def bh_masked_dev(self, d_p, d_tested, d_q):
        self.log.append("bh")
        t = d_tested.host != 0
        d_q.host[:] = 0
        d_q.host[t] = O.bh_fdr(d_p.host[t])


N = 7
TESTED = np.array([1, 0, 1, 1, 0, 0, 1], np.uint8)
P = np.array([0.04, 0.5, 0.001, 0.2, 0.9, 0.3, 0.03])
OUTPUTS = {"tested": (N, np.uint8), "p": (N, np.float64), "stat": (N, np.float32), "per_set": ((3, N), np.float32)}


def _launch(d_in, d_out):
    assert d_in["ps"].host.dtype == np.float32 and d_in["cols"].host.dtype == np.int32
    d_out["tested"].host[:] = TESTED
    d_out["p"].host[:] = P
    d_out["stat"].host[:] = np.arange(N)
    d_out["per_set"].host[:] = np.arange(3 * N).reshape(3, N)


def _inputs():
    return {"ps": (np.zeros((N, 4)), np.float32), "cols": ([0, 2], np.int32)}


def test_device_call_returns_every_output_and_frees_every_array():
    ctx = _FakeContext()
    res = _cli.device_call(ctx, _inputs(), OUTPUTS, _launch)
    assert list(res) == list(OUTPUTS) and np.array_equal(res["p"], P) and res["per_set"].shape == (3, N)
    assert ctx.log == ["to_device"] * 2 + ["empty"] * 4 + ["sync"]
    assert [a.freed for a in ctx.arrays] == [1] * 6


def test_device_call_frees_every_array_when_the_launch_raises():
    ctx = _FakeContext()

    def launch(d_in, d_out):
        raise RuntimeError("the launch failed")

    with pytest.raises(RuntimeError, match="the launch failed"):
        _cli.tested_rows(ctx, _inputs(), OUTPUTS, launch)
    assert len(ctx.arrays) == 7 and [a.freed for a in ctx.arrays] == [1] * 7          # (2 inputs, 4 outputs, q)
    assert "sync" not in ctx.log and "bh" not in ctx.log


def test_tested_rows_compacts_to_the_tested_rows_and_corrects_them():
    ctx = _FakeContext()
    keep, r = _cli.tested_rows(ctx, _inputs(), OUTPUTS, _launch)
    assert ctx.log == ["to_device"] * 2 + ["empty"] * 5 + ["bh", "sync"]
    assert [a.freed for a in ctx.arrays] == [1] * 7
    assert np.array_equal(keep, np.flatnonzero(TESTED != 0)) and keep.tolist() == [0, 2, 3, 6]
    assert sorted(r) == ["corrected", "p", "per_set", "stat"]
    assert np.array_equal(r["p"], P[keep]) and np.array_equal(r["stat"], np.arange(N, dtype=np.float32)[keep])
    assert np.array_equal(r["per_set"], np.arange(3 * N, dtype=np.float32).reshape(3, N)[:, keep])
    assert r["per_set"].shape == (3, 4) and r["per_set"].flags.c_contiguous
    assert np.array_equal(r["corrected"], O.bh_fdr(P[keep]))


# ------------------------------------------------------------------------------ the field tables
def test_the_packed_all_gather_layout_is_the_rank_sum_field_table():
    from splicedice_amd import distributed, engine
    assert distributed.STAT_NAMES == ("tested", "p", "z", "med1", "med2", "mean1", "mean2", "delta")
    assert distributed.STAT_DTYPES == (np.uint8, np.float64, np.float64) + (np.float32,) * 5
    assert list(zip(distributed.STAT_NAMES, distributed.STAT_DTYPES)) == engine.RANKSUM_FIELDS


def test_field_shapes_gives_per_set_fields_one_row_per_set():
    from splicedice_amd import engine
    shapes = engine.field_shapes(engine.KRUSKAL_FIELDS, 5, 3)
    assert list(shapes) == ["tested", "p", "h", "med", "mean", "delta"]
    assert shapes["med"] == ((3, 5), np.float32) and shapes["mean"] == ((3, 5), np.float32) and shapes["h"] == (5, np.float64)
    assert engine.field_shapes(engine.GRAM_FIELDS, (4, 4))["prod"] == ((4, 4), np.int64)


# ------------------------------------------------------------------------------ compare_sample_sets: which flags go together
CSS_FLAGS = ("--paired", "--exact", "--strata", "--trend", "--ks", "-mx")
CSS_SUBSETS = [tuple(f for i, f in enumerate(CSS_FLAGS) if bits >> i & 1) for bits in range(1 << len(CSS_FLAGS))]
READS_THE_TABLE = "reads the table"
# subset of CSS_FLAGS -> the first line of stderr at exit status 1, or READS_THE_TABLE when the command gets as far as
# read_ps_table.  Recorded from run_with before the refusals became a table (one row per test): texts and precedence are
# that version's, byte for byte.
CSS_OUTCOMES = {
    (): READS_THE_TABLE,
    ('--paired',): READS_THE_TABLE,
    ('--exact',): READS_THE_TABLE,
    ('--paired', '--exact'): READS_THE_TABLE,
    ('--strata',): READS_THE_TABLE,
    ('--paired', '--strata'):
        'compare_sample_sets --strata: cannot be combined with --paired (the signed-rank test pairs samples '
        'one to one). Exit.',
    ('--exact', '--strata'):
        'compare_sample_sets --strata: cannot be combined with --exact (there is no exact stratified test '
        'here). Exit.',
    ('--paired', '--exact', '--strata'):
        'compare_sample_sets --strata: cannot be combined with --paired (the signed-rank test pairs samples '
        'one to one). Exit.',
    ('--trend',):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--paired', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--exact', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--paired', '--exact', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--strata', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--paired', '--strata', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--exact', '--strata', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--paired', '--exact', '--strata', '--trend'):
        'compare_sample_sets --trend: needs -mx/--moreManifests (three or more ordered sets; two sets are the '
        'rank-sum test). Exit.',
    ('--ks',): READS_THE_TABLE,
    ('--paired', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--ks'): READS_THE_TABLE,
    ('--paired', '--exact', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--strata', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --strata (there is no stratified '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--strata', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--strata', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --strata (there is no stratified '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--exact', '--strata', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--exact', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--strata', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--strata', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--strata', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--exact', '--strata', '--trend', '--ks'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('-mx',): READS_THE_TABLE,
    ('--paired', '-mx'):
        'compare_sample_sets --paired: cannot be combined with -mx/--moreManifests (the signed-rank test '
        'compares two matched sets). Exit.',
    ('--exact', '-mx'):
        'compare_sample_sets --exact: cannot be combined with -mx/--moreManifests (there is no exact '
        'Kruskal-Wallis test here). Exit.',
    ('--paired', '--exact', '-mx'):
        'compare_sample_sets --exact: cannot be combined with -mx/--moreManifests (there is no exact '
        'Kruskal-Wallis test here). Exit.',
    ('--strata', '-mx'):
        'compare_sample_sets --strata: cannot be combined with -mx/--moreManifests (there is no stratified '
        'Kruskal-Wallis test here). Exit.',
    ('--paired', '--strata', '-mx'):
        'compare_sample_sets --strata: cannot be combined with --paired (the signed-rank test pairs samples '
        'one to one). Exit.',
    ('--exact', '--strata', '-mx'):
        'compare_sample_sets --exact: cannot be combined with -mx/--moreManifests (there is no exact '
        'Kruskal-Wallis test here). Exit.',
    ('--paired', '--exact', '--strata', '-mx'):
        'compare_sample_sets --exact: cannot be combined with -mx/--moreManifests (there is no exact '
        'Kruskal-Wallis test here). Exit.',
    ('--trend', '-mx'): READS_THE_TABLE,
    ('--paired', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --paired (the signed-rank test compares two '
        'matched sets). Exit.',
    ('--exact', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --exact (the trend test is asymptotic only). '
        'Exit.',
    ('--paired', '--exact', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --paired (the signed-rank test compares two '
        'matched sets). Exit.',
    ('--strata', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --strata (there is no stratified trend test '
        'here). Exit.',
    ('--paired', '--strata', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --paired (the signed-rank test compares two '
        'matched sets). Exit.',
    ('--exact', '--strata', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --exact (the trend test is asymptotic only). '
        'Exit.',
    ('--paired', '--exact', '--strata', '--trend', '-mx'):
        'compare_sample_sets --trend: cannot be combined with --paired (the signed-rank test compares two '
        'matched sets). Exit.',
    ('--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with -mx/--moreManifests (there is no k-sample '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with -mx/--moreManifests (there is no k-sample '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--exact', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--strata', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with -mx/--moreManifests (there is no k-sample '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--strata', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--strata', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with -mx/--moreManifests (there is no k-sample '
        'Kolmogorov-Smirnov test here). Exit.',
    ('--paired', '--exact', '--strata', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--exact', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--strata', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--strata', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
    ('--exact', '--strata', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --trend (the trend test orders three or more '
        'sets). Exit.',
    ('--paired', '--exact', '--strata', '--trend', '--ks', '-mx'):
        'compare_sample_sets --ks: cannot be combined with --paired (the signed-rank test compares matched '
        'samples; this test compares two distributions). Exit.',
}


class _ReadsTheTable(Exception):
    pass


def _css_outcome(flags, tmp_path, monkeypatch, capsys):
    """run_with on three sets of three samples, a label file and a header-only table; read_ps_table raises the sentinel"""
    from splicedice_amd import compare_sample_sets as css
    sets = [[f"s{3 * g + i}" for i in range(3)] for g in range(3)]
    paths = []
    for g, names in enumerate(sets):
        paths.append(tmp_path / f"m{g + 1}.txt")
        paths[-1].write_text("".join(f"{name}\tbam\n" for name in names))
    strata = tmp_path / "strata.tsv"
    strata.write_text("".join(f"{name}\tbatch{i % 2}\n" for names in sets for i, name in enumerate(names)))
    table = tmp_path / "in_allPS.tsv"
    table.write_text("\t".join(["cluster"] + [name for names in sets for name in names]) + "\n")

    def reads_the_table(*a, **k):
        raise _ReadsTheTable()

    monkeypatch.setattr(css, "read_ps_table", reads_the_table)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    args = argparse.Namespace(psiSPLICEDICE=str(table), manifest1=str(paths[0]), manifest2=str(paths[1]),
                              moreManifests=[str(paths[2])] if "-mx" in flags else None, paired="--paired" in flags,
                              exact="--exact" in flags, strata=str(strata) if "--strata" in flags else None,
                              trend="--trend" in flags, ks="--ks" in flags, annotation="", outputFile=str(tmp_path / "out.tsv"))
    try:
        css.run_with(args, ctx=object())
    except _ReadsTheTable:
        return READS_THE_TABLE
    except SystemExit as e:
        assert e.code == 1
        return capsys.readouterr().err.splitlines()[0]
    raise AssertionError("run_with returned without reading the table")


@pytest.mark.parametrize("flags", CSS_SUBSETS, ids=lambda f: "+".join(f) or "plain")
def test_compare_sample_sets_refuses_or_runs_every_flag_combination_as_before(flags, tmp_path, monkeypatch, capsys):
    assert _css_outcome(flags, tmp_path, monkeypatch, capsys) == CSS_OUTCOMES[flags]
    assert not (tmp_path / "out.tsv").exists()
