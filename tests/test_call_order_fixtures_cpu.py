"""No GPU: every case of call_order_fixtures.py has a reference, and none is degenerate -- the conditions under which
test_gpu_call_order.py can tell a call that read stale scratch from one that did not."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_order_fixtures as CF  # noqa: E402
import cluster_referee as CR  # noqa: E402
import dunn_fixtures as DF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import large_path_fixtures as LP  # noqa: E402
import rank_support as RS  # noqa: E402
import shift_referee as SH  # noqa: E402
from splicedice_amd import engine  # noqa: E402


@pytest.mark.parametrize("name", list(CF.CASES))
def test_case_has_a_reference_that_says_something(name):
    case = CF.CASES[name]
    want = case.want
    assert want and all(isinstance(v, np.ndarray) for v in want.values())
    for field, v in want.items():
        assert v.size > 0, field
        if v.dtype == np.uint8 and field not in case.constant:          # a boolean output takes both values
            assert set(np.unique(v).tolist()) == {0, 1}, (name, field)
    # no output whose reference an all-zero array would satisfy (the h of kruskal and kruskal_dunn is the referee's hf)
    for field in case.outputs:
        if field not in case.constant:
            assert np.any(want["hf" if name in ("kruskal", "kruskal_dunn") and field == "h" else field] != 0), (name, field)
    assert case.want is want and case.inputs is case.inputs               # computed once, shared


def test_every_dev_entry_point_is_in_the_catalogue_or_named_as_left_out():
    dev = {m for m in dir(engine.Context) if m.endswith("_dev")}
    source = open(CF.__file__.replace(".pyc", ".py")).read()
    head, body = source.split('"""', 2)[1:]
    for m in sorted(dev):
        assert (m in body) or (m in head), m
    assert "sort_unique_u64" in body


def test_cluster_cases_take_the_paths_they_claim():
    for name, n, buckets in (("cluster->ps", CF.CLUSTER_LARGE, True), ("cluster->ps one bucket", CF.CLUSTER_SMALL, False),
                             ("cluster generic->ps", CF.CLUSTER_LARGE, True)):
        case = CF.CASES[name]
        cr, left, right, _ = case.inputs["junctions"]
        assert cr.size == n and case.inputs["counts"].shape == (n, CF.PS_COLS) and CF.PS_COLS % 4 == 0
        plan = CR.sort_plan(cr, left, right)
        assert (plan.B > 1) == buckets and (plan.S > 0) == buckets and not plan.overflow
        assert (n <= CF.CLUSTER_ONE_BUCKET_MAX) == (not buckets)
        want = case.want
        nnz = int(want["row_ptr"][-1])
        assert nnz > 0 and want["col"].size == nnz
        rows = np.repeat(np.arange(n), np.diff(want["row_ptr"]))
        assert np.abs(want["col"] - rows).max() > 0                       # block reach > 0 somewhere
        assert 16 * n + 1024 >= nnz                                       # (the list fits the first capacity: one neighbour pass)
        assert np.isnan(want["ps"]).any() and (want["ps"] > 0).any() and (want["excl"] > 0).any()
    assert CF.CASES["cluster generic->ps"].knobs == {"cluster.generic": 1}
    assert CF.CASES["cluster generic->ps"].inputs["junctions"][1].tobytes() == CF.CASES["cluster->ps"].inputs["junctions"][1].tobytes()


def test_unique_case_has_duplicates():
    keys = CF.CASES["sort_unique_u64"].inputs["keys"]
    assert keys.size == 10_000 and 100 < keys.size - np.unique(keys).size < keys.size - 100
    assert (np.diff(keys.astype(np.float64)) < 0).any()                   # not sorted


def test_bh_cases_sit_on_their_paths():
    assert CF.BH_RADIX_M < LP.BH_VECTOR_SAMPLESORT_MIN <= CF.BH_SAMPLESORT_M <= LP.BH_VECTOR_SAMPLESORT_MAX
    assert CF.BH_SAMPLESORT_M == LP.BH_VECTOR_SAMPLESORT_MIN + 1
    for tag, m in (("radix", CF.BH_RADIX_M), ("sample sort", CF.BH_SAMPLESORT_M)):
        x = CF.CASES[f"bh vector {tag} masked"].inputs
        assert x["p"].size == m and 0.2 * m < x["tested"].sum() < 0.8 * m          # present and absent entries
        want = CF.CASES[f"bh vector {tag} masked"].want["q_mask"]
        assert not want[x["tested"] == 0].any() and want[x["tested"] != 0].any()
    for name, case in CF.CASES.items():
        if name.startswith("bh columns"):
            n, pitch = case.inputs["table"].shape
            assert n <= LP.BH_COLS_SAMPLESORT_MAX and case.inputs["c0"] + case.inputs["cols"] <= pitch
            assert (case.want["table"] != case.inputs["table"]).any()
    # bh_cols.hip, sd_bh_cols_samplesort: more than one bucket from 4 * bh.wg (256 threads) values per column on
    assert CF.CASES[CF.BH_COLUMNS_SAMPLESORT].inputs["table"].shape == (5000, 20) and 5000 > 4 * 256
    three = CF.CASES["bh columns sample sort three groups"]
    assert -(-three.inputs["cols"] // three.knobs["bh.max_group"]) == 3
    pitched = CF.CASES["bh columns pitched"]
    assert 0 < pitched.inputs["c0"] and pitched.inputs["cols"] < pitched.inputs["table"].shape[1]


def test_pair_cases():
    for name in ("fisher_pairs", "fisher_pair_list", "chi2_pairs", "chi2_pair_list"):
        case = CF.CASES[name]
        assert case.inputs["incl"].shape == (64, CF.PAIR_S)
        m = len(CF.PAIR_LIST) if name.endswith("list") else CF.PAIR_S * (CF.PAIR_S - 1) // 2
        assert case.want["p"].shape == (64, m)
        if name.startswith("chi2"):
            assert int(case.want["n_bad"][0]) == int(np.isnan(case.want["p"]).sum()) > 0           # bad tables
            assert int(case.want["n_bad"][0]) < case.want["p"].size // 2
        else:
            assert not np.isnan(case.want["p"]).any() and (case.want["p"] < 1e-3).any() and (case.want["p"] == 1.0).any()
    assert (CF.PAIR_LIST[:, 0] > CF.PAIR_LIST[:, 1]).any() and len(np.unique(CF.PAIR_LIST, axis=0)) < len(CF.PAIR_LIST)


def test_gram_case_has_absent_values():
    x = CF.CASES["sample_gram"].inputs
    assert x["ps"].shape == (200, 15) and x["cols"].size == 12 and np.isnan(x["ps"][:, x["cols"]]).mean() > 0.1
    want = CF.CASES["sample_gram"].want
    assert 0 < want["shared"].min() < want["shared"].max() <= 200
    two = CF.CASES["sample_gram two tiles"]
    assert two.inputs["ps"].shape[0] == 200 and CF.GRAM_TILE < two.inputs["cols"].size <= 2 * CF.GRAM_TILE
    assert np.isnan(two.inputs["ps"]).any() and (two.want["sum1"] != two.want["sum1"].T).any()


def test_row_table_drives_both_kernels_of_every_test():
    ps = CF.row_table()
    assert ps.shape == (CF.ROWS, CF.ROW_COLS) == (200, 40) and ps.dtype == np.float32
    grid_rows = RS.on_grid(ps).all(axis=1)
    some = ~np.isnan(ps).all(axis=1)
    assert (grid_rows & some).sum() > 100 and (~grid_rows).sum() >= 30
    for name in ("ranksum", "ranksum_strata", "ranksum_exact", "signedrank", "signedrank_exact", "ks", "ks exact", "shift",
                 "kruskal", "kruskal_dunn", "jonckheere", "spearman"):
        t = CF.CASES[name].want["tested"].astype(bool)
        assert (t & grid_rows).sum() >= 50 and (t & ~grid_rows).sum() >= 15 and (~t).sum() >= 10, name
    assert len(CF.SETS) == 3 and np.unique(np.concatenate(CF.SETS)).size == sum(g.size for g in CF.SETS)
    assert not np.intersect1d(CF.G1, CF.G2).size and not np.intersect1d(CF.PAIR_A, CF.PAIR_B).size
    strata = CF.CASES["ranksum_strata"].want
    assert strata["cond"][strata["tested"].astype(bool)].max() <= CF.COND_MAX
    for name in ("ranksum_exact", "ks exact"):             # both p forms among the tested rows
        w = CF.CASES[name].want
        on = w["exact"].astype(bool)
        assert on.sum() >= 15 and (w["tested"].astype(bool) & ~on).sum() >= 15, name
    assert not CF.CASES["ks"].want["exact"].any()
    cols, x = CF.spearman_design()
    assert np.unique(cols).size == 30 and np.unique(x).size < 30


def test_shift_and_dunn_cases_hang_on_no_rounding():
    """shift: more than 10 distinct ranks among the tested rows, each far from a rounding, tested rows on the grid and off it,
    no NaN triple (the table keeps no infinity); Dunn: no Holm order of a row hangs on a rounding, no pair output all zero
    or NaN, and padj reaches 1 and falls below 0.05"""
    want = CF.CASES["shift"].want
    t = want["tested"].astype(bool)
    assert all(not np.isnan(want[name]).any() for name in SH.OUTS)
    assert want["grid"][t].any() and not want["grid"][t].all()
    assert np.unique(want["rank"][t]).size > 10
    for n1, n2 in {(int(a), int(b)) for a, b in zip(want["n1"][t], want["n2"][t])}:
        assert SH.rank_and_margin(n1, n2, SH.zq_of(CF.SHIFT_CONF))[1] >= 1e-6, (n1, n2)
    want = CF.CASES["kruskal_dunn"].want
    t = want["tested"].astype(bool)
    assert all(np.any(want[name] != 0) and not np.isnan(want[name]).any() for name in DF.PAIR)
    assert DR.close_pairs(want, 1e-6) == []
    assert (want["pair_padj"][:, t] == 1.0).any() and (want["pair_padj"][:, t] < 0.05).any()
