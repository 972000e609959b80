"""The host rules of `similarity` and `findOutliers` against the referee (tests/scoring_referee.py), and the referee against
the oracle and against what the reference itself made of the same inputs (tests/golden/similarity_edge, outliers_edge;
recipe: tests/golden/make_golden_scoring.py).  No GPU and no library: the context is a stand-in whose rowstats / similarity
are the referee's functions, and the PS table is parsed by Python's float().
"""
import argparse
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scoring_fixtures as SF  # noqa: E402
import scoring_referee as R  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd import find_outliers, similarity  # noqa: E402

CUTOFFS = (2, 3, 0)


class RefereeEngine:
    """engine.Context.rowstats / similarity from the referee"""

    def rowstats(self, data, idx):
        return R.rowstats_rows(data, idx)

    def similarity(self, ps, mid, sign):
        return R.similarity_counts(ps, mid, sign)


def assert_same_text(got, want):
    """equal texts; the message is the first line that differs (pytest's own diff of a long text takes minutes)"""
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError((f"line {k} of {len(a)} / {len(b)}", a[k:k + 1], b[k:k + 1]))


# ------------------------------------------------------------------------------ the referee against the oracle
def test_similarity_counts_equal_the_oracle_loop():
    """sign in {-1, 0, 1}, where the oracle's branches are the ABI's: the edge table and a random 300 x 70 table"""
    ps, mid, sign, _ = SF.edge_table()
    rng = np.random.default_rng(17)
    rnd = np.round(rng.random((300, 70)), 3)
    rnd[rng.random(rnd.shape) < 0.1] = np.nan
    for table in ((ps, mid, sign), (rnd, np.round(rng.random(300), 3), rng.integers(-1, 2, 300).astype(np.int8))):
        got, want = R.similarity_counts(*table), O.similarity_scores(*table)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_edge_table_rows_score_what_is_written_out_by_hand():
    rows, hand = SF.edge_rows(), SF.edge_hand()
    assert len(hand) == 9 and tuple(dict.fromkeys(k for k, _, _ in rows[:9])) == SF.HAND_KINDS
    for (kind, values, m), (minus, plus) in zip(rows, hand):
        for sg, want in ((-1, minus), (1, plus)):
            scores, counts = R.similarity_counts(values[None, :], np.array([m]), np.array([sg], np.int8))
            assert np.array_equal(scores, want.astype(np.int64)), (kind, m, sg)
            assert np.array_equal(counts, np.ones(SF.EDGE_LIVE, np.int64)), (kind, m, sg)


def test_same_bits_sees_the_sign_of_a_zero_and_takes_any_nan():
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    assert R.same_bits(a, a.copy()).all()
    assert R.same_bits(a, np.array([-0.0, -0.0, 0.0, 1.0], np.float32)).tolist() == [False, True, False, True]
    assert R.same_bits(np.array([-np.nan]), np.array([np.nan])).all()
    assert not R.same_bits(np.array([1.0]), np.array([np.nan])).any()
    with pytest.raises(AssertionError):
        R.same_bits(a, a.astype(np.float64))


# ------------------------------------------------------------------------------ the referee against the reference's files
@pytest.mark.parametrize("case", list(SF.SIMILARITY_CASES))
def test_similarity_report_reproduces_the_reference(golden_dir, case):
    d = os.path.join(golden_dir, "similarity_edge")
    rec = json.load(open(os.path.join(d, f"expected_{case}.json")))
    text, raised = R.similarity_report(os.path.join(d, rec["comparison"]), os.path.join(d, rec["allps"]),
                                       rec["manifest"] and os.path.join(d, rec["manifest"]))
    assert (raised and raised.__name__) == rec["raises"]
    assert_same_text(text, open(os.path.join(d, f"expected_{case}.tsv")).read())


def test_similarity_golden_inputs_are_the_fixture_modules(golden_dir, tmp_path):
    """the committed inputs are what tests/scoring_fixtures.py writes today"""
    d = os.path.join(golden_dir, "similarity_edge")
    for case in SF.SIMILARITY_CASES:
        for path in SF.write_similarity_case(tmp_path, case):
            assert path is None or open(path).read() == open(os.path.join(d, os.path.basename(path))).read(), (case, path)


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("tag,dtype", [("f32", np.float32), ("f64", np.float64)])
def test_outlier_lines_reproduce_the_reference(golden_dir, tag, dtype, cutoff):
    d = os.path.join(golden_dir, "outliers_edge")
    data = np.load(os.path.join(d, f"matrix_{tag}.npz"))
    t = SF.outlier_table(dtype, 120, 24)
    assert data["data"].dtype == dtype and R.same_bits(data["data"], t["data"]).all()
    assert data["cols"].tolist() == t["cols"].tolist() and data["rows"].tolist() == t["rows"].tolist()
    samples, null = (find_outliers.first_fields(os.path.join(d, f)) for f in ("samples.tsv", "null.tsv"))
    assert samples == t["samples"] and null == t["null"]
    want = open(os.path.join(d, f"expected_{tag}_cutoff{cutoff}.txt")).read()
    assert want
    assert_same_text(R.outlier_lines(data["data"], data["cols"], data["rows"], samples, null, cutoff), want)


# ------------------------------------------------------------------------------ findOutliers host rules
def _run_find_outliers(tmp_path, capsys, t, cutoff):
    np.savez(tmp_path / "m.npz", cols=t["cols"], rows=t["rows"], data=t["data"])
    args = argparse.Namespace(psiSPLICEDICE=str(tmp_path / "m.npz"), manifest=SF.write_manifest(tmp_path / "s.tsv", t["samples"]),
                              nullMan=SF.write_manifest(tmp_path / "n.tsv", t["null"]), outlierCutoff=cutoff, dpsiThrsh=0.1)
    capsys.readouterr()
    find_outliers.run_with(args, ctx=RefereeEngine())
    return capsys.readouterr().out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_outlier_table_has_the_rows_it_is_there_for(dtype):
    """the fixture's own conditions, from the referee's statistics in the matrix dtype"""
    t = SF.outlier_table(dtype, 200, 30)
    null_at = np.flatnonzero(np.isin(t["cols"], t["null"]))
    sample_at = np.flatnonzero(np.isin(t["cols"], t["samples"]))
    assert null_at.size == SF.N_NULL and (t["cols"] == "samp3").sum() == 2 and set(null_at) & set(sample_at)
    mean, std, n_nan = R.rowstats_rows(t["data"], null_at)
    assert n_nan[0] == 4 and n_nan[1] == 5 and n_nan[0] / SF.N_NULL == 0.2
    assert 0.00099 < std[2] < 0.001 <= std[3] < 0.00101 and std.dtype == dtype
    assert mean[4] == 0 and std[4] == 0.25 and mean[6] == 0.5 and std[6] == 0.25
    with np.errstate(all="ignore"):
        z = (t["data"][:, sample_at] - mean[:, None]) / std[:, None]
    assert {2.0, 3.0} <= set(z[4].tolist()) and 0.0 in z[5].tolist()
    for cut in (2, 3):      # z passes on both sides of |z - mean| = cut-off
        passing = z[6][z[6] >= cut]
        assert (np.abs(passing - mean[6]) >= cut).any() and (np.abs(passing - mean[6]) < cut).any()
    assert np.isnan(std[9]) and n_nan[10] == SF.N_NULL and std[11] < 0.001


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
def test_find_outliers_prints_the_reference_lines(tmp_path, capsys, dtype, cutoff):
    t = SF.outlier_table(dtype, 200, 30)
    want = R.outlier_lines(t["data"], t["cols"], t["rows"], t["samples"], t["null"], cutoff)
    assert len(want.splitlines()) >= 10
    assert_same_text(_run_find_outliers(tmp_path, capsys, t, cutoff), want)


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_find_outliers_float16_is_computed_in_float64(tmp_path, capsys, cutoff):
    """The reference computes a float16 matrix's statistics and z in float16; the command converts the matrix to float64
    first (the kernel takes float32 and float64), so it prints the lines of the converted matrix, which are not the
    reference's (find_outliers.py, module docstring)."""
    t = SF.outlier_table(np.float16, 200, 30)
    got = _run_find_outliers(tmp_path, capsys, t, cutoff)
    assert_same_text(got, R.outlier_lines(t["data"].astype(np.float64), t["cols"], t["rows"], t["samples"], t["null"], cutoff))
    assert got and got != R.outlier_lines(t["data"], t["cols"], t["rows"], t["samples"], t["null"], cutoff)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_find_hits_positions_and_empty_lists(dtype):
    t = SF.outlier_table(dtype, 200, 30)
    null_at = np.flatnonzero(np.isin(t["cols"], t["null"]))
    sample_at = np.flatnonzero(np.isin(t["cols"], t["samples"]))
    ev, pos, z, mean, std = find_outliers.find_hits(RefereeEngine(), t["data"], null_at, sample_at, 2)
    lines = R.outlier_lines(t["data"], t["cols"], t["rows"], t["samples"], t["null"], 2).splitlines()
    assert [(t["rows"][e], t["cols"][sample_at[p]]) for e, p in zip(ev, pos)] == [tuple(x.split("\t")[:2]) for x in lines]
    assert z.dtype == dtype and mean.dtype == dtype and std.dtype == dtype
    none = np.zeros(0, np.int64)
    for a, b in ((none, sample_at), (null_at, none), (none, none)):
        ev, pos = find_outliers.find_hits(RefereeEngine(), t["data"], a, b, 0)[:2]
        assert ev.size == 0 and pos.size == 0
    # the reference prints nothing either when a list selects no column
    assert R.outlier_lines(t["data"], t["cols"], t["rows"], t["samples"], ["nobody"], 0) == ""
    assert R.outlier_lines(t["data"], t["cols"], t["rows"], ["nobody"], t["null"], 0) == ""


# ------------------------------------------------------------------------------ similarity host rules
def _report(folder, case):
    """the command's own reading and writing rules around the referee's counts -> (text, exception type or None)"""
    vs, allps, manifest = SF.write_similarity_case(folder, case)
    events = similarity.significant_events(vs)
    with open(allps) as f:
        samples = f.readline().rstrip().split("\t")[1:]
        cells = [line.rstrip().split("\t") for line in f]
    ps = np.array([[float(x) for x in row[1:]] for row in cells])
    mid, sign = similarity.row_parameters([row[0] for row in cells], events)
    scores, counts = RefereeEngine().similarity(ps, mid, sign)
    out, raised = folder / "report.tsv", None
    try:
        similarity.write_report(str(out), samples, scores.tolist(), counts.tolist(),
                                similarity.sample_groups(manifest) if manifest else None)
    except ZeroDivisionError as e:
        raised = type(e)
    return out.read_text(), raised, (vs, allps, manifest)


@pytest.mark.parametrize("case", list(SF.SIMILARITY_CASES))
def test_similarity_host_rules_write_the_reference_report(tmp_path, case):
    text, raised, paths = _report(tmp_path, case)
    want, want_raised = R.similarity_report(*paths)
    assert raised is want_raised
    assert_same_text(text, want)
    if case == "nan_column":
        assert raised is ZeroDivisionError and text.endswith("z_zero\t0.000\t0\t10\n") and "a_zero" not in text
    elif case == "plain":
        lines = [x.split("\t") for x in text.splitlines()]
        assert [x[0] for x in lines[1:5]] == ["dup", "dup", "tie_b", "tie_a"]
        assert lines[1][2] == lines[2][2] and int(lines[1][3]) > int(lines[2][3])        # equal score and name: by count
        assert lines[3][1:] == lines[4][1:]                                                # equal score: by name
    elif case == "groups":
        assert "not_in_table" not in text and len(text.splitlines()) == 5
    elif case == "empty_manifest":
        assert text == R.similarity_report(paths[0], paths[1], None)[0]


def test_similarity_events_and_row_parameters(tmp_path):
    vs, allps, _ = SF.write_similarity_case(tmp_path, "plain")
    events = similarity.significant_events(vs)
    for skipped in ("ev_delta_negzero", "ev_delta_zero", "ev_p_over"):
        assert skipped not in events
    for kept in ("ev_delta_nan", "ev_p_nan", "ev_p_005", "ev_p_5e2", "ev_p_long", "ev_absent"):
        assert kept in events
    assert events["ev_twice"] == (0.35 - (-0.3) / 2, -0.3) and events["ev_keeps_first"] == (0.7 - 0.4 / 2, 0.4)
    assert events["ev_delta_inf"][0] == -np.inf and np.isnan(events["ev_median_nan"][0])
    names = ["ev_delta_nan", "ev_plain_up", "ev_plain_down", "ev_not_compared_1", "ev_delta_inf", "ev_median_inf"]
    mid, sign = similarity.row_parameters(names, events)
    assert sign.dtype == np.int8 and sign.tolist() == [0, 1, -1, 0, 1, -1]                  # a NaN delta scores nothing
    assert mid.dtype == np.float64 and mid[3] == 0 and mid[5] == np.inf
