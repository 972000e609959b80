"""Inputs of the similarity / findOutliers suites that more than one file needs (helper module, no tests in here): the
edge-value table of the similarity kernel, the hand-made comparison / PS / manifest texts of the similarity host rules
and the edge matrix of the findOutliers host rules.  tests/golden/make_golden_scoring.py writes the last two under
tests/golden/ and records what the reference makes of them."""
import numpy as np

# ------------------------------------------------------------------------------ similarity kernel: edge values
EDGE_S = 70
EDGE_LIVE = 68            # columns 68 and 69 are NaN in every row that is scored
HAND_KINDS = ("equal", "ulp", "off grid", "zeros", "inf")


def _nan_with_payload():
    return np.array([0xFFF8000000000123], np.uint64).view(np.float64)[0]


def edge_rows():
    """-> [(kind, values float64 [EDGE_LIVE], midpoint)], the kinds of HAND_KINDS first"""
    c = np.arange(EDGE_LIVE)
    m3 = 0.1 + 0.2                                             # 0.30000000000000004, not float("0.3")
    assert m3 != 0.3 and np.nextafter(0.3, 1.0) == m3
    tiny = 5e-324
    rows = [("equal", np.full(EDGE_LIVE, m3), m3),
            ("ulp", np.where(c % 2 == 0, np.nextafter(0.627, -np.inf), np.nextafter(0.627, np.inf)), 0.627),
            ("off grid", np.full(EDGE_LIVE, 0.3), m3),
            ("off grid", np.full(EDGE_LIVE, m3), 0.3),
            ("zeros", np.full(EDGE_LIVE, -0.0), 0.0),
            ("zeros", np.full(EDGE_LIVE, 0.0), -0.0),
            ("inf", np.choose(c % 3, [np.inf, -np.inf, 0.5]), 0.5),
            ("inf", np.choose(c % 3, [np.inf, -np.inf, 1e308]), np.inf),
            ("inf", np.choose(c % 3, [np.inf, -np.inf, -1e308]), -np.inf),
            ("nan midpoint", np.choose(c % 3, [0.25, np.inf, -0.0]), np.nan),
            ("subnormal", np.choose(c % 5, [0.0, tiny, 2 * tiny, 2.2e-308, -tiny]), tiny),
            ("subnormal", np.choose(c % 5, [0.0, tiny, 2 * tiny, 2.2e-308, -tiny]), 2.2250738585072014e-308),
            ("nan payload", np.where(c % 4 == 1, _nan_with_payload(), np.where(c % 4 == 3, -np.nan, 0.4)), 0.5),
            ("all nan", np.full(EDGE_LIVE, np.nan), 0.5)]
    assert [k for k, _, _ in rows[:9]] == [k for k in HAND_KINDS for _ in range({"off grid": 2, "zeros": 2, "inf": 3}.get(k, 1))]
    return rows


def edge_hand():
    """what the rows of HAND_KINDS score, written out by hand: one (scored under sign -1, scored under sign +1) pair of
    bool [EDGE_LIVE] per row of edge_rows(), in its order; every one of these cells is counted"""
    c = np.arange(EDGE_LIVE)
    none, every = np.zeros(EDGE_LIVE, bool), np.ones(EDGE_LIVE, bool)
    return [(none, none),                                      # equal in every bit: neither < nor >
            (c % 2 == 0, c % 2 == 1),                          # one ulp below / above
            (every, none),                                     # 0.3 < 0.1 + 0.2
            (none, every),                                     # 0.1 + 0.2 > 0.3
            (none, none), (none, none),                        # -0.0 == +0.0
            (c % 3 == 1, c % 3 == 0),                          # -inf < 0.5 < +inf, 0.5 == 0.5
            (c % 3 != 0, none),                                # midpoint +inf: all but +inf are below, nothing above
            (none, c % 3 != 1)]                                # midpoint -inf: all but -inf are above


def edge_table():
    """-> (ps float64 [n, EDGE_S], mid, sign int8, kind of every row): each row of edge_rows() under sign -1 and +1,
    then the same values under sign 0 with the last two columns filled in (so they are NaN on the scored rows only)"""
    ps, mid, sign, kinds = [], [], [], []
    for kind, values, m in edge_rows():
        for sg in (-1, 1, 0):
            ps.append(np.r_[values, [0.9, 0.1] if sg == 0 else [np.nan, np.nan]])
            mid.append(m)
            sign.append(sg)
            kinds.append(kind)
    return np.array(ps), np.array(mid), np.array(sign, np.int8), kinds


# ------------------------------------------------------------------------------ similarity host rules: hand-made texts
VS_HEADER = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected\n"
# event, median1, delta, p-value (the other columns are not read)
VS_ROWS = [("ev_plain_up", "0.6", "0.2", "0.01"),
           ("ev_plain_down", "0.4", "-0.2", "1e-9"),
           ("ev_delta_nan", "0.5", "nan", "0.01"),             # kept by the reader, scored and counted by nobody
           ("ev_delta_negzero", "0.5", "-0.0", "0.01"),        # skipped
           ("ev_delta_zero", "0.5", "0", "0.01"),              # skipped
           ("ev_delta_inf", "0.5", "inf", "0.01"),             # midpoint -inf, every value scores
           ("ev_p_nan", "0.6", "0.2", "nan"),                  # kept: nan > 0.05 is false
           ("ev_p_005", "0.4", "-0.2", "0.05"),
           ("ev_p_5e2", "0.55", "0.1", "5e-2"),
           ("ev_p_long", "0.45", "-0.1", "0.050000000000000001"),       # parses to 0.05: kept
           ("ev_p_over", "0.6", "0.2", "0.05000000000000001"),          # one ulp above: skipped
           ("ev_median_nan", "nan", "0.2", "0.01"),            # midpoint NaN: counted, never scored
           ("ev_median_inf", "inf", "-0.2", "0.01"),           # midpoint +inf: every finite value scores
           ("ev_twice", "0.65", "0.3", "0.01"),
           ("ev_keeps_first", "0.7", "0.4", "0.01"),
           ("ev_absent", "0.5", "0.2", "0.01"),                # no line in the PS table
           ("ev_twice", "0.35", "-0.3", "0.02"),               # the later line wins
           ("ev_keeps_first", "0.3", "-0.4", "0.9")]           # skipped by p: the earlier line stays
PS_SAMPLES = ["s_hi", "tie_a", "tie_b", "dup", "dup", "z_zero", "m_nan", "a_zero", "s_lo", "s_mix"]
NAN_COLUMN = PS_SAMPLES.index("m_nan")
PS_EVENTS = ["ev_plain_up", "ev_not_compared_1", "ev_plain_down", "ev_delta_nan", "ev_delta_negzero", "ev_delta_zero",
             "ev_delta_inf", "ev_p_nan", "ev_p_005", "ev_plain_up", "ev_p_5e2", "ev_p_long", "ev_p_over", "ev_median_nan",
             "ev_median_inf", "ev_twice", "ev_not_compared_2", "ev_keeps_first"]       # ev_plain_up is on two lines


def vs_text():
    return VS_HEADER + "".join(f"{e}\t0.5\t0.5\t{m1}\t0.5\t{d}\t{p}\t0.5\n" for e, m1, d, p in VS_ROWS)


def ps_text(nan_column=False):
    """the PS table; every midpoint but the special ones is 0.5 (or the float next to it).  s_hi sides with every event,
    s_lo against; tie_a / tie_b are equal cell for cell; the two `dup` columns score alike on different counts;
    z_zero / a_zero never score; m_nan is NaN on every line when nan_column, a copy of s_mix otherwise"""
    up = {"ev_plain_up": 1, "ev_plain_down": 0, "ev_delta_inf": 1, "ev_p_nan": 1, "ev_p_005": 0, "ev_p_5e2": 1, "ev_p_long": 0,
          "ev_median_nan": 1, "ev_median_inf": 0, "ev_twice": 0, "ev_keeps_first": 1}
    rng = np.random.default_rng(5)
    lines = ["cluster\t" + "\t".join(PS_SAMPLES) + "\n"]
    for k, ev in enumerate(PS_EVENTS):
        with_it, against = ("0.812", "0.107") if up.get(ev, 1) else ("0.107", "0.812")
        mix = rng.choice(["0.5", "0.499", "0.501", "nan", "0.000", "1.000"])
        tie = rng.choice([with_it, against, "nan", "0.5"])
        never = "nan" if ev in ("ev_delta_inf", "ev_median_inf") else against      # (these two score any finite value)
        dup1 = "nan" if ev == "ev_p_005" else with_it if k % 2 else against
        dup2 = against if ev == "ev_p_005" else dup1
        row = [with_it, tie, tie, dup1, dup2, never, "nan" if nan_column else mix, never, against, mix]
        lines.append(ev + "\t" + "\t".join(row) + "\n")
    return "".join(lines)


MANIFEST_SUBSET = "".join(f"{n}\t/data/{n}.bam\t{g1}\t{g2}\n" for n, g1, g2 in
                          [("s_lo", "tumour", "batch1"), ("dup", "normal", "batch2"), ("not_in_table", "tumour", "batch1"),
                           ("tie_b", "tumour", "batch2"), ("s_hi", "normal", "batch1")])
# name -> (PS table with the all-NaN column, manifest text or None)
SIMILARITY_CASES = {"plain": (False, None), "groups": (False, MANIFEST_SUBSET), "empty_manifest": (False, ""),
                    "nan_column": (True, None), "nan_column_groups": (True, MANIFEST_SUBSET)}


def write_similarity_case(folder, case):
    """writes the inputs of one case into `folder` (a pathlib.Path) -> (comparison, PS table, manifest or None) paths"""
    nan_column, manifest = SIMILARITY_CASES[case]
    vs, ps = folder / "in_vs.tsv", folder / ("in_allPS_nan_column.tsv" if nan_column else "in_allPS.tsv")
    vs.write_text(vs_text())
    ps.write_text(ps_text(nan_column))
    if manifest is None:
        return str(vs), str(ps), None
    m = folder / ("manifest_empty.tsv" if manifest == "" else "manifest_subset.tsv")
    m.write_text(manifest)
    return str(vs), str(ps), str(m)


# ------------------------------------------------------------------------------ findOutliers host rules: edge matrix
N_NULL = 20               # null columns: 20 % of them is exactly 4


def outlier_table(dtype, n, s, seed=3):
    """-> dict(data [n, s] of dtype, cols, rows, samples, null, kind: row -> what the row is there for).
    Columns: samp0 .. samp<s-2>, and the last column is named samp3 again.  The null list names samp0 .. samp18 (N_NULL
    columns with the repeat), the sample list samp15 .. samp<s-2>, samp3 (both lists, both columns) and a name the
    table lacks.  Integer tables hold 0 / 1 and no NaN; the float rows are described where they are made."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    cols = np.array([f"samp{j}" for j in range(s - 1)] + ["samp3"])
    rows = np.array([f"chr1:{1000 + 10 * i}-{2000 + 10 * i}:+" for i in range(n)])
    null = [f"samp{j}" for j in range(N_NULL - 1)]
    samples = [f"samp{j}" for j in range(15, s - 1)] + ["samp3", "not_in_table"]
    null_at = np.flatnonzero(np.isin(cols, null))
    only_sample = np.setdiff1d(np.flatnonzero(np.isin(cols, samples)), null_at)      # columns free to hold anything
    assert null_at.size == N_NULL and only_sample.size >= 4
    kind = {}
    if dtype.kind == "i":
        data = (rng.random((n, s)) < 0.12).astype(dtype)
        data[:, only_sample] = rng.random((n, only_sample.size)) < 0.5
        data[0, null_at] = 0                                   # std 0: skipped
        data[1, null_at] = 1
        kind.update({0: "constant 0", 1: "constant 1"})
        return dict(data=data, cols=cols, rows=rows, samples=samples, null=null, kind=kind)
    data = np.round(0.5 + 0.05 * rng.standard_normal((n, s)), 3)
    data[rng.random((n, s)) < 0.06] = np.nan
    spike = rng.random((n, s)) < 0.15
    data[spike] = np.round(data[spike] + 0.25, 3)
    half = np.where(np.arange(N_NULL) % 2 == 0, -1.0, 1.0)

    def put(r, what, null_vals, sample_vals=None):
        kind[r] = what
        data[r, null_at] = null_vals
        if sample_vals is not None:
            data[r, only_sample[:len(sample_vals)]] = sample_vals

    base = np.round(0.5 + 0.05 * rng.standard_normal(N_NULL), 3)
    with_nan = lambda k: np.r_[np.full(k, np.nan), base[k:]]                         # noqa: E731
    put(0, "4 of 20 null values NaN: kept", with_nan(4), [0.95, 0.9, 0.1, np.nan])
    put(1, "5 of 20 null values NaN: skipped", with_nan(5), [0.95, 0.9, 0.1, np.nan])
    put(2, "null std just under 0.001", 0.5 + 0.000999 * half, [0.6, 0.51, 0.4, 0.503])
    put(3, "null std just over 0.001", 0.5 + 0.001001 * half, [0.6, 0.51, 0.4, 0.503])
    # mean 0, std 0.25, all exact: z = 4 v
    put(4, "z at the cut-offs", 0.25 * half, [0.5, np.nextafter(dtype.type(0.5), dtype.type(0)), 0.75,
                                              np.nextafter(dtype.type(0.75), dtype.type(0))])
    put(5, "z of 0", 0.25 * half, [0.0, -0.0, np.nextafter(dtype.type(0), dtype.type(-1)), 0.25])
    # mean 0.5, std 0.25, all exact: z = 4 v - 2, printed when also |z - 0.5| >= cut-off
    put(6, "|z - mean| around 2 and 3", 0.5 + 0.25 * half, [1.125, np.nextafter(dtype.type(1.125), dtype.type(0)), 1.375,
                                                           np.nextafter(dtype.type(1.375), dtype.type(0))])
    put(7, "z passes, |z - mean| does not", 0.5 + 0.25 * half, [1.0, 1.25, 1.0625, 1.3125])
    put(8, "NaN and inf among the sample values", base, [np.nan, np.inf, -np.inf, 0.9])
    put(9, "inf among the null values", np.r_[np.inf, base[1:]], [0.9, np.inf, 0.1, np.nan])
    put(10, "all null values NaN", np.full(N_NULL, np.nan), [0.9, 0.5, 0.1, np.nan])
    put(11, "constant null values", np.full(N_NULL, 0.1), [0.9, 0.5, 0.1, np.nan])
    with np.errstate(over="ignore"):
        return dict(data=data.astype(dtype), cols=cols, rows=rows, samples=samples, null=null, kind=kind)


def write_manifest(path, names):
    with open(path, "w") as f:
        f.write("".join(f"{x}\t/data/{x}.bam\n" for x in names))
    return str(path)
