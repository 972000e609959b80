"""`splicedice compare_sample_sets`: two-group rank-sum test per junction of an `_allPS.tsv`.

Drop-in for splicedice/compareSampleSets.py (add_parser :124-159, run_with :163-270): same
flags, same `<3 samples` exit, same output columns
`event mean1 mean2 median1 median2 delta p-value corrected` (+ gene/overlapping/transcript_id
with -a GTF), values printed as numpy float32 / float64 scalars.

One flag the reference lacks: `-mx FILE [FILE ...]` names the third and later sample sets; the test is then the
Kruskal-Wallis H test across all k sets (sdice_kruskal) and the columns are
`event mean1..meank median1..mediank delta H p-value corrected`.

Another one: `--paired` pairs line i of -m1 with line i of -m2 (matched samples: tumour / normal of one patient, before /
after) and the test is the Wilcoxon signed-rank test of the pairs (sdice_signedrank); the output columns are the
two-set ones.

A third: `--exact` replaces the normal approximation of the p-value by the exact conditional (permutation) value on the
rows small enough for it -- at most 32 kept values in the two-set test, at most 31 non-zero differences with `--paired`
(sdice_ranksum_exact, sdice_signedrank_exact); larger rows keep the asymptotic p-value, as R's wilcox.test does.  Same
columns; not with -mx.

A fourth: `--strata FILE` (lines `sample<TAB>label`) names the batch (centre, library prep, sex, ...) of every sample
and the test becomes van Elteren's stratified rank-sum test (sdice_ranksum_strata): values are ranked inside their batch
only and the batches' rank-sum deviations are added with weights 1 / (N_h + 1).  Same columns; not with --paired, -mx or
--exact.  Unlike the plain test its variance carries the tie correction.

A fifth: `--trend` (with -mx) takes the sets as ORDERED -- dose levels, time points, stages: -m1 < -m2 < the -mx files in
the order given -- and the test becomes the Jonckheere-Terpstra trend test (sdice_jonckheere): z > 0 where the PS rises
along the order, two-sided asymptotic p.  The columns are the -mx ones with `z` where `H` stood; not with --paired, --exact
or --strata.

A sixth: `--ks` replaces the rank-sum test by the two-sample Kolmogorov-Smirnov test (sdice_ks), which answers to any
difference between the two distributions -- a junction switched on in part of a set, a bimodal set with the other's median
-- where the rank-sum statistic and `delta` stay near 0.  The columns gain `D` (the KS statistic) before `p-value`; with
`--exact` the rows that keep at most 32 values get the exact conditional p-value.  Not with --paired, -mx, --strata or
--trend.

A seventh: `--shift` adds the size of the difference that belongs to the rank-sum test: the Hodges-Lehmann shift (the median
of all pairwise differences set 1 - set 2) and its distribution-free confidence interval at `--conf LEVEL` (0.95), two
order statistics of the same differences (sdice_shift; R's wilcox.test(conf.int = TRUE) reports the same interval).  The
test stays the rank-sum test (the exact one with `--exact`) and every other cell is what it is without the flag; the table
gains `shift shift_lo shift_hi` before `p-value`.  Not with --paired, -mx, --trend, --ks or --strata.

An eighth: `--posthoc` (with -mx) answers WHICH sets differ: Dunn's test for every pair of sets, taken from the joint ranking
of the Kruskal-Wallis test in the same pass (sdice_kruskal_dunn).  Every -mx column stays where it is and what it is; between
`H` and `p-value` the table gains, per pair of sets i < j in the order 1v2, 1v3, .., `z{i}v{j}` (> 0 where set i ranks above
set j) and `padj{i}v{j}`, the pair's two-sided p-value after Holm's step-down correction over the pairs of the row.  At most
11 sets; not with --trend.

A ninth: `--repeated` (with -mx) takes the sets as MATCHED -- line i of every manifest is the same subject -- and the test
becomes Friedman's test (sdice_friedman), ranks taken inside each subject's block of k values, blocks with a missing value
dropped; the columns are the -mx ones with `Q W` where `H` stood.  With `--trend` the sets are ordered as well and the test
is Page's L test (sdice_page) with `z` in that place.  Not with --paired, --exact, --strata, --ks, --shift or --posthoc
(DESIGN.md section 7).

A tenth: `--pseudomedian` (with --paired) adds the size of the difference that belongs to the signed-rank test: the paired
Hodges-Lehmann estimate, the median of the Walsh averages (d_i + d_j) / 2, i <= j, of the within-pair differences -- R prints
it as "(pseudo)median" -- and its distribution-free confidence interval at `--conf LEVEL` (0.95), two order statistics of the
same averages (sdice_walsh; the interval of R's wilcox.test(paired = TRUE, conf.int = TRUE) with the rank from the normal
approximation at every size).  `delta`, the difference of the two sets' medians, is not that quantity: it can be 0, or of the opposite sign, on a
row where every pair moves the same way.  The test stays the signed-rank test (the exact one with `--exact`) and every other
cell is what it is without the flag; the table gains `shift shift_lo shift_hi` before `p-value`.

On the GPU: the per-row loop :216-232 (NaN drop, <3 skip, scipy ranksums, medians, means)
-> sdice_ranksum; multipletests(..., "fdr_bh") :235 -> sdice_bh over the tested rows.
The GTF annotation columns are host string work, as in the reference.
"""
import argparse
import sys
import typing

import numpy as np

from . import _cli
from ._cli import annotation_suffixes, read_annotation, read_ps_table, samples_from_manifest, table_header_names  # noqa: F401
from .engine import (DUNN_MAX_SETS, FRIEDMAN_FIELDS, JONCKHEERE_FIELDS, KRUSKAL_DUNN_FIELDS, KRUSKAL_FIELDS, KS_FIELDS,
                     PAGE_FIELDS, RANKSUM_EXACT_FIELDS, RANKSUM_FIELDS, SHIFT_FIELDS, Context, dunn_pairs, field_shapes)

MAX_STRATA = 64                     # strata a call accepts (include/sdice.h)


def row_test(ctx, paired, exact, dev=False):
    """the context's call for the chosen test: ranksum / signedrank, their _exact forms with --exact, _dev on resident data"""
    return getattr(ctx, ("signedrank" if paired else "ranksum") + ("_exact" if exact else "") + ("_dev" if dev else ""))


def column_indices(group, cols):
    """Columns of the table that belong to the group, in TABLE order (compareSampleSets.py:96-102)."""
    return np.nonzero(np.isin(cols, group))[0].astype(np.int32)


def tested(ctx, matrix, fields, inputs, dev, host=None, k=None):
    """The pipeline of every test on the HIP engine, stage by stage: table and `inputs` (name -> (host array, dtype)) up,
    dev(d_in, d_out) + BH over the tested rows on resident vectors, per-row results down (the host calls do the same
    steps inside two calls) -> (kept row indices, dict of the fields at those rows and `corrected`; the `exact` marks stay
    behind).  A table without rows: host() checks the arguments as the device call would and every result is empty."""
    n = matrix.shape[0]
    if n:
        keep, r = _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), **inputs), field_shapes(fields, n, k), dev)
    else:
        keep = np.zeros(0, np.int64)
        r = {name: v[..., :0] for name, v in host().items() if name != "tested"}
        r["corrected"] = np.zeros(0)
    r.pop("exact", None)
    return keep, r


# --shift: the fields of the shift call as they ride beside the rank-sum ones in one device pass (its own `tested` and
# the rank stay behind), and the three that reach the table
SHIFT_RIDERS = [("shift_" + f[0], f[1]) for f in SHIFT_FIELDS if f[0] != "shift"] + [("shift", np.float64)]
SHIFT_COLUMNS = ("shift", "shift_lo", "shift_hi")


def compare(matrix, g1_idx, g2_idx, ctx, paired=False, exact=False, conf=None):
    """-> (kept row indices, dict of compacted per-row results incl. BH-corrected p).  paired: g1_idx[q] and g2_idx[q]
    are the columns of pair q and the test is the signed-rank test.  exact: exact p-values on the small rows (BH runs
    over the mixed p vector).  conf: the level of --shift or, when paired, of --pseudomedian; the shift call (paired: the
    walsh call) then reads the same resident table in the same pass and the results gain SHIFT_COLUMNS."""
    if hasattr(ctx, "ranksum_dev") and matrix.shape[0]:
        test = row_test(ctx, paired, exact, dev=True)
        estimate = ctx.walsh_resident if paired else ctx.shift_dev

        def launch(d, out):
            test(d["ps"], d["g1"], d["g2"], out)
            if conf is not None:
                estimate(d["ps"], d["g1"], d["g2"], {f[0]: out["shift" if f[0] == "shift" else "shift_" + f[0]]
                                                     for f in SHIFT_FIELDS}, conf)

        keep, r = tested(ctx, matrix, (RANKSUM_EXACT_FIELDS if exact else RANKSUM_FIELDS) + (SHIFT_RIDERS if conf is not None else []),
                         dict(g1=(g1_idx, np.int32), g2=(g2_idx, np.int32)), launch)
        for name in ("shift_tested", "shift_rank"):
            r.pop(name, None)
        return keep, r
    res = row_test(ctx, paired, exact)(matrix, g1_idx, g2_idx)
    keep = np.flatnonzero(res["tested"])
    out = {k: res[k][keep] for k in ("p", "med1", "med2", "mean1", "mean2", "delta")}
    if conf is not None:
        sh = (ctx.walsh if paired else ctx.shift)(matrix, g1_idx, g2_idx, conf)
        out.update(shift=sh["shift"][keep], shift_lo=sh["lo"][keep], shift_hi=sh["hi"][keep])
    out["corrected"] = ctx.bh(out["p"]) if keep.size else np.zeros(0)
    return keep, out


def compare_sharded(matrix, g1_idx, g2_idx, ctx, L, paired=False, exact=False):
    """compare() with the table rows cut into one block per rank (rows are independent here): every rank tests its
    block, the per-row statistics cross the ranks as ONE packed block in ONE all-gather (distributed.stat_layout, padded to
    the longest block), rank 0 corrects.  exact: the _exact call; its `exact` marks are not packed."""
    from . import distributed
    n = matrix.shape[0]
    lo, hi = L.row_block(n)
    rows_of = [b - a for a, b in (L.row_block(n, r) for r in range(L.world))]
    maxk = distributed.longest(rows_of)
    res = row_test(ctx, paired, exact)(np.ascontiguousarray(matrix[lo:hi]), g1_idx, g2_idx)
    stats = {k: distributed.pad_rows(np.asarray(res[k], dt), maxk) for k, dt in RANKSUM_FIELDS}
    gathered = L.comm(ctx).allgather(distributed.pack_stats_host(stats, maxk))
    host = distributed.unpack_stats_host(gathered, maxk, L.world)
    full = {k: distributed.drop_padding(host[k], rows_of, maxk) for k, _ in RANKSUM_FIELDS if k != "z"}
    keep = np.flatnonzero(full.pop("tested"))
    out = {k: v[keep] for k, v in full.items()}
    out["corrected"] = ctx.bh(out["p"]) if (keep.size and L.root) else np.zeros(keep.size)
    return keep, out


def add_parser(parser):
    parser.add_argument("--psiSPLICEDICE", type=str, required=True,
                        help="Compressed NPZ formatted PSI matrix from 'splicedice quant'.")
    parser.add_argument("-m1", "--manifest1", type=str, required=True,
                        help="Manifest containing samples for sample set group1")
    parser.add_argument("-m2", "--manifest2", type=str, required=True,
                        help="Manifest containing samples for sample set group2")
    parser.add_argument("-mx", "--moreManifests", type=str, nargs="+", required=False, default=None, metavar="FILE",
                        help="Manifests of the third and later sample sets: the rank-sum test becomes the Kruskal-Wallis "
                             "H test across all sets (not part of the reference)")
    parser.add_argument("--paired", action="store_true",
                        help="Matched samples: line i of -m1 is paired with line i of -m2 (MANIFEST order, not the "
                             "table order of the unpaired test) and the test is the Wilcoxon signed-rank test of the "
                             "pairs; same output columns (not part of the reference)")
    parser.add_argument("--exact", action="store_true",
                        help="Exact p-values for small sample sets: the conditional permutation distribution given the "
                             "row's ties instead of the normal approximation, on rows that keep at most 32 values (with "
                             "--paired: at most 31 non-zero differences).  Rows above these limits keep the asymptotic "
                             "p-value, as R's wilcox.test does.  Not with -mx (not part of the reference)")
    parser.add_argument("--strata", type=str, required=False, default=None, metavar="FILE",
                        help="Batch labels, one `sample<TAB>label` per line: the test becomes van Elteren's stratified "
                             "rank-sum test -- values are ranked inside their batch only and the batches are combined "
                             "with weights 1/(N_h+1).  Every sample of -m1 / -m2 in the table needs exactly one label, at "
                             "most 64 distinct labels; a batch with samples of one set only contributes nothing.  The "
                             "variance carries the tie correction, which the plain test (scipy ranksums) lacks: with one "
                             "batch the p-value is mannwhitneyu(use_continuity=False, method='asymptotic'), equal to "
                             "the plain one only on rows without ties.  Not with --paired, -mx or --exact (not part of "
                             "the reference)")
    parser.add_argument("--trend", action="store_true",
                        help="With -mx: the sets are ORDERED (dose levels, time points, stages), -m1 < -m2 < the -mx files "
                             "in the order given, and the test becomes the Jonckheere-Terpstra trend test: z > 0 where the "
                             "PS rises along that order, z < 0 where it falls; the table carries z where the -mx table "
                             "carries H.  The two-sided p-value is asymptotic only (normal approximation with the "
                             "tie-corrected variance, no exact form).  Not with --paired, --exact or --strata (not part of "
                             "the reference)")
    parser.add_argument("--posthoc", action="store_true",
                        help="With -mx: which sets differ -- Dunn's test for every pair of sets, from the joint ranking of "
                             "the Kruskal-Wallis test.  Between H and p-value the table gains, per pair of sets i < j (1v2, "
                             "1v3, ..), the columns z{i}v{j} (> 0 where set i ranks above set j, tie-corrected, no "
                             "continuity correction) and padj{i}v{j}, the pair's two-sided p-value after Holm's step-down "
                             "correction over the pairs of the row (not across rows: `corrected` stays the Benjamini-"
                             "Hochberg value of the H test).  At most 11 sets.  Not with --trend (not part of the "
                             "reference)")
    parser.add_argument("--repeated", action="store_true",
                        help="With -mx: MATCHED sets -- the same subjects in every set (time points, normal / primary / "
                             "metastasis of one patient, one cell line under several doses): line i of -m1, -m2 and every "
                             "-mx file is the same subject (MANIFEST order, as with --paired) and the test is Friedman's "
                             "test, ranks taken inside each subject's values; a subject with a missing value in any set "
                             "is left out of the row, 3 complete subjects are needed.  The table carries Q and W "
                             "(Kendall's coefficient of concordance) where the -mx table carries H; the p-value is the "
                             "chi-square approximation.  With --trend the sets are ORDERED and the test is Page's L "
                             "test: the table carries z (> 0 where the PS rises along the order; the variance is "
                             "conditional on the row's ties), the p-value is two-sided and asymptotic.  Not with "
                             "--paired, --exact, --strata, --ks, --shift or --posthoc (not part of the reference)")
    parser.add_argument("--ks", action="store_true",
                        help="The two-sample Kolmogorov-Smirnov test instead of the rank-sum test: it answers to any "
                             "difference between the two distributions (a junction switched on in part of a set, a "
                             "bimodal set), not to a shift alone.  The table gains the column D (the KS statistic, 0..1) "
                             "before p-value.  The p-value is Kolmogorov's limiting distribution "
                             "(scipy.special.kolmogorov, no finite-n correction); with --exact the rows that keep at "
                             "most 32 values get the exact conditional p-value given their ties (R's ks.test(exact = "
                             "TRUE)).  Not with --paired, -mx, --strata or --trend (not part of the reference)")
    parser.add_argument("--shift", action="store_true",
                        help="Add the Hodges-Lehmann shift of set 1 against set 2 -- the median of all pairwise differences, "
                             "the estimate that belongs to the rank-sum test -- and its distribution-free confidence "
                             "interval (two order statistics of the same differences; R's wilcox.test(conf.int = TRUE)): "
                             "the table gains the columns shift, shift_lo and shift_hi before p-value, every other column "
                             "is what it is without the flag (with --exact: the exact p-values).  On rows of 3-decimal PS "
                             "values the differences are whole thousandths.  With small sets the interval is the whole "
                             "range of the differences and the level is not reached (3 v 3 at 95 %%).  Not with --paired, "
                             "-mx, --trend, --ks or --strata (not part of the reference)")
    parser.add_argument("--conf", type=float, required=False, default=None, metavar="LEVEL",
                        help="With --shift or --pseudomedian: the confidence level of the interval, 0 < LEVEL < 1 (default "
                             "0.95)")
    parser.add_argument("--pseudomedian", action="store_true",
                        help="With --paired: add the paired Hodges-Lehmann estimate of the within-pair change -- the median "
                             "of the Walsh averages (d_i + d_j) / 2, i <= j, of the pairs' differences d = set 1 - set 2, "
                             "which R prints as (pseudo)median; the estimate that belongs to the signed-rank test -- and "
                             "its distribution-free confidence interval at --conf LEVEL (0.95; two order statistics of "
                             "the same averages): the table gains the columns shift, shift_lo and shift_hi before "
                             "p-value, every other column is what it is without the flag (with --exact: the exact "
                             "p-values).  Pairs with equal values count here (the test drops them).  On rows of "
                             "3-decimal PS values the averages are whole half thousandths.  With few pairs the interval "
                             "is the whole range of the averages and the level is not reached (up to 6 pairs at 95 %%).  "
                             "The rank of the interval's ends is the normal approximation without a tie correction at "
                             "every size (not part of the reference)")
    parser.add_argument("-a", "--annotation", type=str, required=False, default="",
                        help="Optional GTF file to label known splice junctions and genes")
    parser.add_argument("-o", "--outputFile", type=str, required=True,
                        help="Output filename for tab-separated table")


def strata_columns(g1, g2, header_names, labels):
    """--strata: the manifests' sample lists, the table's column names and the label file's sample -> [labels] ->
    (g1_idx, g2_idx in table order, strat1, strat2 int32 dense ids by first appearance, the number of strata); prints why
    and exits with status 1 when a selected column has no label or more than one, sits in both sets, or the selected
    columns carry more than MAX_STRATA labels"""
    from .engine import strata_ids
    cols = np.array(header_names)
    g1_idx, g2_idx = column_indices(g1, cols), column_indices(g2, cols)
    both = np.intersect1d(g1_idx, g2_idx)
    if both.size:
        refuse_strata(f"sample {header_names[both[0]]!r} is in both manifests; a column belongs to one set here")
    chosen = []
    for j in np.concatenate([g1_idx, g2_idx]).tolist():
        found = labels.get(header_names[j], [])
        if len(found) != 1:
            refuse_strata(f"sample {header_names[j]!r} " + ("has no label in the strata file" if not found else
                                                           f"has {len(found)} lines in the strata file"))
        chosen.append(found[0])
    ids, names = strata_ids(chosen)
    if len(names) > MAX_STRATA:
        refuse_strata(f"{len(names)} distinct labels among the selected samples, at most {MAX_STRATA} strata are supported")
    return g1_idx, g2_idx, ids[:g1_idx.size].copy(), ids[g1_idx.size:].copy(), len(names)


def paired_columns(g1, g2, header_names):
    """--paired: the manifests' sample lists and the table's column names -> (a, b) int32 column indices, pair q =
    (a[q], b[q]) in manifest order; prints why and exits with status 1 when the lists cannot be paired"""
    if len(g1) != len(g2):
        refuse(f"the manifests differ in length ({len(g1)} and {len(g2)} samples); line i of -m1 is paired with line i of -m2")
    if len(g1) < 3:
        refuse(f"cannot conduct the signed-rank test with fewer than 3 pairs (got {len(g1)})")
    seen = set()
    for name in g1 + g2:
        if name in seen:
            refuse(f"sample {name!r} appears twice in the manifests; a sample belongs to one pair only")
        seen.add(name)
    idx = _cli.columns_in_header(g1 + g2, header_names, refuse)
    return idx[:len(g1)], idx[len(g1):]


class Test(typing.NamedTuple):
    """One row per flag that changes the test.  The refusals: `needs` another flag (flag, why), or one of `needs_or` in its
    place; `conflicts`, the ordered (other flag, why) it cannot be combined with; `multi_rank`, why it does not run under the multi-rank launcher.  A row
    that replaces the rank-sum pipeline (--exact and --paired are forms of it: compare()) says how: `fields`, the
    engine's table of its _dev call; sel -> `inputs`, the device inputs beside the table; (ctx, sel) -> `dev`, the launch
    on them; (ctx, matrix, sel) -> `host`, the host call; sel -> `k`, the number of sets of its per-set fields.  `stat`: the
    (header cell, result key) of every column the row adds between delta and p-value, or a function of the number of
    sets that returns them; a result key is a field's name or (name, i) for row i of a per-set or per-pair field."""
    flag: str
    conflicts: tuple = ()
    needs: tuple = None
    needs_or: tuple = ()
    multi_rank: str = None
    fields: list = None
    inputs: typing.Callable = None
    dev: typing.Callable = None
    host: typing.Callable = None
    k: typing.Callable = lambda sel: None
    stat: tuple = ()

    def refuse(self, why):
        _cli.refusal(f"compare_sample_sets {self.flag.split('/')[0]}")(why)

    def columns(self, k):
        """`stat` for k sets"""
        return tuple(self.stat(k)) if callable(self.stat) else self.stat


def _multi_rank(flag, carries):
    return (f"compare_sample_sets: {flag} is not available under the multi-rank launcher ({carries}); "
            f"run it in one process.")


def _two_sets(sel):
    return dict(g1=(sel.g1_idx, np.int32), g2=(sel.g2_idx, np.int32))


def _k_sets(test):
    """the rest of a row over k >= 3 sets; test: the engine's name of the call (`<test>_dev` on resident data)"""
    return dict(inputs=lambda sel: dict(cols=(sel.cols, np.int32)), k=lambda sel: len(sel.set_idx),
                dev=lambda ctx, sel: lambda d, out: getattr(ctx, test + "_dev")(d["ps"], d["cols"], sel.set_ptr, out),
                host=lambda ctx, matrix, sel: getattr(ctx, test)(matrix, sel.set_idx))


def _dunn_columns(k):
    """H, then z and the Holm-adjusted p of every pair of sets in the engine's order, sets numbered from 1"""
    yield "H", "h"
    for q, (i, j) in enumerate(dunn_pairs(k)):
        yield f"z{i + 1}v{j + 1}", ("pair_z", q)
        yield f"padj{i + 1}v{j + 1}", ("pair_padj", q)


def repeated_columns(groups, header_names):
    """--repeated: the manifests' sample lists (set by set) and the table's column names -> one int32 column index vector per
    set in MANIFEST order, entry q of every vector the same subject; prints why and exits with status 1 when the lists are
    not one line per subject"""
    refuse = BY_FLAG[REPEATED].refuse
    if len({len(g) for g in groups}) > 1:
        refuse(f"the manifests differ in length ({', '.join(str(len(g)) for g in groups)} samples); line i of every "
               f"manifest is the same subject")
    if len(groups[0]) < 3:
        refuse(f"cannot conduct Friedman's test with fewer than 3 subjects (got {len(groups[0])})")
    seen = set()
    for name in (x for g in groups for x in g):
        if name in seen:
            refuse(f"sample {name!r} appears twice in the manifests; a sample belongs to one set and one subject only")
        seen.add(name)
    idx = _cli.columns_in_header([x for g in groups for x in g], header_names, refuse)
    return [v.copy() for v in np.split(idx, len(groups))]


def _matched_sets(test):
    """the rest of a row over k matched sets; test: the engine's name of the call (`<test>_resident` on resident data)"""
    return dict(inputs=lambda sel: dict(cols=(sel.cols, np.int32)), k=lambda sel: len(sel.set_idx),
                dev=lambda ctx, sel: lambda d, out: getattr(ctx, test + "_resident")(d["ps"], d["cols"], len(sel.set_idx), out),
                host=lambda ctx, matrix, sel: getattr(ctx, test)(matrix, sel.set_idx))


PAIRED, EXACT, STRATA, TREND, KS, MX = "--paired", "--exact", "--strata", "--trend", "--ks", "-mx/--moreManifests"
SHIFT, CONF, POSTHOC, REPEATED, PSEUDOMEDIAN = "--shift", "--conf", "--posthoc", "--repeated", "--pseudomedian"
# in the order the refusals are made; the first selected row with a pipeline is the test that runs
TESTS = (
    # k matched sets: Friedman's test per junction (with --trend: Page's test, PAGE below).  First, so that it, not the
    # --trend / -mx rows, is the test that runs
    Test(REPEATED, needs=(MX, "two matched sets are the signed-rank test: --paired"),
         conflicts=((PAIRED, "the signed-rank test compares two matched sets; this test compares three or more"),
                    (EXACT, "there is no exact Friedman test here"),
                    (STRATA, "the subjects are the blocks already; there is no stratified form"),
                    (KS, "the Kolmogorov-Smirnov test compares two independent sets"),
                    (SHIFT, "the shift is an estimate between two independent sets"),
                    (POSTHOC, "there is no post-hoc test of matched sets here")),
         multi_rank=_multi_rank(REPEATED, "the packed all-gather carries the two-set fields only"),
         fields=FRIEDMAN_FIELDS, stat=(("Q", "q"), ("W", "w")), **_matched_sets("friedman")),
    Test(CONF, needs=(SHIFT, "it is the level of the shift's confidence interval"), needs_or=(PSEUDOMEDIAN,)),
    # (keeps the rank-sum pipeline, as --exact does: compare() adds the shift call to the same pass)
    Test(SHIFT, conflicts=((PAIRED, "the paired estimate is the median of the Walsh averages, which is not offered"),
                           (MX, "the shift is an estimate between two sets"),
                           (TREND, "the shift is an estimate between two sets"),
                           (KS, "the shift belongs to the rank-sum test"),
                           (STRATA, "there is no stratified shift here")),
         multi_rank=_multi_rank(SHIFT, "the packed all-gather carries the rank-sum fields only"),
         stat=tuple((name, name) for name in SHIFT_COLUMNS)),
    Test(KS, conflicts=((PAIRED, "the signed-rank test compares matched samples; this test compares two distributions"),
                        (TREND, "the trend test orders three or more sets"),
                        (MX, "there is no k-sample Kolmogorov-Smirnov test here"),
                        (STRATA, "there is no stratified Kolmogorov-Smirnov test here")),
         multi_rank=_multi_rank(KS, "the packed all-gather carries the rank-sum fields only"),
         fields=KS_FIELDS, inputs=_two_sets, stat=(("D", "d"),),
         dev=lambda ctx, sel: lambda d, out: ctx.ks_dev(d["ps"], d["g1"], d["g2"], out, sel.exact),
         host=lambda ctx, matrix, sel: ctx.ks(matrix, sel.g1_idx, sel.g2_idx, sel.exact)),
    Test(TREND, needs=(MX, "three or more ordered sets; two sets are the rank-sum test"),
         conflicts=((PAIRED, "the signed-rank test compares two matched sets"),
                    (EXACT, "the trend test is asymptotic only"),
                    (STRATA, "there is no stratified trend test here")),
         multi_rank=_multi_rank(TREND, "the packed all-gather carries the two-set fields only"),
         fields=JONCKHEERE_FIELDS, stat=(("z", "z"),), **_k_sets("jonckheere")),
    Test(EXACT, conflicts=((MX, "there is no exact Kruskal-Wallis test here"),)),
    Test(STRATA, conflicts=((PAIRED, "the signed-rank test pairs samples one to one"),
                            (MX, "there is no stratified Kruskal-Wallis test here"),
                            (EXACT, "there is no exact stratified test here")),
         multi_rank=_multi_rank(STRATA, "the sharded two-set path does not carry the stratum ids"),
         fields=RANKSUM_FIELDS, inputs=lambda sel: dict(_two_sets(sel), s1=(sel.strat1, np.int32), s2=(sel.strat2, np.int32)),
         dev=lambda ctx, sel: lambda d, out: ctx.ranksum_strata_dev(d["ps"], d["g1"], d["g2"], d["s1"], d["s2"],
                                                                    sel.n_strata, out),
         host=lambda ctx, matrix, sel: ctx.ranksum_strata(matrix, sel.g1_idx, sel.g2_idx, sel.strat1, sel.strat2)),
    Test(PAIRED, conflicts=((MX, "the signed-rank test compares two matched sets"),)),
    # (before -mx: the Kruskal-Wallis pipeline with the pair epilogue is the one that runs)
    Test(POSTHOC, needs=(MX, "Dunn's test compares the pairs of three or more sets; two sets are the rank-sum test"),
         conflicts=((TREND, "the trend test has one ordered alternative, not pairs"),),
         multi_rank=_multi_rank(POSTHOC, "the packed all-gather carries the two-set fields only"),
         fields=[f for f in KRUSKAL_DUNN_FIELDS if f[0] != "pair_p"],        # (the table prints z and padj: pair_p stays NULL)
         stat=_dunn_columns, **_k_sets("kruskal_dunn")),
    # k >= 3 sets: Kruskal-Wallis per junction (--trend above: Jonckheere-Terpstra over the sets in this order)
    Test(MX, multi_rank=_multi_rank(MX, "the packed all-gather carries the two-set fields only"),
         fields=KRUSKAL_FIELDS, stat=(("H", "h"),), **_k_sets("kruskal")),
    # (last, so that every older refusal of what it is combined with comes first; it keeps the signed-rank pipeline, as
    # --shift keeps the rank-sum one: compare() adds the walsh call to the same pass)
    Test(PSEUDOMEDIAN, needs=(PAIRED, "it is the estimate that belongs to the signed-rank test of matched samples; two "
                                      "independent sets have --shift"),
         multi_rank=_multi_rank(PSEUDOMEDIAN, "the packed all-gather carries the signed-rank fields only"),
         stat=tuple((name, name) for name in SHIFT_COLUMNS)),
)
BY_FLAG = {t.flag: t for t in TESTS}
# --repeated --trend: the same row with Page's call, fields and column
PAGE = BY_FLAG[REPEATED]._replace(fields=PAGE_FIELDS, stat=(("z", "z"),), **_matched_sets("page"))
KS_MULTI_RANK_REFUSAL, TREND_MULTI_RANK_REFUSAL, STRATA_MULTI_RANK_REFUSAL, MULTI_RANK_REFUSAL = (
    BY_FLAG[f].multi_rank for f in (KS, TREND, STRATA, MX))
refuse, refuse_strata = BY_FLAG[PAIRED].refuse, BY_FLAG[STRATA].refuse


def run_with(args, ctx=None):
    from . import _stages, mgpu
    from .engine import friedman_columns, kruskal_sets
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    g1 = samples_from_manifest(args.manifest1)
    g2 = samples_from_manifest(args.manifest2)
    more = [samples_from_manifest(m) for m in (getattr(args, "moreManifests", None) or [])]
    on = {PAIRED: getattr(args, "paired", False), EXACT: getattr(args, "exact", False), STRATA: getattr(args, "strata", None),
          TREND: getattr(args, "trend", False), KS: getattr(args, "ks", False), MX: more,
          SHIFT: getattr(args, "shift", False), CONF: getattr(args, "conf", None) is not None,
          POSTHOC: getattr(args, "posthoc", False), REPEATED: getattr(args, "repeated", False),
          PSEUDOMEDIAN: getattr(args, "pseudomedian", False)}
    chosen = [PAGE if t.flag == REPEATED and on[TREND] else t for t in TESTS if on[t.flag]]
    sel = argparse.Namespace(exact=bool(on[EXACT]))
    conf = None
    if on[SHIFT] or on[PSEUDOMEDIAN]:
        conf = float(args.conf) if on[CONF] else 0.95
        if not 0.0 < conf < 1.0:                  # (NaN included)
            BY_FLAG[CONF].refuse(f"LEVEL must satisfy 0 < LEVEL < 1 (got {args.conf})")
    for t in chosen:
        if t.needs and not on[t.needs[0]] and not any(on[f] for f in t.needs_or):
            t.refuse(f"needs {t.needs[0]} ({t.needs[1]})")
        for other, why in t.conflicts:
            if on[other]:
                t.refuse(f"cannot be combined with {other} ({why})")
        if t.multi_rank and t.flag != MX:        # (-mx alone is refused after the size check below, as it always was)
            _cli.refuse_multi_rank(L, t.multi_rank)
    if on[STRATA]:                   # (the two that pick their columns from the header alone: they exit before any GPU call)
        sel.g1_idx, sel.g2_idx, sel.strat1, sel.strat2, sel.n_strata = strata_columns(
            g1, g2, table_header_names(args.psiSPLICEDICE), _cli.read_labels(on[STRATA], refuse_strata))
    if on[PAIRED]:
        sel.g1_idx, sel.g2_idx = paired_columns(g1, g2, table_header_names(args.psiSPLICEDICE))
    if on[REPEATED]:
        sel.set_idx = repeated_columns([g1, g2] + more, table_header_names(args.psiSPLICEDICE))
        sel.g1_idx, sel.g2_idx = sel.set_idx[:2]
    if len(g1) < 3 or len(g2) < 3 or any(len(g) < 3 for g in more):
        print("Cannot conduct wilcoxon with less than 3 samples in either group. Exit.", file=sys.stderr)
        sys.exit(1)
    if more:
        _cli.refuse_multi_rank(L, MULTI_RANK_REFUSAL)
    if on[POSTHOC] and 2 + len(more) > DUNN_MAX_SETS:
        BY_FLAG[POSTHOC].refuse(f"{2 + len(more)} sample sets, at most {DUNN_MAX_SETS} are supported (their "
                                f"{(2 + len(more)) * (1 + len(more)) // 2} pairs do not fit the 64 lanes of a wave)")
    test = next((t for t in chosen if t.dev), None)
    with _stages.stage("parse"):
        rows, cols, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    if not hasattr(sel, "g1_idx"):
        sel.g1_idx, sel.g2_idx = column_indices(g1, cols), column_indices(g2, cols)
    if on[REPEATED]:
        sel.cols = friedman_columns(sel.set_idx, matrix.shape[1])
    elif more:
        sel.set_idx = [sel.g1_idx, sel.g2_idx] + [column_indices(g, cols) for g in more]
        sel.cols, sel.set_ptr = kruskal_sets(sel.set_idx, matrix.shape[1])       # (raises on a column in two sets)
    with _cli.engine_scope(ctx, lambda: Context(L.local_rank)) as ctx:
        if test:
            keep, r = tested(ctx, matrix, test.fields, test.inputs(sel), test.dev(ctx, sel),
                             lambda: test.host(ctx, matrix, sel), test.k(sel))
        elif L.world > 1:
            keep, r = compare_sharded(matrix, sel.g1_idx, sel.g2_idx, ctx, L, bool(on[PAIRED]), sel.exact)
        else:
            keep, r = compare(matrix, sel.g1_idx, sel.g2_idx, ctx, bool(on[PAIRED]), sel.exact, conf)
    if not L.root:
        return                       # one set of output files: rank 0 writes the table
    # the library's multithreaded formatter (numpy str() of float32 / float64 per column, byte-identical to the
    # reference's print(*fields, sep="\t")); columns: event mean1..meank median1..mediank delta [statistics] p-value corrected
    k = 2 + len(more)
    means, medians = (r["mean"], r["med"]) if more else ((r["mean1"], r["mean2"]), (r["med1"], r["med2"]))
    stat = [cell for t in chosen if t is test or not t.dev for cell in t.columns(k)]
    header = "\t".join(["event"] + [f"mean{i + 1}" for i in range(k)] + [f"median{i + 1}" for i in range(k)] + ["delta"] +
                       [cell for cell, _ in stat] + ["p-value", "corrected"])
    columns = ([*means, *medians, r["delta"]] + [r[key] if isinstance(key, str) else r[key[0]][key[1]] for _, key in stat] +
               [r["p"], r["corrected"]])
    _cli.write_event_table(args.outputFile, header, rows, keep, columns, ["repr"] * len(columns), args.annotation)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
