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

On the GPU: the per-row loop :216-232 (NaN drop, <3 skip, scipy ranksums, medians, means)
-> sdice_ranksum; multipletests(..., "fdr_bh") :235 -> sdice_bh over the tested rows.
The GTF annotation columns are host string work, as in the reference.
"""
import sys

import numpy as np

from . import _cli
from ._cli import annotation_suffixes, read_annotation, read_ps_table, samples_from_manifest, table_header_names  # noqa: F401
from .engine import (JONCKHEERE_FIELDS, KRUSKAL_FIELDS, KS_FIELDS, RANKSUM_EXACT_FIELDS, RANKSUM_FIELDS, Context,
                     field_shapes)

refuse = _cli.refusal("compare_sample_sets --paired")
refuse_exact = _cli.refusal("compare_sample_sets --exact")
refuse_strata = _cli.refusal("compare_sample_sets --strata")
refuse_trend = _cli.refusal("compare_sample_sets --trend")
refuse_ks = _cli.refusal("compare_sample_sets --ks")
MAX_STRATA = 64                     # strata a call accepts (include/sdice.h)


def row_test(ctx, paired, exact, dev=False):
    """the context's call for the chosen test: ranksum / signedrank, their _exact forms with --exact, _dev on resident data"""
    return getattr(ctx, ("signedrank" if paired else "ranksum") + ("_exact" if exact else "") + ("_dev" if dev else ""))


def column_indices(group, cols):
    """Columns of the table that belong to the group, in TABLE order (compareSampleSets.py:96-102)."""
    return np.nonzero(np.isin(cols, group))[0].astype(np.int32)


def compare_dev(matrix, g1_idx, g2_idx, ctx, paired=False, exact=False):
    """compare() on the HIP engine stage by stage: table up, rank-sum (paired: signed-rank) + BH over the tested rows on
    resident vectors, per-row results down (sdice_ranksum + sdice_bh do the same steps inside two host calls).  exact:
    the _exact calls; BH runs over the mixed p vector and the `exact` marks stay behind."""
    test = row_test(ctx, paired, exact, dev=True)
    keep, r = _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), g1=(g1_idx, np.int32), g2=(g2_idx, np.int32)),
                               field_shapes(RANKSUM_EXACT_FIELDS if exact else RANKSUM_FIELDS, matrix.shape[0]),
                               lambda d, out: test(d["ps"], d["g1"], d["g2"], out))
    r.pop("exact", None)
    return keep, r


def compare(matrix, g1_idx, g2_idx, ctx, paired=False, exact=False):
    """-> (kept row indices, dict of compacted per-row results incl. BH-corrected p).  paired: g1_idx[q] and g2_idx[q]
    are the columns of pair q and the test is the signed-rank test.  exact: exact p-values on the small rows."""
    if hasattr(ctx, "ranksum_dev") and matrix.shape[0]:
        return compare_dev(matrix, g1_idx, g2_idx, ctx, paired, exact)
    res = row_test(ctx, paired, exact)(matrix, g1_idx, g2_idx)
    keep = np.flatnonzero(res["tested"])
    out = {k: res[k][keep] for k in ("p", "med1", "med2", "mean1", "mean2", "delta")}
    out["corrected"] = ctx.bh(out["p"]) if keep.size else np.zeros(0)
    return keep, out


def compare_strata(matrix, g1_idx, g2_idx, strat1, strat2, n_strata, ctx):
    """compare_dev() for --strata: table, column lists and their stratum ids up, the stratified rank-sum test + BH over
    the tested rows on resident vectors, per-row results down"""
    if not matrix.shape[0]:
        res = ctx.ranksum_strata(matrix, g1_idx, g2_idx, strat1, strat2)
        out = {k: res[k][:0] for k in ("p", "z", "med1", "med2", "mean1", "mean2", "delta")}
        return np.zeros(0, np.int64), {**out, "corrected": np.zeros(0)}
    return _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), g1=(g1_idx, np.int32), g2=(g2_idx, np.int32),
                                      s1=(strat1, np.int32), s2=(strat2, np.int32)),
                            field_shapes(RANKSUM_FIELDS, matrix.shape[0]),
                            lambda d, out: ctx.ranksum_strata_dev(d["ps"], d["g1"], d["g2"], d["s1"], d["s2"], n_strata, out))


def compare_ks(matrix, g1_idx, g2_idx, ctx, exact=False):
    """compare_dev() for --ks: table and column lists up, the Kolmogorov-Smirnov test + BH over the tested rows on
    resident vectors, per-row results down (the `exact` marks stay behind)"""
    if not matrix.shape[0]:
        res = ctx.ks(matrix, g1_idx, g2_idx, exact)
        out = {k: res[k][:0] for k in ("p", "d", "med1", "med2", "mean1", "mean2", "delta")}
        return np.zeros(0, np.int64), {**out, "corrected": np.zeros(0)}
    keep, r = _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), g1=(g1_idx, np.int32), g2=(g2_idx, np.int32)),
                               field_shapes(KS_FIELDS, matrix.shape[0]),
                               lambda d, out: ctx.ks_dev(d["ps"], d["g1"], d["g2"], out, exact))
    r.pop("exact", None)
    return keep, r


def compare_sets_dev(matrix, set_idx, ctx, trend=False):
    """the k-set pipeline (-mx): table up, Kruskal-Wallis (trend: Jonckheere-Terpstra over the sets in their order) + BH
    over the tested rows on resident vectors, per-row results down -> (kept row indices, dict: mean / med float32
    [k, kept], delta, h (trend: z, j), p, corrected)"""
    from .engine import kruskal_sets
    n, s = matrix.shape
    cols, set_ptr = kruskal_sets(set_idx, s)          # (raises on a column in two sets, before any launch)
    test = ctx.jonckheere_dev if trend else ctx.kruskal_dev
    return _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), cols=(cols, np.int32)),
                            field_shapes(JONCKHEERE_FIELDS if trend else KRUSKAL_FIELDS, n, len(set_idx)),
                            lambda d, out: test(d["ps"], d["cols"], set_ptr, out))


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
    parser.add_argument("--ks", action="store_true",
                        help="The two-sample Kolmogorov-Smirnov test instead of the rank-sum test: it answers to any "
                             "difference between the two distributions (a junction switched on in part of a set, a "
                             "bimodal set), not to a shift alone.  The table gains the column D (the KS statistic, 0..1) "
                             "before p-value.  The p-value is Kolmogorov's limiting distribution "
                             "(scipy.special.kolmogorov, no finite-n correction); with --exact the rows that keep at "
                             "most 32 values get the exact conditional p-value given their ties (R's ks.test(exact = "
                             "TRUE)).  Not with --paired, -mx, --strata or --trend (not part of the reference)")
    parser.add_argument("-a", "--annotation", type=str, required=False, default="",
                        help="Optional GTF file to label known splice junctions and genes")
    parser.add_argument("-o", "--outputFile", type=str, required=True,
                        help="Output filename for tab-separated table")


MULTI_RANK_REFUSAL = ("compare_sample_sets: -mx/--moreManifests is not available under the multi-rank launcher "
                      "(the packed all-gather carries the two-set fields only); run it in one process.")

STRATA_MULTI_RANK_REFUSAL = ("compare_sample_sets: --strata is not available under the multi-rank launcher "
                             "(the sharded two-set path does not carry the stratum ids); run it in one process.")


TREND_MULTI_RANK_REFUSAL = ("compare_sample_sets: --trend is not available under the multi-rank launcher "
                            "(the packed all-gather carries the two-set fields only); run it in one process.")


KS_MULTI_RANK_REFUSAL = ("compare_sample_sets: --ks is not available under the multi-rank launcher "
                         "(the packed all-gather carries the rank-sum fields only); run it in one process.")


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


def run_with(args, ctx=None):
    from . import _stages, mgpu
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    g1 = samples_from_manifest(args.manifest1)
    g2 = samples_from_manifest(args.manifest2)
    more = [samples_from_manifest(m) for m in (getattr(args, "moreManifests", None) or [])]
    paired = bool(getattr(args, "paired", False))
    exact = bool(getattr(args, "exact", False))
    trend = bool(getattr(args, "trend", False))
    ks = bool(getattr(args, "ks", False))
    if ks:
        for on, flag in ((paired, "--paired (the signed-rank test compares matched samples; this test compares two "
                                  "distributions)"),
                         (trend, "--trend (the trend test orders three or more sets)"),
                         (more, "-mx/--moreManifests (there is no k-sample Kolmogorov-Smirnov test here)"),
                         (getattr(args, "strata", None), "--strata (there is no stratified Kolmogorov-Smirnov test here)")):
            if on:
                refuse_ks(f"cannot be combined with {flag}")
        _cli.refuse_multi_rank(L, KS_MULTI_RANK_REFUSAL)
    if trend:
        if not more:
            refuse_trend("needs -mx/--moreManifests (three or more ordered sets; two sets are the rank-sum test)")
        for on, flag in ((paired, "--paired (the signed-rank test compares two matched sets)"),
                         (exact, "--exact (the trend test is asymptotic only)"),
                         (getattr(args, "strata", None), "--strata (there is no stratified trend test here)")):
            if on:
                refuse_trend(f"cannot be combined with {flag}")
        _cli.refuse_multi_rank(L, TREND_MULTI_RANK_REFUSAL)
    if exact and more:
        refuse_exact("cannot be combined with -mx/--moreManifests (there is no exact Kruskal-Wallis test here)")
    strata = getattr(args, "strata", None)
    if strata:
        for on, flag in ((paired, "--paired (the signed-rank test pairs samples one to one)"),
                         (more, "-mx/--moreManifests (there is no stratified Kruskal-Wallis test here)"),
                         (exact, "--exact (there is no exact stratified test here)")):
            if on:
                refuse_strata(f"cannot be combined with {flag}")
        _cli.refuse_multi_rank(L, STRATA_MULTI_RANK_REFUSAL)
        strat = strata_columns(g1, g2, table_header_names(args.psiSPLICEDICE), _cli.read_labels(strata, refuse_strata))
    if paired:
        if more:
            refuse("cannot be combined with -mx/--moreManifests (the signed-rank test compares two matched sets)")
        pair_idx = paired_columns(g1, g2, table_header_names(args.psiSPLICEDICE))      # (exits before any GPU call)
    if len(g1) < 3 or len(g2) < 3 or any(len(g) < 3 for g in more):
        print("Cannot conduct wilcoxon with less than 3 samples in either group. Exit.", file=sys.stderr)
        sys.exit(1)
    if more:
        _cli.refuse_multi_rank(L, MULTI_RANK_REFUSAL)
    with _stages.stage("parse"):
        rows, cols, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    with _cli.engine_scope(ctx, lambda: Context(L.local_rank)) as ctx:
        if strata:
            keep, r = compare_strata(matrix, *strat, ctx)
        elif ks:
            keep, r = compare_ks(matrix, column_indices(g1, cols), column_indices(g2, cols), ctx, exact)
        elif more:
            # k >= 3 sets: Kruskal-Wallis per junction; columns event mean1..meank median1..mediank delta H p-value corrected
            # (--trend: Jonckheere-Terpstra over the sets in this order, z where H stands)
            keep, r = compare_sets_dev(matrix, [column_indices(g, cols) for g in [g1, g2] + more], ctx, trend)
        else:
            g1_idx, g2_idx = pair_idx if paired else (column_indices(g1, cols), column_indices(g2, cols))
            if L.world > 1:
                keep, r = compare_sharded(matrix, g1_idx, g2_idx, ctx, L, paired, exact)
            else:
                keep, r = compare(matrix, g1_idx, g2_idx, ctx, paired, exact)
    if not L.root:
        return                       # one set of output files: rank 0 writes the table
    # the library's multithreaded formatter (numpy str() of float32 / float64 per column, byte-identical to the
    # reference's print(*fields, sep="\t"))
    if more:
        k = 2 + len(more)
        header = "\t".join(["event"] + [f"mean{i + 1}" for i in range(k)] + [f"median{i + 1}" for i in range(k)] +
                           ["delta", "z" if trend else "H", "p-value", "corrected"])
        columns = [*r["mean"], *r["med"], r["delta"], r["z" if trend else "h"], r["p"], r["corrected"]]
    elif ks:
        header = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tD\tp-value\tcorrected"
        columns = [r["mean1"], r["mean2"], r["med1"], r["med2"], r["delta"], r["d"], r["p"], r["corrected"]]
    else:
        header = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected"
        columns = [r["mean1"], r["mean2"], r["med1"], r["med2"], r["delta"], r["p"], r["corrected"]]
    _cli.write_event_table(args.outputFile, header, rows, keep, columns, ["repr"] * len(columns), args.annotation)


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
