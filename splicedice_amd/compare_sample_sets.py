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

On the GPU: the per-row loop :216-232 (NaN drop, <3 skip, scipy ranksums, medians, means)
-> sdice_ranksum; multipletests(..., "fdr_bh") :235 -> sdice_bh over the tested rows.
The GTF annotation columns are host string work, as in the reference.
"""
import sys

import numpy as np

from .engine import Context


def samples_from_manifest(path):
    """First whitespace-separated token of every line (compareSampleSets.py:105-115)."""
    with open(path) as fin:
        return [line.split()[0] for line in fin]


def column_indices(group, cols):
    """Columns of the table that belong to the group, in TABLE order (compareSampleSets.py:96-102)."""
    return np.nonzero(np.isin(cols, group))[0].astype(np.int32)


def read_ps_table(path, as_table=False):
    """`_allPS.tsv` -> (row names array, column names array, float32 matrix), :193-204.  as_table: the row names as a
    textio.NameTable (one byte string + offsets: a million-row table costs no Python string per row)."""
    from . import textio
    header, rows, matrix = textio.read_table_numeric(path, np.float32, as_table=as_table)     # text -> float64 -> float32, as numpy
    headers = header.strip().split("\t")[1:]
    return (rows if as_table else np.array(rows)), np.array(headers), matrix


def read_annotation(gtf_path):
    """GTF -> (junction -> gene names, (chrom,strand) -> {(start,stop): gene names},
    junction -> transcript ids); restates getAnnotated (compareSampleSets.py:32-93)."""
    def attr(info, key):
        return [x[1] for x in info if key in x[0]][0]

    gene_coords, genes, transcripts = {}, {}, {}
    with open(gtf_path) as gtf:
        for line in gtf:
            if line.startswith("#"):
                continue
            row = line.rstrip().split("\t")
            info = [x.split('"') for x in row[8].split(";")]
            chrom, strand = row[0], row[6]
            start, stop = int(row[3]), int(row[4]) - 1
            if row[2] == "transcript":
                tid = attr(info, "transcript_id")
                genes[tid] = attr(info, "gene_name")
                transcripts[(tid, chrom, strand)] = []
            elif row[2] == "exon":
                transcripts[(attr(info, "transcript_id"), chrom, strand)].append((start, stop))
            elif row[2] == "gene":
                gene_name = attr(info, "gene_name")
                attr(info, "gene_id")      # the reference requires the attribute to exist
                gene_coords.setdefault((chrom, strand), {}).setdefault((start, stop), []).append(gene_name)
    annotated, transcript_ids = {}, {}
    for (tid, chromosome, strand), exons in transcripts.items():
        for i in range(len(exons) - 1):
            junction = (chromosome, exons[i][1], exons[i + 1][0], strand)
            if junction in annotated:
                if genes[tid] not in annotated[junction]:
                    annotated[junction].append(genes[tid])
                    transcript_ids[junction].append(tid)
            else:
                annotated[junction] = [genes[tid]]
                transcript_ids[junction] = [tid]
    return annotated, gene_coords, transcript_ids


def annotation_suffixes(names, gtf_path):
    """'\\tgene\\toverlapping\\ttranscript_id' for every event name (compareSampleSets.py:238-264).  The reference
    walks all gene intervals of the event's (chromosome, strand) per event in Python; here that scan is the
    library's threaded interval join (sdice_interval_overlaps) and the known-junction look-ups stay dict
    look-ups; order of the listed genes = the reference's (dict order of the intervals, file order inside)."""
    from . import textio
    annotated, gene_coords, transcript_ids = read_annotation(gtf_path)
    groups = {key: g for g, key in enumerate(gene_coords)}
    grp_ptr = np.zeros(len(groups) + 1, dtype=np.int64)
    lo, hi, key_names = [], [], []
    for g, intervals in enumerate(gene_coords.values()):
        for (gene_start, gene_stop), gene_names in intervals.items():
            lo.append(gene_start)
            hi.append(gene_stop)
            key_names.append(",".join(gene_names))
        grp_ptr[g + 1] = len(lo)
    ev_group = np.empty(len(names), dtype=np.int32)
    ev_a = np.empty(len(names), dtype=np.int64)
    ev_b = np.empty(len(names), dtype=np.int64)
    junctions = []
    for n, name in enumerate(names):
        chromosome, coords, strand = name.split(":")
        start, stop = (int(x) for x in coords.split("-"))
        start -= 1
        stop += 1
        junctions.append((chromosome, start, stop, strand))
        ev_group[n] = groups.get((chromosome, strand), -1)
        ev_a[n] = start
        ev_b[n] = stop
    ptr, idx = textio.interval_overlaps(ev_group, ev_a, ev_b, grp_ptr, lo, hi)
    ptr = ptr.tolist()
    idx = idx.tolist()
    nan = ["nan"]
    return ["\t" + ",".join(annotated.get(j, nan)) + "\t" + ",".join(key_names[k] for k in idx[ptr[n]:ptr[n + 1]]) +
            "\t" + ",".join(transcript_ids.get(j, nan)) for n, j in enumerate(junctions)]


def compare_dev(matrix, g1_idx, g2_idx, ctx, paired=False):
    """compare() on the HIP engine stage by stage: table up, rank-sum (paired: signed-rank) + BH over the tested rows on
    resident vectors, per-row results down (sdice_ranksum + sdice_bh do the same steps inside two host calls)"""
    from . import _stages
    n = matrix.shape[0]
    f32 = ("med1", "med2", "mean1", "mean2", "delta")
    with _stages.stage("h2d"):
        d_ps = ctx.to_device(matrix, np.float32)
        d_g1, d_g2 = ctx.to_device(g1_idx, np.int32), ctx.to_device(g2_idx, np.int32)
        out = dict(tested=ctx.empty(n, np.uint8), p=ctx.empty(n, np.float64), z=ctx.empty(n, np.float64),
                   **{k: ctx.empty(n, np.float32) for k in f32})
        d_q = ctx.empty(n, np.float64)
    with _stages.stage("kernels"):
        (ctx.signedrank_dev if paired else ctx.ranksum_dev)(d_ps, d_g1, d_g2, out)
        ctx.bh_masked_dev(out["p"], out["tested"], d_q)
        ctx.sync()
    with _stages.stage("d2h"):
        res = {k: v.to_host() for k, v in out.items()}
        q = d_q.to_host()
    for a in (d_ps, d_g1, d_g2, d_q, *out.values()):
        a.free()
    keep = np.flatnonzero(res["tested"])
    r = {k: res[k][keep] for k in ("p",) + f32}
    r["corrected"] = q[keep]
    return keep, r


def compare(matrix, g1_idx, g2_idx, ctx, paired=False):
    """-> (kept row indices, dict of compacted per-row results incl. BH-corrected p).  paired: g1_idx[q] and g2_idx[q]
    are the columns of pair q and the test is the signed-rank test."""
    if hasattr(ctx, "ranksum_dev") and matrix.shape[0]:
        return compare_dev(matrix, g1_idx, g2_idx, ctx, paired)
    res = (ctx.signedrank if paired else ctx.ranksum)(matrix, g1_idx, g2_idx)
    keep = np.flatnonzero(res["tested"])
    out = {k: res[k][keep] for k in ("p", "med1", "med2", "mean1", "mean2", "delta")}
    out["corrected"] = ctx.bh(out["p"]) if keep.size else np.zeros(0)
    return keep, out


def compare_sets_dev(matrix, set_idx, ctx):
    """the k-set pipeline (-mx): table up, Kruskal-Wallis + BH over the tested rows on resident vectors, per-row results
    down -> (kept row indices, dict: mean / med float32 [k, kept], delta, h, p, corrected)"""
    from . import _stages
    from .engine import kruskal_sets
    n, s = matrix.shape
    cols, set_ptr = kruskal_sets(set_idx, s)          # (raises on a column in two sets, before any launch)
    k = len(set_idx)
    with _stages.stage("h2d"):
        d_ps = ctx.to_device(matrix, np.float32)
        d_cols = ctx.to_device(cols, np.int32)
        out = dict(tested=ctx.empty(n, np.uint8), p=ctx.empty(n, np.float64), h=ctx.empty(n, np.float64),
                   med=ctx.empty((k, n), np.float32), mean=ctx.empty((k, n), np.float32), delta=ctx.empty(n, np.float32))
        d_q = ctx.empty(n, np.float64)
    with _stages.stage("kernels"):
        ctx.kruskal_dev(d_ps, d_cols, set_ptr, out)
        ctx.bh_masked_dev(out["p"], out["tested"], d_q)
        ctx.sync()
    with _stages.stage("d2h"):
        res = {name: v.to_host() for name, v in out.items()}
        q = d_q.to_host()
    for a in (d_ps, d_cols, d_q, *out.values()):
        a.free()
    keep = np.flatnonzero(res["tested"])
    r = {name: res[name][keep] for name in ("p", "h", "delta")}
    r["med"] = np.ascontiguousarray(res["med"][:, keep])
    r["mean"] = np.ascontiguousarray(res["mean"][:, keep])
    r["corrected"] = q[keep]
    return keep, r


def compare_sharded(matrix, g1_idx, g2_idx, ctx, L, paired=False):
    """compare() with the table rows cut into one block per rank (rows are independent here): every rank tests its
    block, the per-row statistics cross the ranks as ONE packed block in ONE all-gather (distributed.stat_layout, padded to
    the longest block), rank 0 corrects."""
    from . import distributed
    n = matrix.shape[0]
    lo, hi = L.row_block(n)
    rows_of = [b - a for a, b in (L.row_block(n, r) for r in range(L.world))]
    maxk = distributed.longest(rows_of)
    res = (ctx.signedrank if paired else ctx.ranksum)(np.ascontiguousarray(matrix[lo:hi]), g1_idx, g2_idx)
    stats = {k: distributed.pad_rows(np.asarray(res[k], dt), maxk) for k, dt in zip(distributed.STAT_NAMES, distributed.STAT_DTYPES)}
    gathered = L.comm(ctx).allgather(distributed.pack_stats_host(stats, maxk))
    host = distributed.unpack_stats_host(gathered, maxk, L.world)
    full = {k: distributed.drop_padding(host[k], rows_of, maxk) for k in ("tested", "p", "med1", "med2", "mean1", "mean2", "delta")}
    keep = np.flatnonzero(full["tested"])
    out = {k: full[k][keep] for k in ("p", "med1", "med2", "mean1", "mean2", "delta")}
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
    parser.add_argument("-a", "--annotation", type=str, required=False, default="",
                        help="Optional GTF file to label known splice junctions and genes")
    parser.add_argument("-o", "--outputFile", type=str, required=True,
                        help="Output filename for tab-separated table")


MULTI_RANK_REFUSAL = ("compare_sample_sets: -mx/--moreManifests is not available under the multi-rank launcher "
                      "(the packed all-gather carries the two-set fields only); run it in one process.")


def paired_columns(g1, g2, header_names):
    """--paired: the manifests' sample lists and the table's column names -> (a, b) int32 column indices, pair q =
    (a[q], b[q]) in manifest order; prints why and exits with status 1 when the lists cannot be paired"""
    def refuse(why):
        print(f"compare_sample_sets --paired: {why}. Exit.", file=sys.stderr)
        sys.exit(1)
    if len(g1) != len(g2):
        refuse(f"the manifests differ in length ({len(g1)} and {len(g2)} samples); line i of -m1 is paired with line i of -m2")
    if len(g1) < 3:
        refuse(f"cannot conduct the signed-rank test with fewer than 3 pairs (got {len(g1)})")
    seen = set()
    for name in g1 + g2:
        if name in seen:
            refuse(f"sample {name!r} appears twice in the manifests; a sample belongs to one pair only")
        seen.add(name)
    where = {}
    for j, name in enumerate(header_names):
        where.setdefault(name, []).append(j)
    for name in g1 + g2:
        hits = where.get(name, [])
        if len(hits) != 1:
            refuse(f"sample {name!r} " + ("is missing from the table header" if not hits else
                                          f"appears {len(hits)} times in the table header"))
    return (np.array([where[x][0] for x in g1], dtype=np.int32), np.array([where[x][0] for x in g2], dtype=np.int32))


def table_header_names(path):
    """the sample names of an `_allPS.tsv` header (its first line alone is read)"""
    with open(path) as fin:
        return fin.readline().strip().split("\t")[1:]


def run_sets(args, groups, ctx=None, device=0):
    """compare_sample_sets with -mx: k >= 3 sets, Kruskal-Wallis per junction, BH over the tested rows; columns
    event mean1..meank median1..mediank delta H p-value corrected (+ the GTF columns with -a)."""
    from . import _stages, textio
    with _stages.stage("parse"):
        rows, cols, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    set_idx = [column_indices(g, cols) for g in groups]
    own_ctx = ctx is None
    ctx = ctx if ctx is not None else Context(device)
    try:
        keep, r = compare_sets_dev(matrix, set_idx, ctx)
    finally:
        if own_ctx:
            ctx.close()
    k = len(groups)
    header = "\t".join(["event"] + [f"mean{i + 1}" for i in range(k)] + [f"median{i + 1}" for i in range(k)] +
                       ["delta", "H", "p-value", "corrected"])
    columns = [*r["mean"], *r["med"], r["delta"], r["h"], r["p"], r["corrected"]]
    if not args.annotation:
        with _stages.stage("format+write"):
            textio.write_columns(args.outputFile, header + "\n", rows.take(keep), columns, ["repr"] * len(columns))
        return
    names = list(rows.take(keep))
    textio.write_columns(args.outputFile, header + "\tgene\toverlapping\ttranscript_id\n", names, columns,
                         ["repr"] * len(columns), suffixes=annotation_suffixes(names, args.annotation))


def run_with(args, ctx=None):
    from . import mgpu
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    g1 = samples_from_manifest(args.manifest1)
    g2 = samples_from_manifest(args.manifest2)
    more = [samples_from_manifest(m) for m in (getattr(args, "moreManifests", None) or [])]
    paired = bool(getattr(args, "paired", False))
    if paired:
        if more:
            print("compare_sample_sets --paired: cannot be combined with -mx/--moreManifests (the signed-rank test "
                  "compares two matched sets). Exit.", file=sys.stderr)
            sys.exit(1)
        pair_idx = paired_columns(g1, g2, table_header_names(args.psiSPLICEDICE))      # (exits before any GPU call)
    if len(g1) < 3 or len(g2) < 3 or any(len(g) < 3 for g in more):
        print("Cannot conduct wilcoxon with less than 3 samples in either group. Exit.", file=sys.stderr)
        sys.exit(1)
    if more:
        if L.world > 1:
            print(MULTI_RANK_REFUSAL, file=sys.stderr)
            sys.exit(1)
        return run_sets(args, [g1, g2] + more, ctx, L.local_rank)

    from . import _stages
    with _stages.stage("parse"):
        rows, cols, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    g1_idx, g2_idx = pair_idx if paired else (column_indices(g1, cols), column_indices(g2, cols))

    own_ctx = ctx is None
    ctx = ctx if ctx is not None else Context(L.local_rank)
    try:
        if L.world > 1:
            keep, r = compare_sharded(matrix, g1_idx, g2_idx, ctx, L, paired)
        else:
            keep, r = compare(matrix, g1_idx, g2_idx, ctx, paired)
    finally:
        if own_ctx:
            ctx.close()
    if not L.root:
        return                       # one set of output files: rank 0 writes the table

    base_header = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected"
    if not args.annotation:
        from . import textio
        # numeric table only: the library's multithreaded formatter (numpy str() of float32 /
        # float64 per column, byte-identical to the reference's print(*fields, sep="\t"))
        with _stages.stage("format+write"):
            textio.write_columns(args.outputFile, base_header + "\n", rows.take(keep),
                                 [r["mean1"], r["mean2"], r["med1"], r["med2"], r["delta"], r["p"], r["corrected"]],
                                 ["repr"] * 7)
        return
    from . import textio
    names = list(rows.take(keep))
    textio.write_columns(args.outputFile, base_header + "\tgene\toverlapping\ttranscript_id\n", names,
                         [r["mean1"], r["mean2"], r["med1"], r["med2"], r["delta"], r["p"], r["corrected"]],
                         ["repr"] * 7, suffixes=annotation_suffixes(names, args.annotation))


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
