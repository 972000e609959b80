"""`splicedice correlate`: Spearman rank correlation per junction of an `_allPS.tsv` with one covariate value per sample
(age, tumour purity, dose, time point, the expression of a splicing factor).  Not part of the reference; DESIGN.md
section 7.

    splicedice correlate --psiSPLICEDICE t_allPS.tsv --covariate age.tsv [-a genes.gtf] -o out.tsv

The covariate file holds one `sample<whitespace>value` per line; blank lines are ignored and a sample whose value is `NA` or
`nan` (any case) is left out.  Per junction the samples with a PS value are kept; with at least 3 of them the row is
tested: scipy.stats.spearmanr of the kept covariate values and the kept PS values, Benjamini-Hochberg over the tested
rows.  Output columns `event n mean median rho p-value corrected` (+ gene / overlapping / transcript_id with -a GTF): n is
the kept count, mean and median are of the kept PS values, floats are printed as numpy float32 / float64 scalars.

On the GPU: sdice_spearman (rank correlation, its p-value, n, mean, median) -> sdice_bh over the tested rows.
"""
import sys

import numpy as np

from .compare_sample_sets import annotation_suffixes, read_ps_table, table_header_names
from .engine import Context, spearman_order

MIN_SAMPLES = 3
MAX_SAMPLES = 4096                  # columns one sdice_spearman call takes (include/sdice.h)

MULTI_RANK_REFUSAL = ("correlate: not available under the multi-rank launcher (the packed all-gather carries the two-set "
                      "fields only); run it in one process.")


def refuse(why):
    print(f"correlate: {why}. Exit.", file=sys.stderr)
    sys.exit(1)


def read_covariate(path):
    """the covariate file -> ([sample names], float64 values) of the usable lines, in file order; prints why and exits with
    status 1 on a line that cannot be read, an infinite value or a name listed twice"""
    names, values, seen = [], [], set()
    with open(path) as fin:
        for lineno, line in enumerate(fin, 1):
            cells = line.split()
            if not cells:
                continue
            if len(cells) < 2:
                refuse(f"{path} line {lineno}: sample {cells[0]!r} has no value")
            name, text = cells[0], cells[1]
            if name in seen:
                refuse(f"{path} line {lineno}: sample {name!r} is listed twice")
            seen.add(name)
            if text.lower() in ("na", "nan"):
                continue
            try:
                value = float(text)
            except ValueError:
                refuse(f"{path} line {lineno}: cannot read {text!r} as a number (sample {name!r})")
            if not np.isfinite(value):          # (inf, or a spelling of NaN that float() knows and the rule above does not)
                refuse(f"{path} line {lineno}: the value of sample {name!r} is not finite ({text})")
            names.append(name)
            values.append(value)
    return names, np.array(values, dtype=np.float64)


def covariate_columns(names, header_names):
    """the usable samples and the table's column names -> int32 column index of each sample; prints why and exits with
    status 1 when a sample is not exactly once in the header or their number is outside 3..4096"""
    if len(names) < MIN_SAMPLES:
        refuse(f"cannot correlate with fewer than {MIN_SAMPLES} samples that have a value (got {len(names)})")
    if len(names) > MAX_SAMPLES:
        refuse(f"{len(names)} samples have a value, at most {MAX_SAMPLES} are supported")
    where = {}
    for j, name in enumerate(header_names):
        where.setdefault(name, []).append(j)
    for name in names:
        hits = where.get(name, [])
        if len(hits) != 1:
            refuse(f"sample {name!r} " + ("is missing from the table header" if not hits else
                                          f"appears {len(hits)} times in the table header"))
    return np.array([where[x][0] for x in names], dtype=np.int32)


def correlate_dev(matrix, cols, xg, ctx):
    """the pipeline of compare_sample_sets.compare_dev: table up, Spearman + BH over the tested rows on resident vectors,
    per-row results down -> (kept row indices, dict of compacted per-row results incl. BH-corrected p)"""
    from . import _stages
    n = matrix.shape[0]
    with _stages.stage("h2d"):
        d_ps = ctx.to_device(matrix, np.float32)
        d_cols, d_xg = ctx.to_device(cols, np.int32), ctx.to_device(xg, np.int32)
        out = dict(tested=ctx.empty(n, np.uint8), p=ctx.empty(n, np.float64), rho=ctx.empty(n, np.float64),
                   n_kept=ctx.empty(n, np.int32), med=ctx.empty(n, np.float32), mean=ctx.empty(n, np.float32))
        d_q = ctx.empty(n, np.float64)
    with _stages.stage("kernels"):
        ctx.spearman_dev(d_ps, d_cols, d_xg, out)
        ctx.bh_masked_dev(out["p"], out["tested"], d_q)
        ctx.sync()
    with _stages.stage("d2h"):
        res = {k: v.to_host() for k, v in out.items()}
        q = d_q.to_host()
    for a in (d_ps, d_cols, d_xg, d_q, *out.values()):
        a.free()
    keep = np.flatnonzero(res["tested"])
    r = {k: res[k][keep] for k in ("n_kept", "mean", "med", "rho", "p")}
    r["corrected"] = q[keep]
    return keep, r


def add_parser(parser):
    parser.add_argument("--psiSPLICEDICE", type=str, required=True,
                        help="PS table (_allPS.tsv) from 'splicedice quant'.")
    parser.add_argument("--covariate", type=str, required=True, metavar="FILE",
                        help="One 'sample<whitespace>value' per line; a sample whose value is NA or nan is left out")
    parser.add_argument("-a", "--annotation", type=str, required=False, default="",
                        help="Optional GTF file to label known splice junctions and genes")
    parser.add_argument("-o", "--outputFile", type=str, required=True,
                        help="Output filename for tab-separated table")


def run_with(args, ctx=None):
    from . import _stages, mgpu, textio
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    if L.world > 1:
        print(MULTI_RANK_REFUSAL, file=sys.stderr)
        sys.exit(1)
    names, values = read_covariate(args.covariate)
    idx = covariate_columns(names, table_header_names(args.psiSPLICEDICE))      # (exits before any GPU call)
    cols, xg = spearman_order(idx, values)
    with _stages.stage("parse"):
        rows, _, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    n = matrix.shape[0]
    if n:
        own_ctx = ctx is None
        ctx = ctx if ctx is not None else Context(L.local_rank)
        try:
            keep, r = correlate_dev(matrix, cols, xg, ctx)
        finally:
            if own_ctx:
                ctx.close()
    else:
        keep = np.zeros(0, np.int64)
        r = dict(n_kept=np.zeros(0, np.int32), mean=np.zeros(0, np.float32), med=np.zeros(0, np.float32),
                 rho=np.zeros(0), p=np.zeros(0), corrected=np.zeros(0))
    header = "event\tn\tmean\tmedian\trho\tp-value\tcorrected"
    columns = [r["n_kept"], r["mean"], r["med"], r["rho"], r["p"], r["corrected"]]
    modes = [".0f"] + ["repr"] * 5
    if not args.annotation:
        with _stages.stage("format+write"):
            textio.write_columns(args.outputFile, header + "\n", rows.take(keep), columns, modes)
        return
    kept_names = list(rows.take(keep))
    suffixes = annotation_suffixes(kept_names, args.annotation)
    with _stages.stage("format+write"):
        textio.write_columns(args.outputFile, header + "\tgene\toverlapping\ttranscript_id\n", kept_names, columns, modes,
                             suffixes=suffixes)


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
