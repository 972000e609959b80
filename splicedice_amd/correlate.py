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
import numpy as np

from . import _cli
from ._cli import read_ps_table, table_header_names
from .engine import SPEARMAN_FIELDS, Context, field_shapes, spearman_order

MIN_SAMPLES = 3
MAX_SAMPLES = 4096                  # columns one sdice_spearman call takes (include/sdice.h)

MULTI_RANK_REFUSAL = ("correlate: not available under the multi-rank launcher (the packed all-gather carries the two-set "
                      "fields only); run it in one process.")


refuse = _cli.refusal("correlate")


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
    return _cli.columns_in_header(names, header_names, refuse)


def correlate_dev(matrix, cols, xg, ctx):
    """the pipeline of compare_sample_sets.tested: table up, Spearman + BH over the tested rows on resident vectors,
    per-row results down -> (kept row indices, dict of compacted per-row results incl. BH-corrected p)"""
    return _cli.tested_rows(ctx, dict(ps=(matrix, np.float32), cols=(cols, np.int32), xg=(xg, np.int32)),
                            field_shapes(SPEARMAN_FIELDS, matrix.shape[0]),
                            lambda d, out: ctx.spearman_dev(d["ps"], d["cols"], d["xg"], out))


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
    from . import _stages, mgpu
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    _cli.refuse_multi_rank(L, MULTI_RANK_REFUSAL)
    names, values = read_covariate(args.covariate)
    idx = covariate_columns(names, table_header_names(args.psiSPLICEDICE))      # (exits before any GPU call)
    cols, xg = spearman_order(idx, values)
    with _stages.stage("parse"):
        rows, _, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    if matrix.shape[0]:
        with _cli.engine_scope(ctx, lambda: Context(L.local_rank)) as ctx:
            keep, r = correlate_dev(matrix, cols, xg, ctx)
    else:
        keep = np.zeros(0, np.int64)
        r = dict(n_kept=np.zeros(0, np.int32), mean=np.zeros(0, np.float32), med=np.zeros(0, np.float32),
                 rho=np.zeros(0), p=np.zeros(0), corrected=np.zeros(0))
    _cli.write_event_table(args.outputFile, "event\tn\tmean\tmedian\trho\tp-value\tcorrected", rows, keep,
                           [r["n_kept"], r["mean"], r["med"], r["rho"], r["p"], r["corrected"]], [".0f"] + ["repr"] * 5,
                           args.annotation)


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
