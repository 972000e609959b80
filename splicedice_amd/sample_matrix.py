"""`splicedice sample_matrix`: which samples of an `_allPS.tsv` look alike -- the sample x sample Pearson correlation and
root-mean-square PS difference over the junctions two samples share, the input of hierarchical clustering, MDS or PCA and
the first look for batch effects, swapped or duplicated samples and outlier libraries.  Not part of the reference;
DESIGN.md section 7.

    splicedice sample_matrix --psiSPLICEDICE t_allPS.tsv -o PREFIX [-s samples.txt] [--minShared N]

Writes three square tables, header `sample<TAB>name...` and one row per sample in the same order:
PREFIX_sampleCorrelation.tsv (float64), PREFIX_sampleDistance.tsv (float64, in PS units) and PREFIX_sampleShared.tsv
(the number of junctions both samples have).  A pair with fewer than --minShared shared junctions is `nan` in the first two,
and so is the correlation of a sample that is constant over the shared junctions.  The statistics are pairwise-complete,
as pandas' DataFrame.corr(), and exact: the table's values lie on the 3-decimal grid, so every sum is an integer.

On the GPU: sdice_sample_gram (the four integer matrices); on the host: sdice_sample_matrix_finish.
"""
import sys

import numpy as np

from . import _cli
from ._cli import read_ps_table, table_header_names
from .engine import GRAM_FIELDS, Context, SdiceError, field_shapes, sample_matrix_finish

MIN_SAMPLES = 2
MAX_SAMPLES = 4096                  # columns one sdice_sample_gram call takes (include/sdice.h)

MULTI_RANK_REFUSAL = ("sample_matrix: not available under the multi-rank launcher (the sums are additive over row ranges, "
                      "but no exchange for them exists yet); run it in one process.")


refuse = _cli.refusal("sample_matrix")


def read_samples(path):
    """the -s file -> [sample names] in file order: the first whitespace-separated token of every non-blank line; prints
    why and exits with status 1 on a name listed twice"""
    names, seen = [], set()
    with open(path) as fin:
        for lineno, line in enumerate(fin, 1):
            cells = line.split()
            if not cells:
                continue
            if cells[0] in seen:
                refuse(f"{path} line {lineno}: sample {cells[0]!r} is listed twice")
            seen.add(cells[0])
            names.append(cells[0])
    return names


def sample_columns(names, header_names):
    """the chosen samples (None: every column in table order) and the table's column names -> (names, int32 column index of
    each); prints why and exits with status 1 when a sample is not exactly once in the header or their number is outside
    2..4096"""
    if names is None:
        names = list(header_names)
    if len(names) < MIN_SAMPLES:
        refuse(f"cannot compare fewer than {MIN_SAMPLES} samples (got {len(names)})")
    if len(names) > MAX_SAMPLES:
        refuse(f"{len(names)} samples, at most {MAX_SAMPLES} are supported")
    return names, _cli.columns_in_header(names, header_names, refuse)


def gram_dev(matrix, cols, ctx):
    """table up, the four integer matrices on resident buffers, matrices down -> dict of int64 [m, m]"""
    return _cli.device_call(ctx, dict(ps=(matrix, np.float32), cols=(cols, np.int32)),
                            field_shapes(GRAM_FIELDS, (cols.size, cols.size)),
                            lambda d, out: ctx.sample_gram_dev(d["ps"], d["cols"], out))


def add_parser(parser):
    parser.add_argument("--psiSPLICEDICE", type=str, required=True,
                        help="PS table (_allPS.tsv) from 'splicedice quant'.")
    parser.add_argument("-s", "--samples", type=str, required=False, default="", metavar="FILE",
                        help="One sample name per line (the first token): selects and orders the samples; default: every "
                             "column in table order")
    parser.add_argument("--minShared", type=int, required=False, default=3,
                        help="Fewest shared junctions a sample pair needs for a value (default 3)")
    parser.add_argument("-o", "--outputPrefix", type=str, required=True,
                        help="Prefix of the three output tables")


def run_with(args, ctx=None):
    from . import _stages, mgpu, textio
    L = mgpu.launcher()             # (reads the torchrun environment before any GPU call)
    _cli.refuse_multi_rank(L, MULTI_RANK_REFUSAL)
    if args.minShared < 1:
        refuse(f"--minShared must be at least 1 (got {args.minShared})")
    chosen = read_samples(args.samples) if args.samples else None
    names, cols = sample_columns(chosen, table_header_names(args.psiSPLICEDICE))     # (exits before any GPU call)
    with _stages.stage("parse"):
        _, _, matrix = read_ps_table(args.psiSPLICEDICE, as_table=True)
    with _cli.engine_scope(ctx, lambda: Context(L.local_rank)) as ctx:
        try:
            sums = gram_dev(matrix, cols, ctx)
        except SdiceError as e:         # a value off the 3-decimal grid: the library's line
            print(f"sample_matrix: {e}", file=sys.stderr)
            sys.exit(1)
    corr, rmsd = sample_matrix_finish(sums["shared"], sums["sum1"], sums["sum2"], sums["prod"], args.minShared)
    header = "sample\t" + "\t".join(names) + "\n"
    with _stages.stage("format+write"):
        textio.write_table(args.outputPrefix + "_sampleCorrelation.tsv", header, names, corr, "repr")
        textio.write_table(args.outputPrefix + "_sampleDistance.tsv", header, names, rmsd, "repr")
        textio.write_table(args.outputPrefix + "_sampleShared.tsv", header, names, sums["shared"].astype(np.int32), ".0f")


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser()
    add_parser(p)
    run_with(p.parse_args())
