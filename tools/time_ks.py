#!/usr/bin/env python3
"""Time ks_dev (the two-sample Kolmogorov-Smirnov test; asymptotic, then with exact p asked for) beside ranksum_dev
reading the same table, in one process:

    python tools/time_ks.py [--reps 21] [--out profiles/ks_times.json]

Tables: 1 M rows x (8 v 8), 1 M x (50 v 50), 100 k x (500 v 500); the two groups are the two halves of the columns.  Tables
hold 3-decimal PS values with 2 % NaN (what compare_sample_sets reads; a block of rows repeated).  HIP events on the
context stream through sdice_timer_*, one event pair per launch, two warm-up launches, then the median of `reps`.  Per
table: the three times, the table bytes (n * s * 4) over the time as a fraction of 8 TB/s, the rows that carry an exact p,
and the ratio of each KS time to the rank-sum time of the same run -- the unchanged rank-sum call is the yardstick.  Prints
one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import KS_FIELDS, RANKSUM_FIELDS, Context, field_shapes

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(19)

results = []
for n, m, blk in ((1_000_000, 8, 25_000), (1_000_000, 50, 25_000), (100_000, 500, 5_000)):
    s = 2 * m
    d_ps = resident_table(ctx, host_block(rng, blk, s), n)
    g1, g2 = np.arange(0, m, dtype=np.int32), np.arange(m, s, dtype=np.int32)
    d_g1, d_g2 = ctx.to_device(g1, np.int32), ctx.to_device(g2, np.int32)
    out = {x: ctx.empty(*sd) for x, sd in field_shapes(KS_FIELDS, n).items()}
    out["z"] = ctx.empty(*field_shapes(RANKSUM_FIELDS, n)["z"])
    row = dict(rows=n, samples=s, group=m, reps=args.reps)
    calls = dict(ranksum_dev=lambda: ctx.ranksum_dev(d_ps, d_g1, d_g2, out),
                 ks_dev=lambda: ctx.ks_dev(d_ps, d_g1, d_g2, out),
                 ks_dev_exact=lambda: ctx.ks_dev(d_ps, d_g1, d_g2, out, exact=True))
    for name, call in calls.items():
        med, lo, hi = timed(ctx, call, args.reps)
        row[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()),
                         hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
        if name != "ranksum_dev":
            row[name]["exact_rows"] = int(out["exact"].to_host().sum())
            row[name]["ratio_to_ranksum"] = med / row["ranksum_dev"]["median_ms"]
    results.append(row)
    for a in (d_ps, d_g1, d_g2, *out.values()):
        a.free()
emit(ctx, results, args.out)
ctx.close()
