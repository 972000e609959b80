#!/usr/bin/env python3
"""Time ranksum_strata_dev (van Elteren's stratified rank-sum test) beside ranksum_dev reading the same table, in one
process:

    python tools/time_strata.py [--reps 21] [--out profiles/strata_times.json]

Tables: 1 M rows x (8 v 8) in 2 strata, 1 M x (50 v 50) in 4 strata, 100 k x (500 v 500) in 8 strata; the two groups are
the two halves of the columns, the strata are dealt to the columns of each group in turn.  Tables hold 3-decimal PS values
with 2 % NaN (what compare_sample_sets reads; a block of rows repeated).  HIP events on the context stream through
sdice_timer_*, one event pair per launch, two warm-up launches, then the median of `reps`.  Per table: both times, the table
bytes (n * s * 4) over the time as a fraction of 8 TB/s, and the ratio of the stratified time to the rank-sum time of the
same run -- the unchanged rank-sum call is the yardstick.  Prints one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import RANKSUM_FIELDS, Context, field_shapes

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(17)

results = []
for n, m, H, blk in ((1_000_000, 8, 2, 25_000), (1_000_000, 50, 4, 25_000), (100_000, 500, 8, 5_000)):
    s = 2 * m
    d_ps = resident_table(ctx, host_block(rng, blk, s), n)
    g1, g2 = np.arange(0, m, dtype=np.int32), np.arange(m, s, dtype=np.int32)
    strat = (np.arange(m) % H).astype(np.int32)
    d_g1, d_g2, d_st = ctx.to_device(g1, np.int32), ctx.to_device(g2, np.int32), ctx.to_device(strat, np.int32)
    out = {x: ctx.empty(*sd) for x, sd in field_shapes(RANKSUM_FIELDS, n).items()}
    row = dict(rows=n, samples=s, group=m, strata=H, reps=args.reps)
    calls = dict(ranksum_dev=lambda: ctx.ranksum_dev(d_ps, d_g1, d_g2, out),
                 ranksum_strata_dev=lambda: ctx.ranksum_strata_dev(d_ps, d_g1, d_g2, d_st, d_st, H, out))
    for name, call in calls.items():
        med, lo, hi = timed(ctx, call, args.reps)
        row[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()),
                         hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
    row["ratio_to_ranksum"] = row["ranksum_strata_dev"]["median_ms"] / row["ranksum_dev"]["median_ms"]
    results.append(row)
    for a in (d_ps, d_g1, d_g2, d_st, *out.values()):
        a.free()
emit(ctx, results, args.out)
ctx.close()
