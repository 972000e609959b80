#!/usr/bin/env python3
"""Time spearman_dev (Spearman rank correlation of PS with a sample covariate) beside ranksum_dev reading the same table,
in one process:

    python tools/time_spearman.py [--reps 21] [--out profiles/spearman_times.json]

Tables: 1 M rows x 16, 1 M x 100, 100 k x 1000, 20 k x 4096 samples; the covariate lists every column (a quarter as many
distinct values as samples, so it has ties), the rank-sum groups are the two halves of the columns.  Tables hold 3-decimal
PS values with 2 % NaN (what `correlate` reads; a block of rows repeated).  HIP events on the context stream through
sdice_timer_*, one event pair per launch, two warm-up launches, then the median of `reps`.  Per table: both times, the
table bytes (n * s * 4) over the time as a fraction of 8 TB/s, and the ratio of the Spearman time to the rank-sum time of
the same run -- the unchanged rank-sum call is the yardstick.  Prints one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import RANKSUM_FIELDS, SPEARMAN_FIELDS, Context, field_shapes, spearman_order

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(14)

results = []
for n, s, blk in ((1_000_000, 16, 25_000), (1_000_000, 100, 25_000), (100_000, 1000, 5_000), (20_000, 4096, 1_000)):
    d_ps = resident_table(ctx, host_block(rng, blk, s), n)
    g1, g2 = np.arange(0, s // 2, dtype=np.int32), np.arange(s // 2, s, dtype=np.int32)
    d_g1, d_g2 = ctx.to_device(g1, np.int32), ctx.to_device(g2, np.int32)
    cols, xg = spearman_order(np.arange(s), rng.integers(0, max(2, s // 4), size=s))
    d_cols, d_xg = ctx.to_device(cols, np.int32), ctx.to_device(xg, np.int32)
    rs_out = {x: ctx.empty(*sd) for x, sd in field_shapes(RANKSUM_FIELDS, n).items()}
    sp_out = {x: ctx.empty(*sd) for x, sd in field_shapes(SPEARMAN_FIELDS, n).items()}
    row = dict(rows=n, samples=s, reps=args.reps)
    for name, call, out in (("ranksum_dev", lambda: ctx.ranksum_dev(d_ps, d_g1, d_g2, rs_out), rs_out),
                            ("spearman_dev", lambda: ctx.spearman_dev(d_ps, d_cols, d_xg, sp_out), sp_out)):
        med, lo, hi = timed(ctx, call, args.reps)
        row[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()),
                         hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
    row["ratio_to_ranksum"] = row["spearman_dev"]["median_ms"] / row["ranksum_dev"]["median_ms"]
    results.append(row)
    for a in (d_ps, d_g1, d_g2, d_cols, d_xg, *rs_out.values(), *sp_out.values()):
        a.free()
emit(ctx, results, args.out)
ctx.close()
