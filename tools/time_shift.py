#!/usr/bin/env python3
"""Time shift_dev (sdice_shift_dev: the Hodges-Lehmann shift with its confidence interval) beside ranksum_dev
reading the same table, in one process:

    python tools/time_shift.py [--reps 21] [--out profiles/shift_times.json]

Tables: 1 M rows x (8 v 8), 1 M x (50 v 50), 1 M x (500 v 500); the two groups are the two halves of the columns.  Each size
twice: 3-decimal PS values (what compare_sample_sets reads: the integer paths of the kernels) and uniform float32 values
off the grid (the float64 bisection), both with 2 % NaN; a block of rows repeated.  HIP events on the context stream
through sdice_timer_*, one event pair per launch, two warm-up launches, then the median of `reps`.  Per table: the two
times, the table bytes (n * s * 4) over the time as a fraction of 8 TB/s, and the ratio of the shift time to the rank-sum
time of the same run -- the unchanged rank-sum call is the yardstick.  Prints one JSON document (and writes it to
--out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import RANKSUM_FIELDS, SHIFT_FIELDS, Context, field_shapes

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(20)

results = []
for n, m, blk in ((1_000_000, 8, 25_000), (1_000_000, 50, 25_000), (1_000_000, 500, 5_000)):
    for grid in (True, False):
        s = 2 * m
        d_ps = resident_table(ctx, host_block(rng, blk, s, grid=grid), n)
        g1, g2 = np.arange(0, m, dtype=np.int32), np.arange(m, s, dtype=np.int32)
        d_g1, d_g2 = ctx.to_device(g1, np.int32), ctx.to_device(g2, np.int32)
        plain = {x: ctx.empty(*sd) for x, sd in field_shapes(RANKSUM_FIELDS, n).items()}
        out = {x: ctx.empty(*sd) for x, sd in field_shapes(SHIFT_FIELDS, n).items()}
        row = dict(rows=n, samples=s, group=m, values="3-decimal" if grid else "off the grid", reps=args.reps)
        calls = dict(ranksum_dev=(lambda: ctx.ranksum_dev(d_ps, d_g1, d_g2, plain), plain),
                     shift_dev=(lambda: ctx.shift_dev(d_ps, d_g1, d_g2, out), out))
        for name, (call, fields) in calls.items():
            med, lo, hi = timed(ctx, call, args.reps)
            row[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(fields["tested"].to_host().sum()),
                             hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
        row["shift_dev"]["ratio_to_ranksum"] = row["shift_dev"]["median_ms"] / row["ranksum_dev"]["median_ms"]
        results.append(row)
        for a in (d_ps, d_g1, d_g2, *plain.values(), *out.values()):
            a.free()
emit(ctx, results, args.out)
ctx.close()
