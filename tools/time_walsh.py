#!/usr/bin/env python3
"""Time walsh_resident (sdice_walsh_dev: the paired shift with its confidence interval) beside signedrank_dev and shift_dev
reading the same table, in one process:

    python tools/time_walsh.py [--reps 21] [--out profiles/walsh_times.json]

Tables: 1 M rows x 8, 50 and 500 pairs (16, 100 and 1000 columns); pair q is (column q, column m + q), and the two groups of
the shift call are the same two halves (8 v 8, 50 v 50, 500 v 500).  Each size twice: 3-decimal PS values (what
compare_sample_sets reads: the integer paths of the kernels) and uniform float32 values off the grid (the float64
bisection), both with 2 % NaN; a block of rows repeated.  HIP events on the context stream through sdice_timer_*, one event
pair per launch, two warm-up launches of each call, then the three calls ALTERNATED `reps` times and the median of each.
Per table: the three times, the table bytes (n * s * 4) over the time as a fraction of 8 TB/s, and the ratios of the walsh
time to the other two of the same run -- the unchanged calls are the yardsticks.  Prints one JSON document (and writes it to
--out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table
from splicedice_amd.engine import RANKSUM_FIELDS, SHIFT_FIELDS, WALSH_FIELDS, Context, field_shapes

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(22)

results = []
for n, m, blk in ((1_000_000, 8, 25_000), (1_000_000, 50, 25_000), (1_000_000, 500, 5_000)):
    for grid in (True, False):
        s = 2 * m
        d_ps = resident_table(ctx, host_block(rng, blk, s, grid=grid), n)
        d_a, d_b = ctx.to_device(np.arange(0, m, dtype=np.int32), np.int32), ctx.to_device(np.arange(m, s, dtype=np.int32), np.int32)
        outs = {name: {x: ctx.empty(*sd) for x, sd in field_shapes(fields, n).items()}
                for name, fields in (("walsh_resident", WALSH_FIELDS), ("signedrank_dev", RANKSUM_FIELDS), ("shift_dev", SHIFT_FIELDS))}
        calls = dict(walsh_resident=lambda: ctx.walsh_resident(d_ps, d_a, d_b, outs["walsh_resident"]),
                     signedrank_dev=lambda: ctx.signedrank_dev(d_ps, d_a, d_b, outs["signedrank_dev"]),
                     shift_dev=lambda: ctx.shift_dev(d_ps, d_a, d_b, outs["shift_dev"]))
        for call in calls.values():
            call()
            call()
        ctx.sync()
        ms = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, call in calls.items():
                ctx.timer_start()
                call()
                ms[name].append(ctx.timer_stop())
        row = dict(rows=n, samples=s, pairs=m, values="3-decimal" if grid else "off the grid", reps=args.reps)
        for name, t in ms.items():
            med = float(np.median(t))
            row[name] = dict(median_ms=med, min_ms=float(min(t)), max_ms=float(max(t)),
                             tested_rows=int(outs[name]["tested"].to_host().sum()),
                             hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
        for other in ("signedrank_dev", "shift_dev"):
            row["walsh_resident"]["ratio_to_" + other[:-4]] = row["walsh_resident"]["median_ms"] / row[other]["median_ms"]
        results.append(row)
        for d in (d_ps, d_a, d_b, *(x for o in outs.values() for x in o.values())):
            d.free()
emit(ctx, results, args.out)
ctx.close()
