#!/usr/bin/env python3
"""Time kruskal_dev (Kruskal-Wallis across k sets) beside ranksum_dev reading the same table, in one process:

    python tools/time_kruskal.py [--reps 21] [--out profiles/kruskal_times.json]

Shapes: 1 M x 100 as 2 x 50 and 4 x 25 sets, 625 k x 1000 as 2 x 500 and 10 x 100; ranksum_dev on the two 2-set shapes.
Tables hold 3-decimal PS values with 2 % NaN (what compare_sample_sets reads; a 25 000-row block repeated).  HIP events on
the context stream through sdice_timer_*, one event pair per launch, two warm-up launches, then the median of `reps`.
Per shape: time, the table bytes (n * s * 4) over the time as a fraction of 8 TB/s, and for k = 2 the ratio to the
rank-sum time -- the existing counting kernel is the yardstick.  Prints one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import KRUSKAL_FIELDS, Context, field_shapes, kruskal_sets

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(11)

results = []
for n, s, splits in ((1_000_000, 100, (2, 4)), (625_000, 1000, (2, 10))):
    d_ps = resident_table(ctx, host_block(rng, 25_000, s), n)
    rs_ms = None
    for k in splits:
        sets = [np.arange(i * (s // k), (i + 1) * (s // k), dtype=np.int32) for i in range(k)]
        cols, set_ptr = kruskal_sets(sets, s)
        d_cols = ctx.to_device(cols, np.int32)
        out = {x: ctx.empty(*sd) for x, sd in field_shapes(KRUSKAL_FIELDS, n, k).items()}
        med, lo, hi = timed(ctx, lambda: ctx.kruskal_dev(d_ps, d_cols, set_ptr, out), args.reps)
        tested = int(out["tested"].to_host().sum())
        row = dict(call="kruskal_dev", rows=n, samples=s, sets=k, set_size=s // k, reps=args.reps, median_ms=med, min_ms=lo,
                   max_ms=hi, tested_rows=tested, hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S)
        if k == 2:
            d_g1, d_g2 = ctx.to_device(sets[0], np.int32), ctx.to_device(sets[1], np.int32)
            rout = dict(tested=out["tested"], p=out["p"], z=out["h"], **{x: ctx.empty(n, np.float32) for x in
                                                                         ("med1", "med2", "mean1", "mean2", "delta")})
            rmed, rlo, rhi = timed(ctx, lambda: ctx.ranksum_dev(d_ps, d_g1, d_g2, rout), args.reps)
            rs_ms = rmed
            results.append(dict(call="ranksum_dev", rows=n, samples=s, sets=2, set_size=s // 2, reps=args.reps, median_ms=rmed,
                                min_ms=rlo, max_ms=rhi, hbm_fraction=n * s * 4 / (rmed * 1e-3) / HBM_BYTES_PER_S))
            row["ratio_to_ranksum"] = med / rmed
            for a in (d_g1, d_g2, *[rout[x] for x in ("med1", "med2", "mean1", "mean2", "delta")]):
                a.free()
        else:
            row["ratio_to_ranksum_at_k2"] = med / rs_ms
        results.append(row)
        for a in (d_cols, *out.values()):
            a.free()
    d_ps.free()
emit(ctx, results, args.out)
ctx.close()
