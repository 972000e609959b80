#!/usr/bin/env python3
"""Time jonckheere_dev (Jonckheere-Terpstra across k ordered sets) beside kruskal_dev reading the same table with the same
sets, in one process:

    python tools/time_jonckheere.py [--reps 21] [--out profiles/jonckheere_times.json]

Shapes: 1 M x 100 as 4 x 25 and 625 k x 1000 as 10 x 100 (those of tools/time_kruskal.py), 1 M x 150 as 3 x 50.  Tables hold
3-decimal PS values with 2 % NaN (what compare_sample_sets reads; a 25 000-row block repeated), so both calls run their
histogram kernels.  HIP events on the context stream through sdice_timer_*, one event pair per launch, two warm-up launches,
then the median of `reps`.  Per shape: both times, their ratio -- the existing Kruskal-Wallis kernel is the yardstick -- and
the table bytes (n * s * 4) over the time as a fraction of 8 TB/s.  The sorting kernels are timed once each on an off-grid
table of 10 000 x 300 as 3 x 100, no target.  Prints one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import JONCKHEERE_FIELDS, KRUSKAL_FIELDS, Context, field_shapes, kruskal_sets

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(11)

results = []
for n, s, k, grid in ((1_000_000, 100, 4, True), (625_000, 1000, 10, True), (1_000_000, 150, 3, True), (10_000, 300, 3, False)):
    d_ps = resident_table(ctx, host_block(rng, min(25_000, n), s, grid), n)
    sets = [np.arange(i * (s // k), (i + 1) * (s // k), dtype=np.int32) for i in range(k)]
    cols, set_ptr = kruskal_sets(sets, s)
    d_cols = ctx.to_device(cols, np.int32)
    times = {}
    for name, fields in (("kruskal_dev", KRUSKAL_FIELDS), ("jonckheere_dev", JONCKHEERE_FIELDS)):
        out = {x: ctx.empty(*sd) for x, sd in field_shapes(fields, n, k).items()}
        call = getattr(ctx, name)
        med, lo, hi = timed(ctx, lambda: call(d_ps, d_cols, set_ptr, out), args.reps)
        times[name] = med
        results.append(dict(call=name, kernel="histogram" if grid else "sorting", rows=n, samples=s, sets=k, set_size=s // k,
                            reps=args.reps, median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()),
                            hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S))
        for a in out.values():
            a.free()
    results[-1]["ratio_to_kruskal"] = times["jonckheere_dev"] / times["kruskal_dev"]
    for a in (d_cols, d_ps):
        a.free()
emit(ctx, results, args.out)
ctx.close()
