#!/usr/bin/env python3
"""Time friedman_resident and page_resident (k matched sets) beside kruskal_dev reading the same table, in one process:

    python tools/time_friedman.py [--reps 21] [--out profiles/friedman_times.json]

Shapes: 1 M-row tables of 3 x 16, 4 x 8 and 8 x 8 columns (sets x subjects), 3-decimal PS values with 2 % NaN (a 25 000-row
block repeated).  The three calls are ALTERNATED: every repetition launches each of them once, so that a drift of the
clocks falls on all three alike -- which is why the event loop is written out here and is not _timing.timed, which times
one call at a time; HIP events on the context stream through sdice_timer_*, one event pair per launch, two
warm-up rounds, then the median of `reps`.  Nobody has set a time bar for this kernel: the record is the ratio to
kruskal_dev on the same table in the same run.  Prints one JSON document (and writes it to --out)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table
from splicedice_amd.engine import FRIEDMAN_FIELDS, KRUSKAL_FIELDS, PAGE_FIELDS, Context, field_shapes, friedman_columns, kruskal_sets

args = parse_args()
ctx = Context(0)
rng = np.random.default_rng(21)
n = 1_000_000

results = []
for k, m in ((3, 16), (4, 8), (8, 8)):
    s = k * m
    d_ps = resident_table(ctx, host_block(rng, 25_000, s), n)
    sets = [np.arange(j * m, (j + 1) * m, dtype=np.int32) for j in range(k)]
    cols, set_ptr = kruskal_sets(sets, s)
    assert np.array_equal(cols, friedman_columns(sets, s))              # (set-major is back to back: one list serves the three calls)
    d_cols = ctx.to_device(cols, np.int32)
    outs = {name: {x: ctx.empty(*sd) for x, sd in field_shapes(fields, n, k).items()}
            for name, fields in (("friedman_resident", FRIEDMAN_FIELDS), ("page_resident", PAGE_FIELDS), ("kruskal_dev", KRUSKAL_FIELDS))}
    calls = {"friedman_resident": lambda: ctx.friedman_resident(d_ps, d_cols, k, outs["friedman_resident"]),
             "page_resident": lambda: ctx.page_resident(d_ps, d_cols, k, outs["page_resident"]),
             "kruskal_dev": lambda: ctx.kruskal_dev(d_ps, d_cols, set_ptr, outs["kruskal_dev"])}
    ms = {name: [] for name in calls}
    for rep in range(-2, args.reps):                                    # two warm-up rounds
        for name, call in calls.items():
            ctx.timer_start()
            call()
            t = ctx.timer_stop()
            if rep >= 0:
                ms[name].append(t)
    kw = float(np.median(ms["kruskal_dev"]))
    for name in calls:
        med = float(np.median(ms[name]))
        results.append(dict(call=name, rows=n, samples=s, sets=k, subjects=m, reps=args.reps, median_ms=med, min_ms=float(min(ms[name])),
                            max_ms=float(max(ms[name])), tested_rows=int(outs[name]["tested"].to_host().sum()),
                            hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S, ratio_to_kruskal=med / kw))
    for a in (d_ps, d_cols, *[a for o in outs.values() for a in o.values()]):
        a.free()
emit(ctx, results, args.out)
ctx.close()
