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
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from splicedice_amd.engine import JONCKHEERE_FIELDS, KRUSKAL_FIELDS, Context, field_shapes, kruskal_sets

HBM_BYTES_PER_S = 8e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert args.reps >= 20

ctx = Context(0)
rng = np.random.default_rng(11)


def table(n, s, blk=25_000, grid=True):
    blk = min(blk, n)
    if grid:
        block = (rng.integers(0, 1001, size=(blk, s)) / 1000.0).astype(np.float32)
    else:
        block = rng.random((blk, s), dtype=np.float32)
    block[rng.random((blk, s)) < 0.02] = np.nan
    d = ctx.empty((n, s), np.float32)
    assert n % blk == 0
    for a in range(0, n, blk):
        d.offset(a * s, (blk, s)).upload(block)
    return d


def timed(call):
    for _ in range(2):
        call()
    ctx.sync()
    ms = []
    for _ in range(args.reps):
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), float(min(ms)), float(max(ms))


results = []
for n, s, k, grid in ((1_000_000, 100, 4, True), (625_000, 1000, 10, True), (1_000_000, 150, 3, True), (10_000, 300, 3, False)):
    d_ps = table(n, s, grid=grid)
    sets = [np.arange(i * (s // k), (i + 1) * (s // k), dtype=np.int32) for i in range(k)]
    cols, set_ptr = kruskal_sets(sets, s)
    d_cols = ctx.to_device(cols, np.int32)
    times = {}
    for name, fields in (("kruskal_dev", KRUSKAL_FIELDS), ("jonckheere_dev", JONCKHEERE_FIELDS)):
        out = {x: ctx.empty(*sd) for x, sd in field_shapes(fields, n, k).items()}
        call = getattr(ctx, name)
        med, lo, hi = timed(lambda: call(d_ps, d_cols, set_ptr, out))
        times[name] = med
        results.append(dict(call=name, kernel="histogram" if grid else "sorting", rows=n, samples=s, sets=k, set_size=s // k,
                            reps=args.reps, median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()),
                            hbm_fraction=n * s * 4 / (med * 1e-3) / HBM_BYTES_PER_S))
        for a in out.values():
            a.free()
    results[-1]["ratio_to_kruskal"] = times["jonckheere_dev"] / times["kruskal_dev"]
    for a in (d_cols, d_ps):
        a.free()
doc = dict(device=ctx.device_info()["name"].strip(), hbm_peak_bytes_per_s=HBM_BYTES_PER_S, results=results)
text = json.dumps(doc, indent=1)
print(text, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
ctx.close()
