#!/usr/bin/env python3
"""Time the exact calls of compare_sample_sets --exact (ranksum_exact_dev, signedrank_exact_dev) beside the asymptotic
calls (ranksum_dev, signedrank_dev) on the same tables, in one process:

    python tools/time_exact.py [--reps 21] [--rows 1000000] [--only NAME] [--out profiles/exact_times.json]

Tables: 1 M rows x (3 v 3), (8 v 8), (16 v 16) for the rank-sum pair, 1 M rows x 10 and 31 pairs for the signed-rank pair;
pair q is (column q, column m + q), the rank-sum groups are the same two column ranges.  Tables hold 3-decimal PS values
drawn from 0.000 .. 0.050, so nearly every row has ties (a block of rows repeated), without NaNs: every row is eligible.
HIP events on the context stream through sdice_timer_*, one event pair per launch, two warm-up launches, then the median of
`reps`.  The exact call runs the asymptotic call first and then its own kernel, so its time contains the comparator's; the
ratio is exact / asymptotic of the same run.  --only NAME (3v3, 8v8, 16v16, 10pairs, 31pairs) times one table, so that a
job script can give every table a time limit of its own; a run with --out merges its rows into the file that is there.
Prints one JSON document."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import emit, host_block, parse_args, resident_table, timed
from splicedice_amd.engine import RANKSUM_EXACT_FIELDS, Context, field_shapes

TABLES = {"3v3": (False, 3), "8v8": (False, 8), "16v16": (False, 16), "10pairs": (True, 10), "31pairs": (True, 31)}


def flags(ap):
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--only", choices=sorted(TABLES), default=None)


args = parse_args(flags)
ctx = Context(0)
rng = np.random.default_rng(17)

results = []
for name, (paired, m) in TABLES.items():
    if args.only not in (None, name):
        continue
    n, s = args.rows, 2 * m
    d_ps = resident_table(ctx, host_block(rng, 25_000, s, nan=0, top=50), n)
    g1, g2 = np.arange(0, m, dtype=np.int32), np.arange(m, s, dtype=np.int32)
    d_g1, d_g2 = ctx.to_device(g1, np.int32), ctx.to_device(g2, np.int32)
    out = {x: ctx.empty(*sd) for x, sd in field_shapes(RANKSUM_EXACT_FIELDS, n).items()}
    plain, exact = ("signedrank_dev", "signedrank_exact_dev") if paired else ("ranksum_dev", "ranksum_exact_dev")
    row = dict(table=name, test="signed-rank" if paired else "rank-sum", rows=n, samples=s, reps=args.reps)
    for key, call in (("asymptotic", plain), ("exact", exact)):
        med, lo, hi = timed(ctx, lambda: getattr(ctx, call)(d_ps, d_g1, d_g2, out), args.reps)
        row[key] = dict(call=call, median_ms=med, min_ms=lo, max_ms=hi, tested_rows=int(out["tested"].to_host().sum()))
    row["exact"]["exact_rows"] = int(out["exact"].to_host().sum())
    row["ratio_exact_to_asymptotic"] = row["exact"]["median_ms"] / row["asymptotic"]["median_ms"]
    results.append(row)
    for a in (d_ps, d_g1, d_g2, *out.values()):
        a.free()
if args.out and os.path.exists(args.out):
    old = json.load(open(args.out))
    if old.get("device") == ctx.device_info()["name"].strip():
        results = [r for r in old["results"] if r["table"] not in {x["table"] for x in results}] + results
        results.sort(key=lambda r: list(TABLES).index(r["table"]))
emit(ctx, results, args.out, hbm=False)
ctx.close()
