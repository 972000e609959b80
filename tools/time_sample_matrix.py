#!/usr/bin/env python3
"""Time sample_gram_dev (the sample-by-sample integer sums of `sample_matrix`) on resident tables, in one process:

    python tools/time_sample_matrix.py [--reps 21] [--out profiles/sample_matrix_times.json]

Tables: 2 M rows x 500 samples and 200 k x 1000, every column selected in a random order; 3-decimal PS values with 20 % NaN
(a block of rows repeated).  HIP events on the context stream through sdice_timer_*, one event pair per call, two warm-up
calls, then the median of `reps`; the call contains its one host synchronisation (the bad-value check).  The pre-pass and
the tile kernel are then timed apart through the library's per-kernel events (prof_report) over `reps` further calls.
Per table: the times, the multiply-adds the sums need (3 per ordered pair and row: n * m^2 * 3) and the ones the tile
kernel issues (whole 64 x 64 tiles, 6 per pair of an off-diagonal tile and 4 on a diagonal one), each per second of the
tile kernel, beside the vector integer issue ceiling (compute units x 128 lanes x 2.4 GHz, the FP32 vector FMA rate).

The CPU comparator is the referee's recipe -- four float64 BLAS products of the masked key / key^2 / mask matrices -- with
16 threads on this host at a row count it finishes in seconds, scaled linearly to the table's rows and labelled as scaled.
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time
os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from splicedice_amd.engine import GRAM_FIELDS, Context

LANES_PER_CU_CLOCK = 128
CLOCK_HZ = 2.4e9
NAMES = [name for name, _ in GRAM_FIELDS]
TILE = 64

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--out", default="")
ap.add_argument("--cpu-rows", type=int, default=20_000)
args = ap.parse_args()
assert args.reps >= 20

ctx = Context(0)
info = ctx.device_info()
ceiling = info["compute_units"] * LANES_PER_CU_CLOCK * CLOCK_HZ
rng = np.random.default_rng(15)


def block_of(blk, s):
    block = (rng.integers(0, 1001, size=(blk, s)) / 1000.0).astype(np.float32)
    block[rng.random((blk, s)) < 0.2] = np.nan
    return block


def cpu_comparator(block, cols, n):
    """seconds of the four masked float64 products on the block's rows (best of 3), scaled to n rows"""
    sub = block[:args.cpu_rows, cols]
    best = np.inf
    for _ in range(3):
        t0 = time.perf_counter()
        V = (~np.isnan(sub)).astype(np.float64)
        K = np.where(np.isnan(sub), 0.0, np.rint(sub.astype(np.float64) * 1000.0))
        out = (V.T @ V, K.T @ V, (K * K).T @ V, K.T @ K)
        best = min(best, time.perf_counter() - t0)
    assert out[0].shape == (cols.size, cols.size)
    return dict(rows_timed=int(sub.shape[0]), seconds_timed=best, scaled_to_rows=n, seconds_scaled=best * n / sub.shape[0],
                threads=int(os.environ["OMP_NUM_THREADS"]), note="scaled linearly from rows_timed, not run at full size")


results = []
for n, s, blk in ((2_000_000, 500, 20_000), (200_000, 1000, 20_000)):
    block = block_of(blk, s)
    d_ps = ctx.empty((n, s), np.float32)
    assert n % blk == 0
    for a in range(0, n, blk):
        d_ps.offset(a * s, (blk, s)).upload(block)
    cols = rng.permutation(s).astype(np.int32)
    m = cols.size
    d_cols = ctx.to_device(cols, np.int32)
    out = {k: ctx.empty((m, m), np.int64) for k in NAMES}

    def call():
        ctx.sample_gram_dev(d_ps, d_cols, out)

    for _ in range(2):
        call()
    ctx.sync()
    ms = []
    for _ in range(args.reps):
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    ctx.prof_enable(1)
    ctx.prof_reset()
    for _ in range(args.reps):
        call()
    ctx.sync()
    prof = ctx.prof_report()
    ctx.prof_enable(0)
    per_kernel = {k: v[1] / v[0] for k, v in prof.items() if k.startswith("gram_")}
    # the sums of a repeated block are the block's times the repeat count: a check that costs one small referee product
    got = out["shared"].to_host()
    V = (~np.isnan(block[:, cols])).astype(np.float64)
    assert np.array_equal(got, (V.T @ V).astype(np.int64) * (n // blk)), "shared does not match the block's sums"
    nt = -(-m // TILE)
    needed = 3.0 * n * m * m
    issued = float(n) * TILE * TILE * (6 * nt * (nt - 1) / 2 + 4 * nt)
    tile_s = per_kernel["gram_tile_kernel"] * 1e-3
    row = dict(rows=n, samples=m, reps=args.reps,
               call=dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms))),
               kernel_ms=per_kernel, madds_needed=needed, madds_issued=issued,
               needed_madds_per_s=needed / tile_s, issued_madds_per_s=issued / tile_s,
               issued_fraction_of_ceiling=issued / tile_s / ceiling, needed_fraction_of_ceiling=needed / tile_s / ceiling,
               key_table_bytes=n * nt * TILE * 2, cpu_blas_float64=cpu_comparator(block, cols, n))
    row["cpu_scaled_over_gpu_call"] = row["cpu_blas_float64"]["seconds_scaled"] / (row["call"]["median_ms"] * 1e-3)
    results.append(row)
    for a in (d_ps, d_cols, *out.values()):
        a.free()
doc = dict(device=info["name"].strip(), compute_units=info["compute_units"],
           valu_int_ceiling_madds_per_s=ceiling, ceiling_is="compute units x 128 lanes per clock x 2.4 GHz", results=results)
text = json.dumps(doc, indent=1)
print(text, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
ctx.close()
