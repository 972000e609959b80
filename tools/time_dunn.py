#!/usr/bin/env python3
"""Time sdice_kruskal_dunn_dev (Kruskal-Wallis with Dunn's pair epilogue) beside sdice_kruskal_dev on the same table, and
sdice_kruskal_dev of this build against another build of the library (the parent commit's), alternated in one run:

    python tools/time_dunn.py [--reps 21] [--rounds 4] [--parent-lib build/base_lib/libsplicedice_hip.so]
                              [--out profiles/dunn_times.json]

Shapes: 1 M rows of 3-decimal PS values with 2 % NaN (a 25 000-row block repeated), k = 3 sets of 50 columns, 8 of 16 and
11 of 8.  HIP events on the context stream through sdice_timer_*, one event pair per call, two warm-up calls, then the
median of `reps`.

1. With --parent-lib: `rounds` times in turn, a fresh child process times kruskal_dev with the parent's library, then one
   with this build's (each child: every shape, its own table upload, its own warm-up).  Per shape the record holds every
   child's median, the median of those per build, and the parent's spread: the largest minus the smallest of the
   PARENT's own medians over its rounds -- the yardstick a difference between the builds has to exceed to mean anything.
2. In this process: kruskal_dev, then kruskal_dunn_dev with every output, with pair_p absent (NULL), with pair_padj
   absent and with both absent, on the same resident table; the extra bytes written per row (8 m with z alone, 24 m with
   all three) beside the extra time.  `every output` minus `pair_p NULL` is the cost of m 8-byte stores per row and
   nothing else (p is computed for padj either way); `pair_p NULL` minus both NULL is erfc, Holm and the padj stores.

Prints one JSON document (and writes it to --out)."""
import json
import os
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import HBM_BYTES_PER_S, emit, host_block, parse_args, resident_table, timed

ROWS = 1_000_000
SHAPES = ((3, 50), (8, 16), (11, 8))            # (sets, columns per set)


def _flags(ap):
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child-lib", default="",
                    help="internal: time kruskal_dev with this library on every shape and print one JSON line")


args = parse_args(_flags)

from splicedice_amd import _ffi  # noqa: E402
if args.child_lib:
    _ffi.LIB_PATH = os.path.abspath(args.child_lib)
    import ctypes  # noqa: E402
    probe = ctypes.CDLL(_ffi.LIB_PATH)
    for name in [x for x in _ffi.SIGNATURES if not hasattr(probe, x)]:          # (this process only: an older build lacks
        del _ffi.SIGNATURES[name]                                               # the newer symbols; _ffi.load() stays strict)
from splicedice_amd.engine import KRUSKAL_DUNN_FIELDS, KRUSKAL_FIELDS, Context, field_shapes, kruskal_sets  # noqa: E402


def shape_inputs(ctx, k, size):
    s = k * size
    d_ps = resident_table(ctx, host_block(np.random.default_rng(13 + k), 25_000, s), ROWS)
    sets = [np.arange(i * size, (i + 1) * size, dtype=np.int32) for i in range(k)]
    cols, set_ptr = kruskal_sets(sets, s)
    return d_ps, ctx.to_device(cols, np.int32), set_ptr


def kruskal_time(ctx, d_ps, d_cols, set_ptr, k):
    out = {x: ctx.empty(*sd) for x, sd in field_shapes(KRUSKAL_FIELDS, ROWS, k).items()}
    res = timed(ctx, lambda: ctx.kruskal_dev(d_ps, d_cols, set_ptr, out), args.reps)
    for a in out.values():
        a.free()
    return res


def child():
    ctx = Context(0)
    medians = {}
    for k, size in SHAPES:
        d_ps, d_cols, set_ptr = shape_inputs(ctx, k, size)
        medians[f"{k}x{size}"] = kruskal_time(ctx, d_ps, d_cols, set_ptr, k)[0]
        d_ps.free()
        d_cols.free()
    ctx.close()
    print("CHILD " + json.dumps(medians), flush=True)


def alternate(parent_lib, this_lib):
    """-> per shape: dict(parent_medians_ms, this_medians_ms, their medians, parent_spread_ms, difference_ms, within_spread)"""
    runs = {"parent": [], "this": []}
    for _ in range(args.rounds):
        for who, lib in (("parent", parent_lib), ("this", this_lib)):
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child-lib", lib],
                                  check=True, stdout=subprocess.PIPE, text=True)      # (the child's stderr goes to ours)
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")][-1]
            runs[who].append(json.loads(line[6:]))
    out = []
    for k, size in SHAPES:
        key = f"{k}x{size}"
        a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        ma, mb = float(np.median(a)), float(np.median(b))
        spread = max(a) - min(a)
        out.append(dict(call="kruskal_dev, parent build against this build", rows=ROWS, sets=k, set_size=size, reps=args.reps,
                        rounds=args.rounds, parent_medians_ms=a, this_medians_ms=b, parent_median_ms=ma, this_median_ms=mb,
                        parent_spread_ms=spread, difference_ms=mb - ma, within_parent_spread=bool(abs(mb - ma) <= spread)))
    return out


def main():
    results = []
    if args.parent_lib:
        results += alternate(os.path.abspath(args.parent_lib), _ffi.LIB_PATH)
    ctx = Context(0)
    for k, size in SHAPES:
        m = k * (k - 1) // 2
        d_ps, d_cols, set_ptr = shape_inputs(ctx, k, size)
        base = kruskal_time(ctx, d_ps, d_cols, set_ptr, k)
        table_bytes = ROWS * k * size * 4
        results.append(dict(call="kruskal_dev", rows=ROWS, sets=k, set_size=size, reps=args.reps, median_ms=base[0], min_ms=base[1],
                            max_ms=base[2], hbm_fraction=table_bytes / (base[0] * 1e-3) / HBM_BYTES_PER_S))
        out = {x: ctx.empty(*sd) for x, sd in field_shapes(KRUSKAL_DUNN_FIELDS, ROWS, k).items()}
        for label, absent, per_row in (("every output", (), 24 * m), ("pair_p NULL", ("pair_p",), 16 * m),
                                       ("pair_padj NULL", ("pair_padj",), 16 * m),
                                       ("pair_p and pair_padj NULL", ("pair_p", "pair_padj"), 8 * m)):
            handed = {x: d for x, d in out.items() if x not in absent}
            med, lo, hi = timed(ctx, lambda: ctx.kruskal_dunn_dev(d_ps, d_cols, set_ptr, handed), args.reps)
            results.append(dict(call="kruskal_dunn_dev, " + label, rows=ROWS, sets=k, set_size=size, pairs=m, reps=args.reps,
                                median_ms=med, min_ms=lo, max_ms=hi, ratio_to_kruskal=med / base[0], extra_ms=med - base[0],
                                extra_bytes_per_row=per_row, extra_bytes_over_table_bytes=per_row * ROWS / table_bytes,
                                tested_rows=int(out["tested"].to_host().sum())))
        for a in (d_ps, d_cols, *out.values()):
            a.free()
    emit(ctx, results, args.out)
    ctx.close()


if args.child_lib:
    child()
else:
    main()
