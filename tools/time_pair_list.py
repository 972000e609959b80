#!/usr/bin/env python3
"""Time the pair kernels -- all pairs and a caller's pair list -- with the library given on the command line, so that two
builds can be compared on one GPU inside one session:

    python tools/time_pair_list.py LIB allpairs [rows samples]     fisher_pairs_dev and chi2_pairs_dev, every pair
    python tools/time_pair_list.py LIB matched  [rows samples]     the list (0,1),(2,3),...: s/2 matched pairs
    python tools/time_pair_list.py LIB twoset   [rows samples]     the list A x B, A = first half of the samples, B = the rest

LIB may be a build of the commit before the pair-list entry points existed (build/base_lib/libsplicedice_hip.so, made
from a `git worktree` of that commit): this script then binds only the symbols that build has, and only `allpairs` runs.
Data as bench.py --workload pairwise (25 000 x 200 by default: the config-4 shard).  HIP events on the context stream,
one event pair per call; prints one JSON line with the median and the range of the calls."""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from _timing import resident_table, timed
from splicedice_amd import _ffi, synth

lib_path, mode = os.path.abspath(sys.argv[1]), sys.argv[2]
n, s = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (25_000, 200)
_ffi.LIB_PATH = lib_path
_probe = C.CDLL(lib_path)
missing = [name for name in _ffi.SIGNATURES if not hasattr(_probe, name)]
for name in missing:                       # (this process only; _ffi.load() itself stays strict)
    del _ffi.SIGNATURES[name]
if mode != "allpairs" and missing:
    sys.exit(f"{lib_path} lacks {missing}: only `allpairs` can be timed with it")
from splicedice_amd.engine import Context

ctx = Context(0)
blk = min(n, 25_000)
assert n % blk == 0
junc = synth.make_junctions(blk, 4)
counts_in = synth.make_counts(blk, s, 40)
row_of, row_ptr, col = ctx.cluster(*junc)
counts = np.zeros_like(counts_in)
counts[row_of] = counts_in
excl = ctx.ps(counts, row_ptr, col, want_excl=True, want_ps=False)
d_incl, d_excl = resident_table(ctx, counts, n), resident_table(ctx, excl, n)       # (the 25 000-row block repeated)
if mode == "allpairs":
    m, kw = s * (s - 1) // 2, {}
else:
    pairs = (np.arange(s - s % 2, dtype=np.int32).reshape(-1, 2) if mode == "matched" else
             np.stack(np.meshgrid(np.arange(s // 2), np.arange(s // 2, s), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32))
    m, kw = len(pairs), dict(pairs=ctx.pair_table(s, pairs))
d_p = ctx.empty((n, m), np.float64)
d_bad = ctx.empty(1, np.int64)
reps = 9 if n * m <= 1 << 30 else 3


def stats(call):
    med, lo, hi = timed(ctx, call, reps, warmup=1)
    return dict(median_ms=med, min_ms=lo, max_ms=hi, p_values_per_s=n * m / (med * 1e-3))


out = dict(lib=os.path.relpath(lib_path), mode=mode, rows=n, samples=s, pairs=m, reps=reps,
           fisher=stats(lambda: ctx.fisher_pairs_dev(d_incl, d_excl, d_p, **kw)),
           chi2=stats(lambda: ctx.chi2_pairs_dev(d_incl, d_excl, d_p, d_bad, **kw)))
print(json.dumps(out), flush=True)
ctx.close()
