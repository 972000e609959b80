"""What the tools/time_*.py scripts share: the command line, a block of PS values repeated into a resident table, HIP-event
timing of one call and the JSON document."""
import argparse
import json

import numpy as np

HBM_BYTES_PER_S = 8e12


def parse_args(more=None):
    """--reps (at least 20) and --out; more(parser) adds a tool's own flags"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    if more is not None:
        more(ap)
    args = ap.parse_args()
    assert args.reps >= 20
    return args


def host_block(rng, blk, s, grid=True, nan=0.02, top=1000):
    """blk x s PS values: 3-decimal values 0.000 .. top / 1000 (grid) or uniform float32, a share `nan` of them NaN"""
    if grid:
        block = (rng.integers(0, top + 1, size=(blk, s)) / 1000.0).astype(np.float32)
    else:
        block = rng.random((blk, s), dtype=np.float32)
    if nan:
        block[rng.random((blk, s)) < nan] = np.nan
    return block


def resident_table(ctx, block, n):
    """the block repeated into n rows of device memory"""
    blk, s = block.shape
    assert n % blk == 0
    d = ctx.empty((n, s), block.dtype)
    for a in range(0, n, blk):
        d.offset(a * s, (blk, s)).upload(block)
    return d


def timed(ctx, call, reps, warmup=2):
    """HIP events on the context stream, one event pair per launch -> (median, min, max) in ms"""
    for _ in range(warmup):
        call()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def emit(ctx, results, out, hbm=True):
    """print the JSON document and write it to `out` when given"""
    doc = dict(device=ctx.device_info()["name"].strip())
    if hbm:
        doc["hbm_peak_bytes_per_s"] = HBM_BYTES_PER_S
    doc["results"] = results
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
