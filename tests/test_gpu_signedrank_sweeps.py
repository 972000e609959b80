"""sdice_signedrank sweeps: every rows-per-wave choice of the lane-group kernel's launch, 1 M-row tables past the grid
cap of the lane-per-row and the lane-group kernel (every row compared), sdice_signedrank_dev without the z output, and a p ladder from 1 down the tail at
1024 and 4096 pairs with z of either sign -- against tests/signedrank_referee.py under the bars of
tests/test_gpu_signedrank.py, whose tables and references are reused.

Big tables are a palette (the mixed table of that pair count, a few hundred distinct rows) fancy-indexed into n rows, so
the referee runs once per palette row.  Tests without the gpu mark check on the CPU that the tables are what they claim."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signedrank_referee as SR  # noqa: E402
from rank_support import NOMINAL_CUS, P_FLOOR, chunk_table_rows, draw_pairs, palette_index, scatter  # noqa: E402
from test_gpu_signedrank import OUTS, check, reference, table  # noqa: E402

gpu = pytest.mark.gpu

CHS = (64, 32, 16, 8, 4, 2, 1)
# (pairs, rows per wave chunk): all choices at 9 pairs (the lane-group kernel, 4 rows side by side in a wave: more than a
# chunk of 2 or 1 has), some at 17 (2 side by side) and 33 (1); the lane-per-row kernel of 8 and 3 pairs has no chunks,
# its tables are there for their length
CHUNK_CASES = tuple((9, ch) for ch in CHS) + ((17, 32), (33, 16), (8, 64), (8, 1), (3, 64))


@pytest.mark.parametrize("m,ch", CHUNK_CASES)
def test_chunk_tables_select_their_rows_per_wave(m, ch):
    """for a nominal 256 compute units: the table selects ch, ends in a partial chunk, uses every palette row, and the
    ch = 64 table has more chunks than the capped grid has waves (32 per compute unit)"""
    n = chunk_table_rows(ch, NOMINAL_CUS)
    idx = palette_index(n, table(m)[0].shape[0])
    assert np.unique(idx).size == table(m)[0].shape[0] and (idx[1:] != idx[:-1]).all()
    if ch == 64:
        assert n >= 1_000_000 and -(-n // 64) > 32 * NOMINAL_CUS and n > 256 * 8 * NOMINAL_CUS and n * (2 * m + 3) * 4 < 90e6


@gpu
@pytest.mark.parametrize("m,ch", CHUNK_CASES)
def test_signedrank_rows_per_wave(ctx, m, ch):
    """ch rows per wave chunk, 64 / P of them side by side: every row of every output against the referee.  The 8- and
    9-pair ch = 64 tables (1 M rows, grid-strided in either kernel) also go through sdice_signedrank_dev with the z output
    absent: tested, p and the float32 fields equal the host call's bit for bit."""
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    rows, a, b, _ = table(m)
    idx = palette_index(n, rows.shape[0])
    ps = np.ascontiguousarray(rows[idx])
    got = ctx.signedrank(ps, a, b)
    check(got, scatter(reference(m), idx), f"m={m} ch={ch} n={n} on {cus} CUs")
    if (m, ch) not in ((8, 64), (9, 64)):
        return
    assert -(-n // 64) > 32 * cus and n > 256 * 8 * cus           # more chunks than waves, more rows than lanes
    d_ps, d_a, d_b = ctx.to_device(ps), ctx.to_device(a, np.int32), ctx.to_device(b, np.int32)
    out = {name: ctx.empty(n, dt).memset(0x5A) for name, dt in SR.FIELDS if name != "z"}
    try:
        ctx.signedrank_dev(d_ps, d_a, d_b, out)
        for name in out:
            bad = np.flatnonzero(out[name].to_host().view(np.uint8) != got[name].view(np.uint8))
            assert bad.size == 0, ("sdice_signedrank_dev without z", name, bad.size, bad[:5].tolist())
    finally:
        for d in (d_ps, d_a, d_b, *out.values()):
            d.free()


# ------------------------------------------------------------------------------ the p ladder
LADDER_STEPS = 48
P_BANDS = ((1e-3, 1.0), (1e-20, 1e-3), (1e-100, 1e-20), (1e-200, 1e-100), (1e-280, 1e-200))


@functools.lru_cache(maxsize=None)
def ladder(m):
    """-> (ps float32[2 * 49, 2 m + 3], a, b): step t makes the share 0.5 + t / 96 of the differences positive (the last
    step all of them, with every |d| equal: the largest |z| = sqrt(m) there is); |d| are 1..400 thousandths, so tie runs
    are long.  Every step twice, the second time with the sides exchanged (z of the other sign); steps alternate between
    3-decimal values and the same values scaled off the grid."""
    rng = np.random.default_rng(7700 + m)
    a, b, s = draw_pairs(rng, m)
    rows = []
    for t in range(LADDER_STEPS + 1):
        ky = rng.integers(400, 601, size=m)
        mag = rng.integers(1, 401, size=m) if t < LADDER_STEPS else np.full(m, 7)
        pos = rng.permutation(m) < round(m * (0.5 + t / (2 * LADDER_STEPS)))
        x = ((ky + np.where(pos, mag, -mag)) / 1000.0).astype(np.float32)
        y = (ky / 1000.0).astype(np.float32)
        if t % 2:
            x, y = x * np.float32(1.7) - np.float32(0.3), y * np.float32(1.7) - np.float32(0.3)
        for u, v in ((x, y), (y, x)):
            row = np.full(s, np.nan, np.float32)
            row[a], row[b] = u, v
            rows.append(row)
    return np.stack(rows), a, b


@functools.lru_cache(maxsize=None)
def ladder_reference(m):
    return SR.table_reference(*ladder(m))


@pytest.mark.parametrize("m", [1024, 4096])
def test_ladder_covers_every_p_band(m):
    """the referee's p walks from above 1e-3 down: at 4096 pairs through every band and past the floor of 1e-280; at
    1024 pairs to the smallest p that pair count can give, erfc(sqrt(1024 / 2)) = 1.09e-224 (no row of at most 1100 pairs
    reaches the floor), so the last band is entered but the floor is not passed.  z comes in both signs, rows alternate
    between the two kinds."""
    ref = ladder_reference(m)
    assert ref["tested"].all() and (ref["z"][0::2] == -ref["z"][1::2]).all() and ref["z"][-2] > 0 > ref["z"][-1]
    assert ref["grid"].reshape(-1, 2).all(axis=1).tolist() == [t % 2 == 0 for t in range(LADDER_STEPS + 1)]
    p = ref["p"]
    for lo, hi in P_BANDS:
        need = 2 if (m, hi) == (1024, 1e-200) else 4          # (at 1024 pairs only the last step, in its two signs, gets there)
        assert ((p >= lo) & (p < hi)).sum() >= need, (m, lo, hi)
    assert abs(abs(ref["z"][-1]) - np.sqrt(m)) < 1e-9
    if m == 1024:
        assert p.min() >= P_FLOOR and abs(p.min() / 1.09e-224 - 1) < 0.01
    else:
        assert (p < P_FLOOR).sum() >= 8


@gpu
@pytest.mark.parametrize("m", [1024, 4096])
def test_signedrank_p_ladder(ctx, m):
    """(the 1 % rule is for the mixed tables: this table goes below the floor on purpose)"""
    ps, a, b = ladder(m)
    got = ctx.signedrank(ps, a, b)
    check(got, ladder_reference(m), f"ladder m={m}", floor_share=False)
    assert (got["z"][0::2] == -got["z"][1::2]).all()
    assert set(OUTS) == set(got)
