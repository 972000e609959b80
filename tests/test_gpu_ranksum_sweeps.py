"""Rank-sum sweeps: sdice_ranksum against oracle_np.compare_rows (scipy.stats.ranksums, np.median, np.mean) and mpmath at
the rows-per-wave choices, grid-stride passes, edge values, selection shapes and p tails that the random parity tables
of test_gpu_parity.py and the count sweeps of test_gpu_count_sweeps.py do not reach.

- A, rows per wave and grid stride: tables of 64 x compute_units x ch rows for ch = 64, 32, 8, 2 (the rule of
  launch_wave and of the re-do pass of launch_pairq, the same as sdice_kruskal_dev's) built by one fancy index from a
  palette of 320 rows of eight kinds, 20 v 24 of 48 columns.  The ch = 64 table (about 1.05 M rows) runs through every
  kernel class, ranksum.variant 0, 1, 4, 3, 5, 2, past the second grid-stride pass of each of them, and once more
  through sdice_ranksum_dev without z into outputs pre-filled with 0x5A.  Palettes of 70 v 90, 260 v 300 and 513 v 520
  columns at the ch = 2 size cover count<E> / wave<E> for E = 2, 8, 16;
- B, edge values: signed zeros, subnormals, values one ulp off the grid, values that clamp to keys 0 and 1000, 1e30,
  FLT_MAX, infinities, groups of exactly 3; embedded in 20 v 24 and 70 v 90 columns and in a table of 4099 columns;
- C, selection shapes: group sizes around every boundary of the auto dispatch, with the kernel that ran read back from
  the profiler;
- D, p: ladders of G v G columns (G = 1024, 1100, 60) whose row t has t values of group 1 below group 2 and the rest
  above, p from about 1 down to 0, against erfc(|z| / sqrt 2) from mpmath at 50 digits on the oracle's float64 z.

Bars (those of _check_ranksum in test_gpu_parity.py and DESIGN.md section 7), on every row of every output:
tested equal and never another byte than 0 or 1; z equal by value in float64; med1, med2, mean1, mean2, delta equal as
float32 values with NaN == NaN, the means also bit for bit (a zero's sign included; which zero np.median returns is
numpy's own accident); untested rows all-zero in every output; p within 1e-9 relative where the referee's p >= 1e-280
and below 2e-280 where it is smaller.

The tests without the gpu mark check the fixtures on the CPU: every palette and edge row is what its name says, the
palette index mixes the kinds over chunk positions, last chunks and stride passes, the ladder reaches every p band,
scipy's p agrees with mpmath."""
import functools
import os
import sys
import time
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle_np as O  # noqa: E402
from rank_support import (NOMINAL_CUS, P_FLOOR, P_RTOL, PLACEMENTS, _kept_positions, _values, chunk_table_rows, on_grid,  # noqa: E402
                          rows_per_wave)
from rank_support import bits as _bits, scatter as _scatter  # noqa: E402

gpu = pytest.mark.gpu

CHS = (64, 32, 8, 2)
FIELDS = ("med1", "med2", "mean1", "mean2", "delta")
OUT_DTYPES = dict(tested=np.uint8, p=np.float64, z=np.float64, med1=np.float32, med2=np.float32, mean1=np.float32,
                  mean2=np.float32, delta=np.float32)
# ranksum.variant -> the kernel that runs for groups of 17..63 columns (20 v 24)
KERNELS = {0: "pairq, then wave<1> re-do", 1: "lane", 4: "pair", 3: "wave on all rows", 5: "count, then wave re-do", 2: "block"}
ALL_VARIANTS = (0, 1, 4, 3, 5, 2)
POISON = np.array([np.nan, 1e30, -7.0, 0.12345], np.float32)       # what an unselected column holds


# ------------------------------------------------------------------------------ reference and comparison
def _on_grid(v):
    """is the value float32(key / 1000) of its clamped key, the kernels' own question (FLT_MAX * 1000 overflows: off)"""
    with np.errstate(over="ignore"):
        return on_grid(v)


def _reference(ps, g1, g2):
    """oracle_np.compare_rows with scipy: tested, p, z, med1, med2, mean1, mean2, delta (numpy's warnings about inf - inf
    and overflowing sums are its IEEE results, wanted here)"""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.compare_rows(ps, g1, g2)


def _check(got, ref, label, p_ref=None, where=None):
    """every bar on every row -> worst relative p error at or above the floor.  p_ref: the referee's p where it is not
    ref["p"] (mpmath's on the ladder); where(rows) describes failing rows in the failure message"""
    def say(what, bad):
        bad = np.asarray(bad)[:8]
        return f"{label}: {what}; first rows {bad.tolist()}" + ("" if where is None else f": {where(bad)}")

    bad = np.flatnonzero(got["tested"] > 1)
    assert bad.size == 0, say(("tested byte other than 0 or 1", hex(int(got["tested"][bad[0]])), bad.size), bad)
    bad = np.flatnonzero(got["tested"] != ref["tested"])
    assert bad.size == 0, say(("tested", bad.size), bad)
    t = ref["tested"].astype(bool)
    bad = np.flatnonzero(~(got["z"] == ref["z"]))
    assert bad.size == 0, say(("z", bad.size, got["z"][bad[:4]], ref["z"][bad[:4]]), bad)
    for name in FIELDS:
        g, w = got[name], ref[name]
        both_nan = np.isnan(g) & np.isnan(w)
        bad = np.flatnonzero(~((g == w) | both_nan))
        assert bad.size == 0, say((name, bad.size, g[bad[:4]], w[bad[:4]]), bad)
        if name.startswith("mean"):
            bad = np.flatnonzero(~((_bits(g) == _bits(w)) | both_nan))
            assert bad.size == 0, say((name + " bits", bad.size, g[bad[:4]], w[bad[:4]]), bad)
    for name in ("p", "z") + FIELDS:
        bad = np.flatnonzero(_bits(got[name][~t]))
        assert bad.size == 0, say(("untested row not zero in " + name, bad.size), np.flatnonzero(~t)[bad])
    pr = ref["p"] if p_ref is None else p_ref
    cell = t & (pr >= P_FLOOR)
    err = np.abs(got["p"][cell] - pr[cell]) / pr[cell]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= P_RTOL, say(("p", worst), np.flatnonzero(cell)[np.argsort(-err)])
    low = t & ~cell
    bad = np.flatnonzero(low & ~((got["p"] >= 0) & (got["p"] < 2 * P_FLOOR)))
    assert bad.size == 0, say(("p below the floor", got["p"][bad[:4]], pr[bad[:4]]), bad)
    return worst


def _run_dev(ctx, d_ps, d_g1, d_g2, variant, with_z=True, fill=None):
    """sdice_ranksum_dev on an uploaded table -> host copies of the outputs"""
    n = d_ps.shape[0]
    out = {name: ctx.empty(n, dtype) for name, dtype in OUT_DTYPES.items() if with_z or name != "z"}
    try:
        if fill is not None:
            for d in out.values():
                d.memset(fill)
        with ctx.params({"ranksum.variant": variant}):
            ctx.ranksum_dev(d_ps, d_g1, d_g2, out)
            return {name: d.to_host() for name, d in out.items()}
    finally:
        for d in out.values():
            d.free()


def _run_variants(ctx, ps, g1, g2, ref, variants, label, **kw):
    d_ps, d_g1, d_g2 = ctx.to_device(ps), ctx.to_device(g1), ctx.to_device(g2)
    try:
        for variant in variants:
            t0 = time.perf_counter()
            got = _run_dev(ctx, d_ps, d_g1, d_g2, variant)
            worst = _check(got, ref, f"{label} variant {variant}", **kw)
            print(f"{label} variant {variant}: {ps.shape[0]} rows, tested {int(ref['tested'].sum())}, worst p rel "
                  f"{worst:.3g}, {time.perf_counter() - t0:.2f} s")
    finally:
        for d in (d_ps, d_g1, d_g2):
            d.free()


def _split_columns(n1, n2, s, rng, ends=False):
    """-> (g1, g2, other): two groups interleaved in table order (a seeded split, each group sorted) and the unselected
    columns; ends: group 1 takes column 0 and group 2 column s - 1"""
    if ends:
        inner = 1 + rng.permutation(s - 2)
        g1 = np.r_[0, inner[: n1 - 1]]
        g2 = np.r_[s - 1, inner[n1 - 1: n1 + n2 - 2]]
        other = inner[n1 + n2 - 2:]
    else:
        perm = rng.permutation(s)
        g1, g2, other = perm[:n1], perm[n1: n1 + n2], perm[n1 + n2:]
    return np.sort(g1).astype(np.int32), np.sort(g2).astype(np.int32), np.sort(other)


# ------------------------------------------------------------------------------ A: the palette
KINDS = ("grid tested", "grid with NaNs", "grid starved", "off-grid tested", "off-grid with NaNs", "off-grid starved",
         "all equal on the grid", "all NaN")
PER_KIND = 40
OFF_GRID_VALUE = np.float32(0.1234567)
WIDE_GROUPS = ((70, 90), (260, 300), (513, 520))                    # count<E> / wave<E> for E = 2, 8, 16


@functools.lru_cache(maxsize=None)
def palette(n1=20, n2=24):
    """-> (rows float32[8 * 40, n1 + n2 + 4], g1, g2, kind[320], reference of the rows).  Four spare columns hold values
    that would show if they were read.  Variants of a kind: ties copied across the groups (v % 4 == 1), NaNs by the four
    placements of the count sweeps, the starved group alternating; an off-grid row is a 3-decimal row with one kept
    value 0.1234567 (v even) or a fully continuous row (v odd)."""
    rng = np.random.default_rng(n1 * 8191 + n2)
    s = n1 + n2 + 4
    g1, g2, spare = _split_columns(n1, n2, s, rng)
    sel = np.r_[g1, g2]
    rows = np.full((len(KINDS) * PER_KIND, s), np.nan, np.float32)
    for r in range(rows.shape[0]):
        kind, v = KINDS[r // PER_KIND], r % PER_KIND
        row = rows[r]
        row[spare] = rng.choice(POISON, size=spare.size)
        if kind == "all NaN":
            continue
        off = kind.startswith("off-grid")
        if kind == "all equal on the grid":
            row[sel] = _values(rng, 1, "q3")[0]
        else:
            row[sel] = _values(rng, n1 + n2, "cont" if off and v % 2 else "q3")
            if v % 4 == 1:
                row[g1[rng.integers(0, n1, 4)]] = row[g2[rng.integers(0, n2, 4)]]
        k1, k2 = n1, n2
        if kind.endswith("with NaNs") or (kind == "all equal on the grid" and v % 3 == 1):
            k1, k2 = int(rng.integers(3, n1)), int(rng.integers(3, n2 + 1))
        elif kind.endswith("starved"):
            k1, k2 = (2, int(rng.integers(3, n2 + 1))) if v % 2 else (int(rng.integers(3, n1 + 1)), 2)
        keep = np.r_[g1[_kept_positions(n1, k1, PLACEMENTS[v % 4], rng)],
                     g2[_kept_positions(n2, k2, PLACEMENTS[(v + 1) % 4], rng)]]
        row[np.setdiff1d(sel, keep)] = np.nan
        if off and v % 2 == 0:
            row[keep[rng.integers(0, keep.size)]] = OFF_GRID_VALUE
    kind = np.repeat(np.arange(len(KINDS)), PER_KIND)
    return rows, g1, g2, kind, _reference(rows, g1, g2)


def palette_index(n):
    """row r takes kind (r + r // 64) % 8: every 64-row chunk holds all kinds, and the kind at a chunk's positions 0 and
    63 moves on by one from chunk to chunk; the variant inside the kind is seeded"""
    r = np.arange(n, dtype=np.int64)
    kind = (r + r // 64) % len(KINDS)
    return kind * PER_KIND + np.random.default_rng(n).integers(0, PER_KIND, size=n)


@pytest.mark.parametrize("n1,n2", ((20, 24),) + WIDE_GROUPS)
def test_palette_kinds_are_what_they_claim(n1, n2):
    rows, g1, g2, kind, ref = palette(n1, n2)
    sel = np.r_[g1, g2]
    assert g1.size == n1 and g2.size == n2 and np.unique(sel).size == n1 + n2 and rows.shape[1] == n1 + n2 + 4
    spare = np.setdiff1d(np.arange(rows.shape[1]), sel)
    assert np.isin(_bits(np.ascontiguousarray(rows[:, spare])), _bits(POISON)).all()
    assert not np.all(_on_grid(POISON))
    for r in range(rows.shape[0]):
        name = KINDS[kind[r]]
        kept1, kept2 = int((~np.isnan(rows[r, g1])).sum()), int((~np.isnan(rows[r, g2])).sum())
        assert bool(np.all(_on_grid(rows[r, sel]))) == (not name.startswith("off-grid")), (r, name)
        assert ref["tested"][r] == (not name.endswith("starved") and name != "all NaN"), (r, name)
        assert ref["tested"][r] == (kept1 >= 3 and kept2 >= 3), (r, name)
        if name.endswith("starved"):
            assert min(kept1, kept2) == 2 and max(kept1, kept2) >= 3, (r, name)
        if name.endswith("with NaNs"):
            assert kept1 < n1 and min(kept1, kept2) >= 3, (r, name)
        if name.endswith("tested"):
            assert kept1 == n1 and kept2 == n2, (r, name)
        if name == "all equal on the grid":
            assert np.unique(rows[r, sel][~np.isnan(rows[r, sel])]).size == 1 and ref["z"][r] == 0.0 and ref["p"][r] == 1.0
        if name == "all NaN":
            assert kept1 == 0 and kept2 == 0
    assert len({row.tobytes() for row in rows}) >= 250
    t = ref["tested"].astype(bool)
    assert np.unique(ref["z"][t]).size > 100 and ref["p"][t].min() >= P_FLOOR
    for name in ("p", "z") + FIELDS:
        assert not ref[name][~t].any()
    # ties across the groups are there: some tested row has a value of group 1 in group 2
    whole = np.flatnonzero(~np.isnan(rows[:, sel]).any(axis=1))
    assert sum(np.intersect1d(rows[r, g1], rows[r, g2]).size > 0 for r in whole) > 20


@pytest.mark.parametrize("ch", CHS)
def test_palette_index_arrangement(ch):
    """for a nominal 256 compute units: the table selects ch and its last chunk is partial; every 64-row chunk mixes at
    least three kinds; every kind occurs at chunk positions 0 and 63, in the partial last chunk as far as it has rows for
    them, and (ch = 64) beyond the rows where the second grid-stride pass of every kernel class starts"""
    n = chunk_table_rows(ch, NOMINAL_CUS)
    assert rows_per_wave(n, NOMINAL_CUS) == ch
    idx = palette_index(n)
    kind = idx // PER_KIND
    every = set(range(len(KINDS)))
    assert idx.min() >= 0 and idx.max() < len(KINDS) * PER_KIND and np.unique(idx).size == len(KINDS) * PER_KIND
    full = kind[: n - n % 64].reshape(-1, 64)
    distinct = (np.diff(np.sort(full, axis=1), axis=1) != 0).sum(axis=1) + 1
    assert distinct.min() >= 3
    assert set(full[:, 0].tolist()) == set(full[:, 63].tolist()) == every
    for pos in (0, ch - 1):                                      # and at the ends of the chunks of ch rows
        assert set(kind[pos: n - n % ch: ch].tolist()) == every
    last = kind[n - n % ch:]
    assert 0 < last.size < ch and np.unique(last).size == min(last.size, len(KINDS))
    if n > 32 * NOMINAL_CUS * ch:                                # the wave and counting kernels stride over chunks
        assert set(kind[32 * NOMINAL_CUS * ch:].tolist()) == every
    if ch == 64:
        assert n * 48 * 4 < 210e6
        for first in (2048 * NOMINAL_CUS, 1536 * NOMINAL_CUS):   # pairq and lane; pair; block strides every 2048 rows
            assert first in (524288, 393216) and n > first and set(kind[first:].tolist()) == every


def _where_in_table(idx, kind, ch, cus):
    def where(rows):
        return [dict(row=int(r), kind=KINDS[kind[idx[r]]], palette_row=int(idx[r]), ch=ch, position_in_chunk=int(r % ch),
                     chunk_pass=int(r // ch // (32 * cus)), lane_pass=int(r // (2048 * cus)), pair_pass=int(r // (1536 * cus)))
                for r in rows]
    return where


@gpu
@pytest.mark.parametrize("ch", CHS)
def test_ranksum_rows_per_wave(ctx, ch):
    """ch rows per wave in ranksum_wave_kernel<1> (all rows, and as the re-do pass behind pairq<32> and count<1>) and in
    ranksum_count_kernel<1>, their stride over chunks, and for ch = 64 the second grid-stride pass of pairq<32>,
    lane<32>, pair<32> and the block kernel: every row of every output against the oracle on the palette, scattered
    through the index.  The ch = 64 table also goes through sdice_ranksum_dev with z absent into outputs pre-filled with
    0x5A: tested, p and the five float outputs equal the run with z bit for bit."""
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    rows, g1, g2, kind, ref = palette()
    idx = palette_index(n)
    ps = np.ascontiguousarray(rows[idx])
    want = _scatter(ref, idx)
    where = _where_in_table(idx, kind, ch, cus)
    d_ps, d_g1, d_g2 = ctx.to_device(ps), ctx.to_device(g1), ctx.to_device(g2)
    try:
        for variant in (ALL_VARIANTS if ch == 64 else (0, 3, 5)):
            t0 = time.perf_counter()
            got = _run_dev(ctx, d_ps, d_g1, d_g2, variant)
            _check(got, want, f"ch={ch} n={n} on {cus} CUs, variant {variant} ({KERNELS[variant]})", where=where)
            print(f"ch={ch} n={n} variant {variant} ({KERNELS[variant]}): {time.perf_counter() - t0:.2f} s")
            if ch == 64 and variant == 0:
                assert n > 2048 * cus and -(-n // ch) > 32 * cus
                bare = _run_dev(ctx, d_ps, d_g1, d_g2, 0, with_z=False, fill=0x5A)
                for name, dev in bare.items():
                    bad = np.flatnonzero(dev.view(np.uint8) != got[name].view(np.uint8))
                    assert bad.size == 0, ("sdice_ranksum_dev without z", name, bad.size, bad[:5].tolist())
    finally:
        for d in (d_ps, d_g1, d_g2):
            d.free()


@gpu
@pytest.mark.parametrize("n1,n2", WIDE_GROUPS)
def test_ranksum_rows_per_wave_wide_groups(ctx, n1, n2):
    """count<E> with its wave<E> re-do pass (auto) and wave<E> on all rows at two rows per wave, E = 2, 8, 16; from
    E = 8 the histogram of the counting kernel lies over the compacted values (H_ALIAS)"""
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(2, cus)
    rows, g1, g2, kind, ref = palette(n1, n2)
    idx = palette_index(n)
    ps = np.ascontiguousarray(rows[idx])
    assert ps.nbytes < 150e6 * cus / NOMINAL_CUS
    _run_variants(ctx, ps, g1, g2, _scatter(ref, idx), (0, 3), f"{n1} v {n2}, ch=2 n={n}",
                  where=_where_in_table(idx, kind, 2, cus))


# ------------------------------------------------------------------------------ B: edge values
F = np.float32
TINY = F(1e-45)                       # the smallest float32 subnormal
FLT_MIN = F(1.17549435e-38)
FLT_MAX = np.finfo(np.float32).max
INF = F(np.inf)


def _up(x):
    return np.nextafter(F(x), INF)


def _down(x):
    return np.nextafter(F(x), -INF)


def _pool(*values):
    values = np.array(values, np.float32)
    return lambda rng, k: values[rng.integers(0, values.size, size=k)]


def _grid(rng, k):
    return (rng.integers(50, 951, size=k) / 1000.0).astype(np.float32)


def _cont(rng, k):
    return _values(rng, k, "cont")


UNDER_ULPS = (0.3, 0.7, 0.001, 0.999, 0.5)
# name -> (values group 1 must hold, values group 2 must hold, what fills the rest of group 1, of group 2; None: NaN)
EDGE_ROWS = {
    "-0.0 among +0.0 across both groups (one tie group)":
        ([-0.0, 0.0, -0.0, 0.5, 0.25], [-0.0, -0.0, 0.0, 0.1, 0.2], _pool(-0.0, 0.0), _pool(0.0, -0.0)),
    "group 1 only -0.0":
        ([-0.0] * 3, [0.0, -0.0, 0.001, 0.5], _pool(-0.0), _grid),
    "both groups only -0.0":
        ([-0.0] * 3, [-0.0] * 3, _pool(-0.0), _pool(-0.0)),
    "subnormals next to 0.0 (distinct values)":
        ([0.0, -0.0, -TINY, -2 * TINY, TINY, -FLT_MIN], [0.0, TINY, 2 * TINY, 3 * TINY, F(1e-40), FLT_MIN, -TINY],
         _pool(0.0, -TINY, -2 * TINY, TINY), _pool(0.0, TINY, 2 * TINY, 3 * TINY, F(1e-40))),
    "one ulp above and below grid values, the grid values beside them":
        ([x for k in UNDER_ULPS for x in (F(k), _up(k))], [x for k in UNDER_ULPS for x in (F(k), _down(k))],
         _pool(*[f(k) for k in UNDER_ULPS for f in (F, _up, _down)]), _pool(*[f(k) for k in UNDER_ULPS for f in (F, _up, _down)])),
    "values that clamp to keys 0 and 1000":
        ([1.0004, -0.0004, 2.0, -1.0, 1.0, 0.0], [1.0004, -0.0004, 1.0, 0.0, 0.999, 0.001, 2.0],
         _pool(0.0, 1.0, 1.0004, -0.0004, 0.5), _pool(0.0, 1.0, 1.0004, -0.0004, 0.5, -1.0)),
    "large magnitudes, +-1e30":
        ([1e30, -1e30, 0.5, 1e30], [-1e30, 0.25, 1e30, 3e29], _cont, _cont),
    "FLT_MAX: the means overflow to +inf and -inf":
        ([FLT_MAX, FLT_MAX, 0.5, FLT_MAX], [-FLT_MAX, -FLT_MAX, -0.5, -FLT_MAX], _pool(FLT_MAX, 0.5, 1.0), _pool(-FLT_MAX, -1.0)),
    "FLT_MAX of both signs in one group (the order of the additions decides)":
        ([FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, 0.1], [0.2, 0.4, 0.6], _pool(FLT_MAX, -FLT_MAX, 0.3), _grid),
    "+inf alone in group 1":
        ([np.inf, 0.2, 0.4, 0.6], [0.1, 0.3, 0.5], _grid, _grid),
    "-inf alone in group 2":
        ([0.1, 0.3, 0.5], [-np.inf, 0.2, 0.4, 0.6], _grid, _grid),
    "+inf and -inf together in group 1":
        ([np.inf, -np.inf, 0.3, 0.5, 0.7], [0.1, 0.3, 0.5], _grid, _grid),
    "+inf in both groups (a tie at the top)":
        ([np.inf, 0.2, 0.4, 0.6], [np.inf, np.inf, 0.3, 0.5], _grid, _grid),
    "group 1 holds only infinities (its median is inf - inf)":
        ([-np.inf, np.inf, -np.inf, np.inf], [0.1, 0.3, 0.5], None, _grid),
    "group 1 keeps exactly 3":
        ([0.2, 0.8, 0.5], [0.1, 0.3, 0.5], None, _grid),
    "both groups keep exactly 3, ties":
        ([0.5, 0.5, 0.25], [0.25, 0.5, 0.75], None, None),
}
EDGE_ON_GRID = ("-0.0 among +0.0 across both groups (one tie group)", "group 1 only -0.0", "both groups only -0.0",
                "group 1 keeps exactly 3", "both groups keep exactly 3, ties")
EDGE_SHAPES = {"20 v 24": (20, 24, 48, ALL_VARIANTS), "70 v 90": (70, 90, 164, (0, 3, 5, 2)),
               "20 v 24 of 4099 columns": (20, 24, 4099, ALL_VARIANTS)}


@functools.lru_cache(maxsize=None)
def edge_table(shape):
    """-> (ps, g1, g2, names, reference).  Every named row with its values at seeded positions of the groups; a row on
    the grid is followed by `name / sorted`, the same row with its largest value moved up by an ulp, which takes it off
    the grid and to the sorting kernels.  Every unselected column is poison.  The 4099-column table selects columns 0
    and 4098."""
    n1, n2, s, _ = EDGE_SHAPES[shape]
    rng = np.random.default_rng(s * 31 + n1)
    g1, g2, other = _split_columns(n1, n2, s, rng, ends=s == 4099)
    names, table = [], []
    for name, (a, b, fill_a, fill_b) in EDGE_ROWS.items():
        row = np.empty(s, np.float32)
        row[other] = rng.choice(POISON, size=other.size)
        for g, core, fill in ((g1, a, fill_a), (g2, b, fill_b)):
            vals = np.full(g.size, np.nan, np.float32) if fill is None else fill(rng, g.size).astype(np.float32)
            vals[rng.permutation(g.size)[: len(core)]] = np.array(core, np.float32)
            row[g] = vals
        names.append(name)
        table.append(row)
        if name in EDGE_ON_GRID:
            moved = row.copy()
            sel = np.r_[g1, g2]
            at = sel[int(np.nanargmax(row[sel]))]
            moved[at] = _up(row[at])
            names.append(name + " / sorted")
            table.append(moved)
    ps = np.stack(table)
    return ps, g1, g2, tuple(names), _reference(ps, g1, g2)


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_rows_are_what_they_claim(shape):
    ps, g1, g2, names, ref = edge_table(shape)
    n1, n2, s, _ = EDGE_SHAPES[shape]
    sel = np.r_[g1, g2]
    assert ps.shape == (len(EDGE_ROWS) + len(EDGE_ON_GRID), s) and np.unique(sel).size == n1 + n2 == sel.size
    other = np.setdiff1d(np.arange(s), sel)
    assert np.isin(_bits(np.ascontiguousarray(ps[:, other])), _bits(POISON)).all()
    if s == 4099:
        assert g1[0] == 0 and g2[-1] == 4098 and other.size == 4099 - 44
    assert ref["tested"].all()
    row = {name: ps[r] for r, name in enumerate(names)}
    out = {name: {k: v[r] for k, v in ref.items()} for r, name in enumerate(names)}
    for name in names:
        assert bool(np.all(_on_grid(row[name][sel]))) == (name in EDGE_ON_GRID), name
        assert (name + " / sorted" in names) == (name in EDGE_ON_GRID), name
    r = row["-0.0 among +0.0 across both groups (one tie group)"]
    assert np.unique(r[sel]).size == 5 and (r[sel] == 0).sum() == n1 + n2 - 4
    assert 3 <= np.signbit(r[g1]).sum() < n1 - 2 and 3 <= np.signbit(r[g2]).sum() < n2 - 2
    r, o = row["group 1 only -0.0"], out["group 1 only -0.0"]
    assert np.signbit(r[g1]).all() and not r[g1].any() and _bits(o["mean1"][None])[0] == 0      # numpy: +0.0 of -0.0 values
    r, o = row["group 1 only -0.0 / sorted"], out["group 1 only -0.0 / sorted"]
    assert np.signbit(r[g1]).all() and not r[g1].any() and _bits(o["mean1"][None])[0] == 0
    o = out["both groups only -0.0"]
    assert o["z"] == 0.0 and o["p"] == 1.0 and _bits(o["mean1"][None])[0] == 0 and _bits(o["mean2"][None])[0] == 0
    r, o = row["subnormals next to 0.0 (distinct values)"], out["subnormals next to 0.0 (distinct values)"]
    assert np.unique(r[sel]).size == 9 and np.all(np.abs(r[sel]) <= FLT_MIN) and 0 < (r[sel] == 0).sum() < n1 + n2
    assert o["z"] < -1.0                       # flushed to zero the row would be one tie group, z = 0
    r = row["one ulp above and below grid values, the grid values beside them"]
    assert np.unique(r[sel]).size == 15 and np.unique(np.rint(r[sel] * F(1000))).size == 5
    r = row["values that clamp to keys 0 and 1000"]
    k = np.rint(r[sel] * F(1000))
    assert r[sel].max() == 2.0 and r[sel].min() == -1.0 and (k > 1000).any() and (k < 0).any()
    assert ((k == 1000) & (r[sel] > 1)).any() and ((k == 0) & (r[sel] < 0)).any()
    o = out["large magnitudes, +-1e30"]
    assert np.isfinite([o["mean1"], o["mean2"], o["med1"], o["med2"]]).all() and abs(o["mean1"]) > 1e27
    o = out["FLT_MAX: the means overflow to +inf and -inf"]
    assert o["mean1"] == np.inf and o["mean2"] == -np.inf
    o = out["+inf alone in group 1"]
    assert o["mean1"] == np.inf and np.isfinite(o["med1"]) and np.isfinite(o["z"]) and np.isfinite(o["mean2"])
    o = out["-inf alone in group 2"]
    assert o["mean2"] == -np.inf and np.isfinite(o["med2"]) and np.isfinite(o["mean1"])
    o = out["+inf and -inf together in group 1"]
    assert np.isnan(o["mean1"]) and np.isfinite(o["med1"]) and 0 < o["p"] <= 1
    o = out["+inf in both groups (a tie at the top)"]
    assert o["mean1"] == np.inf and o["mean2"] == np.inf
    o = out["group 1 holds only infinities (its median is inf - inf)"]
    assert np.isnan(o["med1"]) and np.isnan(o["delta"]) and np.isnan(o["mean1"]) and np.isfinite(o["med2"])
    r = row["group 1 keeps exactly 3"]
    assert (~np.isnan(r[g1])).sum() == 3 and (~np.isnan(r[g2])).sum() == n2
    r = row["both groups keep exactly 3, ties"]
    assert (~np.isnan(r[g1])).sum() == 3 and (~np.isnan(r[g2])).sum() == 3 and np.unique(r[sel][~np.isnan(r[sel])]).size == 3


@gpu
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_ranksum_edge_values(ctx, shape):
    """the named rows through every kernel class that takes the group sizes: pairq, lane, pair, wave, count and block
    for 20 v 24 (also out of a table of 4099 columns, the selection reaching its first and last column), count<2>,
    wave<2> and block for 70 v 90.  With the sums taken without np.sum's identity 0 (ranksum.hip before it added it) the
    rows `group 1 only -0.0` and `both groups only -0.0` fail on the bits of the means in every float kernel: -0.0 where
    numpy has +0.0"""
    ps, g1, g2, names, ref = edge_table(shape)
    _run_variants(ctx, ps, g1, g2, ref, EDGE_SHAPES[shape][3], f"edge values {shape}",
                  where=lambda rows: [names[r] for r in rows])


# ------------------------------------------------------------------------------ C: selection shapes of the dispatch
# (n1, n2) -> the first kernel of the auto dispatch: the 16-bit kernel for a larger group of 17..64 with n1 <= 63 (its
# sentinel slot), pairq<32> up to 32 and pairq<64> above; the float pair kernel below 17 and for n1 = 64
DISPATCH = {(16, 16): "pair", (16, 17): "pairq", (17, 16): "pairq", (17, 17): "pairq", (32, 32): "pairq", (32, 33): "pairq",
            (33, 32): "pairq", (63, 17): "pairq", (63, 40): "pairq", (63, 63): "pairq", (63, 64): "pairq",
            (64, 17): "pair", (64, 40): "pair", (64, 63): "pair", (64, 64): "pair"}
RANKSUM_KERNELS = ("ranksum_pairq_kernel", "ranksum_pair_kernel", "ranksum_lane_kernel", "ranksum_wave_kernel",
                   "ranksum_count_kernel", "ranksum_block_kernel", "ranksum_finish_kernel")


def test_dispatch_shapes_cover_the_boundaries():
    for (n1, n2), kernel in DISPATCH.items():
        big = max(n1, n2)
        assert kernel == ("pairq" if big > 16 and n1 <= 63 else "pair") and big <= 64
    sizes = set(DISPATCH)
    assert {(16, 16), (16, 17), (17, 16), (32, 32), (32, 33), (33, 32), (63, 64), (64, 64), (63, 17), (64, 17)} <= sizes
    assert {n2 for n1, n2 in sizes if n1 == 63} >= {17, 40, 64} and {n2 for n1, n2 in sizes if n1 == 64} >= {17, 40, 64}


@gpu
@pytest.mark.parametrize("n1,n2", sorted(DISPATCH))
def test_ranksum_dispatch_shapes(ctx, n1, n2):
    """the palette of the group sizes (rows on and off the grid, with NaNs, starved) through the auto dispatch; the
    profiler tells which kernels ran: the 16-bit kernel and the wave kernel behind it, or the float pair kernel alone"""
    rows, g1, g2, kind, ref = palette(n1, n2)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        got = ctx.ranksum(rows, g1, g2)
        ctx.sync()
        report = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    ran = {name for name in RANKSUM_KERNELS if report.get(name, (0, 0.0))[0]}
    want = {"pairq": {"ranksum_pairq_kernel", "ranksum_wave_kernel"}, "pair": {"ranksum_pair_kernel"}}[DISPATCH[n1, n2]]
    assert ran == want | {"ranksum_finish_kernel"}, (n1, n2, report)
    _check(got, ref, f"dispatch {n1} v {n2}", where=lambda r: [KINDS[kind[x]] for x in r])


# ------------------------------------------------------------------------------ D: the p ladder
P_BANDS = ((1e-3, 1.0), (1e-20, 1e-3), (1e-100, 1e-20), (1e-200, 1e-100), (1e-280, 1e-200))
LADDERS = {1024: (0, 3, 2), 1100: (0,), 60: (0, 1, 4, 3, 2)}           # group size -> variants (auto first)
LADDER_CLASS = {(1024, 0): "count, then wave<16> re-do", (1024, 3): "wave<16>", (1024, 2): "block", (1100, 0): "block (auto)",
                (60, 0): "pairq<64>", (60, 1): "lane<64>", (60, 4): "pair<64>", (60, 3): "wave<1>", (60, 2): "block"}


@functools.lru_cache(maxsize=None)
def ladder(G):
    """-> (ps float32[G + 1, 2 G + 3], g1, g2, reference, p from mpmath as floats, the same as mpmath numbers).  Row t: t
    of group 1's G values lie below all of group 2 and the others above; all 2 G values distinct, 3-decimal values when
    the grid has that many (G = 60), continuous otherwise.  U = (G - t) G, so z falls from its largest value at t = 0
    through 0 at t = G / 2 to its smallest at t = G."""
    import mpmath
    rng = np.random.default_rng(G)
    s = 2 * G + 3
    g1, g2, other = _split_columns(G, G, s, rng)
    ps = np.empty((G + 1, s), np.float32)
    ps[:, other] = rng.choice(POISON, size=(G + 1, other.size))
    for t in range(G + 1):
        if 2 * G <= 1001:
            v = (np.sort(rng.choice(1001, 2 * G, replace=False)) / 1000.0).astype(np.float32)
        else:
            v = np.sort(rng.choice(np.unique(rng.random(2 * G + 256).astype(np.float32)), 2 * G, replace=False))
        ps[t, g1] = rng.permutation(np.r_[v[:t], v[t + G:]])
        ps[t, g2] = rng.permutation(v[t: t + G])
    ref = _reference(ps, g1, g2)
    with mpmath.workdps(50):
        exact = [mpmath.erfc(abs(mpmath.mpf(float(z))) / mpmath.sqrt(2)) for z in ref["z"]]
    return ps, g1, g2, ref, np.array([float(p) for p in exact]), exact


def _assert_ladder_bands(exact, z):
    """every band, values below the floor, subnormal values and exact 0, on either side of z = 0 (p takes |z|)"""
    for side in (z > 0, z < 0):
        ps = [p for p, here in zip(exact, side) if here]
        for lo, hi in P_BANDS:
            assert any(lo <= p < hi for p in ps), (lo, hi)
        assert any(1e-300 < p < P_FLOOR for p in ps), "below the floor"
        assert any(0 < float(p) < 2.2250738585072014e-308 for p in ps), "subnormal"
        assert any(float(p) == 0.0 for p in ps), "exact 0"


@pytest.mark.parametrize("G", LADDERS)
def test_ladder_is_what_it_claims(G):
    """every row tested with all 2 G values distinct, z as U = (G - t) G gives it, p = 1 in the middle; the ladders of
    1024 and 1100 reach every band of p down to 1e-280, values below the floor, subnormal values and exact 0, with z of
    either sign"""
    ps, g1, g2, ref, p_ref, exact = ladder(G)
    assert ps.shape == (G + 1, 2 * G + 3) and ref["tested"].all()
    sel = np.r_[g1, g2]
    assert all(np.unique(row[sel]).size == 2 * G for row in ps)
    assert bool(np.all(_on_grid(ps[:, sel]))) == (G == 60) and (G == 60 or not np.all(_on_grid(ps[:, sel]), axis=1).any())
    t = np.arange(G + 1)
    below = (ps[:, g1] < ps[:, g2].min(axis=1, keepdims=True)).sum(axis=1)
    above = (ps[:, g1] > ps[:, g2].max(axis=1, keepdims=True)).sum(axis=1)
    assert np.array_equal(below, t) and np.array_equal(above, G - t)
    z = ((G - t) * G - G * G / 2.0) / np.sqrt(G * G * (2 * G + 1) / 12.0)
    assert np.array_equal(ref["z"], z) and np.all(np.diff(ref["z"]) < 0) and ref["z"][G // 2] == 0 and p_ref[G // 2] == 1.0
    if G >= 1024:
        _assert_ladder_bands(exact, ref["z"])
    else:
        assert 1e-22 < min(exact) < 1e-18


def test_scipy_ranksums_p_against_mpmath_on_the_ladder():
    """scipy's p, the referee of every other rank-sum test, within 1e-12 relative of mpmath's 50-digit erfc on every
    ladder row with p >= 1e-280"""
    worst, cells = 0.0, 0
    for G in LADDERS:
        _, _, _, ref, p_ref, exact = ladder(G)
        for t, p in enumerate(exact):
            if p >= P_FLOOR:
                worst = max(worst, float(abs(ref["p"][t] - p) / p))
                cells += 1
    print(f"scipy ranksums p against mpmath: {cells} cells, worst relative difference {worst:.3g}")
    assert cells > 1800 and worst <= 1e-12


@gpu
@pytest.mark.parametrize("G", LADDERS)
def test_ranksum_p_ladder(ctx, G):
    """p of every ladder row through the finish of every kernel class (rs_finish in the block kernel,
    ranksum_finish_kernel behind the others) against mpmath: within 1e-9 relative at or above 1e-280, below 2e-280
    where mpmath's p is smaller (subnormal or 0 included); prints the worst relative error per band"""
    ps, g1, g2, ref, p_ref, _ = ladder(G)
    d_ps, d_g1, d_g2 = ctx.to_device(ps), ctx.to_device(g1), ctx.to_device(g2)
    try:
        for variant in LADDERS[G]:
            got = _run_dev(ctx, d_ps, d_g1, d_g2, variant)
            per_band = []
            for lo, hi in P_BANDS:
                cell = (p_ref >= lo) & ((p_ref < hi) | (hi == 1.0))
                err = np.abs(got["p"][cell] - p_ref[cell]) / p_ref[cell]
                per_band.append(f"[{lo:g}, {hi:g}{']' if hi == 1.0 else ')'}: {int(cell.sum())} rows, {err.max() if err.size else 0.0:.3g}")
            low = p_ref < P_FLOOR
            print(f"ladder {G} v {G} variant {variant} ({LADDER_CLASS[G, variant]}): worst relative p error per band "
                  + "; ".join(per_band) + f"; below 1e-280: {int(low.sum())} rows, largest p returned "
                  f"{got['p'][low].max() if low.any() else 0.0:.3g}, exact zeros returned {int((got['p'][low] == 0).sum())}")
            _check(got, ref, f"ladder {G} v {G} variant {variant}", p_ref=p_ref, where=lambda r: [f"t = {int(x)}" for x in r])
    finally:
        for d in (d_ps, d_g1, d_g2):
            d.free()
