"""sdice_ranksum_strata (van Elteren's stratified rank-sum test) and compare_sample_sets --strata against the referee
(tests/strata_referee.py: Fractions, one mpmath square root, mpmath erfc), numpy and the unstratified call.

Bars: tested mask, medians, means and delta bit-exact against numpy, and bit-exact against ctx.ranksum on the same lists
on the rows both calls test (with one licence: sdice_ranksum reports np.median by value and returns -0.0 for the median of
an even count of -0.0 values where numpy, and this call, return +0.0 -- the two bars cannot both hold there, so a zero
median or zero delta of the plain call that differs from numpy's in sign alone is let through); |z - z_ref| <= 1e-12 max(1, |z_ref|); p within 1e-9 relative wherever the referee's p >=
1e-280 and under 2e-280 below that, such cells at most 1 % of a table's tested rows (asserted); every slot 0 where a row is
not tested.  The z bar: at most 64 once-rounded float64 terms added with at most 63 roundings are within 64 * 2^-53 * cond
of exact, cond = sum |d_h| / sqrt(sum V_h); the tests assert cond <= 100 on their own inputs, so the bound is 7e-13.

The tables mix every row kind of KINDS, each on 3-decimal values and on off-grid float32 values, at every total column
count that changes the kernel or its lane-group width; builders and references are cached and shared with
tests/test_gpu_strata_sweeps.py.  Tests without the gpu mark check on the CPU that the tables are what they claim."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_support as RS  # noqa: E402
import strata_referee as VR  # noqa: E402
from rank_support import P_FLOOR, P_RTOL, same_f32  # noqa: E402

gpu = pytest.mark.gpu

Z_TOL = 1e-12
COND_MAX = 100.0
GROUP_LIMIT = 4096                  # columns of one group, and
STRATA_LIMIT = 64                   # strata a call accepts (include/sdice.h)
# every total in 6..66: both kernels, every lane-group width (8, 16, 32, 64 lanes), the switch at 64 | 65; and the
# workgroup kernel's first LDS sizes
TOTALS = tuple(range(6, 67)) + (127, 128, 129)
HS = (1, 2, 3, 5)
KINDS = ("no NaN", "6 % NaN", "a stratum emptied on one side", "every stratum emptied on one side", "3 v 3 informative",
         "2 v 3 informative", "informative strata fully tied", "all values equal", "signed zeros", "subnormals and FLT_MAX")
F32 = ("med1", "med2", "mean1", "mean2", "delta")
OUTS = ("tested", "p", "z") + F32


def draw_lists(rng, n1, n2, H, spare=3):
    """two disjoint column lists of a shuffled table of n1 + n2 + spare columns and a stratum id per listed column;
    three columns of each list lie in stratum 0 and every id below H is used when the lists are long enough"""
    s = n1 + n2 + spare
    perm = rng.permutation(s).astype(np.int32)
    g1, g2 = perm[:n1].copy(), perm[n1: n1 + n2].copy()
    s1, s2 = rng.integers(0, H, size=n1).astype(np.int32), rng.integers(0, H, size=n2).astype(np.int32)
    s1[rng.permutation(n1)[:3]] = 0
    s2[rng.permutation(n2)[:3]] = 0
    free = np.flatnonzero(s1 != 0) if n1 >= n2 else np.flatnonzero(s2 != 0)
    longer = s1 if n1 >= n2 else s2
    for h, at in zip(range(1, H), free):           # (ids 1 .. H - 1 at least once, where there is room)
        longer[at] = h
    return g1, g2, s1, s2, s


def _base(rng, n1, n2, s1, s2, H, grid):
    """the two sides of a row before its kind is applied: uniform values with a batch shift of up to 0.2 per stratum, side
    1 shifted by what moves z by a draw from -5..5, so p stays far above the floor at any size"""
    shift = rng.uniform(-5.0, 5.0) * 0.29 * np.sqrt((n1 + n2) / (n1 * n2))
    batch = 0.2 * rng.random(H)
    x, y = 0.6 * rng.random(n1) + batch[s1] + shift, 0.6 * rng.random(n2) + batch[s2]
    if grid:
        return [(np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32) for v in (x, y)]     # float32(k / 1000.0)
    x, y = ((v * 1.7 - 0.3).astype(np.float32) + rng.random(v.size, dtype=np.float32) * np.float32(1e-3) for v in (x, y))
    dup = rng.integers(0, min(n1, n2), size=(max(1, min(n1, n2) // 4), 2))       # exact duplicates across the sides ...
    x[dup[:, 0]] = y[dup[:, 1]]
    dup = rng.integers(0, n2, size=(max(1, n2 // 6), 2))                         # ... and inside one
    y[dup[:, 0]] = y[dup[:, 1]]
    return [x, y]


def make_row(rng, kind, v, g1, g2, s1, s2, H, s):
    """one row of KINDS[kind], variant v (even: 3-decimal values, odd: off-grid float32)"""
    name = KINDS[kind]
    n1, n2 = g1.size, g2.size
    x, y = _base(rng, n1, n2, s1, s2, H, v % 2 == 0)
    nan = np.float32(np.nan)
    in0 = [np.flatnonzero(s1 == 0), np.flatnonzero(s2 == 0)]
    if name == "6 % NaN":
        x[rng.random(n1) < 0.06] = nan
        y[rng.random(n2) < 0.06] = nan
    elif name == "a stratum emptied on one side":
        h = int(rng.integers(0, H))
        if rng.integers(0, 2):
            x[s1 == h] = nan
        else:
            y[s2 == h] = nan
    elif name == "every stratum emptied on one side":
        for h in range(H):
            if rng.integers(0, 2):
                x[s1 == h] = nan
            else:
                y[s2 == h] = nan
    elif name in ("3 v 3 informative", "2 v 3 informative"):
        # stratum 0 keeps 3 (or 2) v 3, every other stratum keeps one side only: plenty of values, few that count
        x[in0[0][(3 if name[0] == "3" else 2):]] = nan
        y[in0[1][3:]] = nan
        for h in range(1, H):
            if rng.integers(0, 2):
                x[s1 == h] = nan
            else:
                y[s2 == h] = nan
    elif name == "informative strata fully tied":
        level = (rng.permutation(1001)[:H] / 1000.0).astype(np.float32) if v % 2 == 0 else rng.random(H, dtype=np.float32) * np.float32(3)
        x, y = level[s1].copy(), level[s2].copy()
        if n1 >= 8:
            x[rng.random(n1) < 0.05] = nan
    elif name == "all values equal":
        x[:], y[:] = (np.float32(0.5), np.float32(0.5)) if v % 2 == 0 else (np.float32(0.1234567), np.float32(0.1234567))
    elif name == "signed zeros":
        zeros = np.array([-0.0, 0.0], np.float32)
        sx, sy = rng.random(n1) < 0.4, rng.random(n2) < 0.4
        x[sx], y[sy] = rng.choice(zeros, size=int(sx.sum())), rng.choice(zeros, size=int(sy.sum()))
    elif name == "subnormals and FLT_MAX":
        # multiples of 2^-149 of either sign, and the largest float of one sign (two of them overflow a float32 sum)
        x, y = (rng.integers(1, 41, size=k).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], np.float32), size=k)
                for k in (n1, n2))
        top = np.float32(np.finfo(np.float32).max)
        x[rng.permutation(n1)[: 1 + v % 2]] = top
        y[rng.permutation(n2)[:1]] = top
    row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)       # would show if a spare column were read
    row[g1], row[g2] = x, y
    return row


@functools.lru_cache(maxsize=None)
def table(n1, n2, H, per_kind=2, kinds=None):
    """-> (ps float32[rows, n1 + n2 + 3], g1, g2, strat1, strat2, kind[rows]); the kinds interleaved, so that the rows side
    by side in a wave are of different kinds"""
    rng = np.random.default_rng(7000 + 131 * n1 + 17 * n2 + H)
    g1, g2, s1, s2, s = draw_lists(rng, n1, n2, H)
    rows, names = [], []
    for v in range(per_kind):
        for k in (range(len(KINDS)) if kinds is None else kinds):
            rows.append(make_row(rng, k, v, g1, g2, s1, s2, H, s))
            names.append(k)
    ps = np.ascontiguousarray(np.stack(rows))
    ps.setflags(write=False)
    return ps, g1, g2, s1, s2, np.array(names)


@functools.lru_cache(maxsize=None)
def reference(n1, n2, H, per_kind=2, kinds=None):
    ps, g1, g2, s1, s2, _ = table(n1, n2, H, per_kind, kinds)
    return VR.table_reference(ps, g1, g2, s1, s2)


def split(total):
    return total // 2, total - total // 2


def check(got, ref, label, floor_share=True, plain=None, quiet=False):
    """asserts every bar -> dict(tested, below, z_err, p_err, cond); plain: ctx.ranksum's result on the same lists"""
    t = RS.check_common(got, ref, F32, OUTS, label)
    if plain is not None:
        for name in F32:
            both = t & plain["tested"].astype(bool)
            unlike = both & ~same_f32(got[name], plain[name])
            # the one licence: where the plain call itself departs from numpy, in the sign of a zero median (or of the
            # delta of two zero medians), this call keeps numpy's zero
            excused = ~same_f32(plain[name], ref[name]) & (plain[name] == 0) & (ref[name] == 0) & (name in ("med1", "med2", "delta"))
            assert not (unlike & ~excused).any(), (label, name, "unlike the unstratified call", np.flatnonzero(unlike & ~excused)[:5])
        assert np.all(plain["tested"][t] == 1), label           # (what this call tests the plain call tests)
    cond = float(ref["cond"][t].max()) if t.any() else 0.0
    assert cond <= COND_MAX, (label, cond)
    z, zr = got["z"][t], ref["z"][t]
    err_z = np.abs(z - zr) / np.maximum(1.0, np.abs(zr))
    out = dict(tested=int(t.sum()), z_err=float(err_z.max()) if err_z.size else 0.0, cond=cond)
    if not quiet:
        print(f"{label}: rows {t.size} tested {out['tested']} worst z err {out['z_err']:.3g} largest cond {cond:.3g}", end=" ")
    assert np.all(err_z <= Z_TOL), (label, out["z_err"])
    assert np.all(z[ref["cond"][t] == 0] == 0), label           # no informative deviation at all: z is 0, not small
    out["below"], out["p_err"] = RS.check_p(got["p"][t], ref["p"][t], label, quiet)
    if floor_share:
        RS.check_floor_share(out["tested"], out["below"], label)
    return out


# ---------------------------------------------------------------- the tables, on the CPU
@pytest.mark.parametrize("total,H", [(6, 1), (9, 2), (33, 3), (64, 5), (65, 5), (129, 3)])
def test_tables_are_what_they_claim(total, H):
    n1, n2 = split(total)
    ps, g1, g2, s1, s2, kind = table(n1, n2, H)
    ref = reference(n1, n2, H)
    assert np.unique(np.concatenate([g1, g2])).size == total and ps.shape == (2 * len(KINDS), total + 3)
    assert (s1 == 0).sum() >= 3 and (s2 == 0).sum() >= 3 and max(s1.max(), s2.max()) < H
    if max(n1, n2) >= H + 3:
        assert np.union1d(s1, s2).size == H
    for r in range(ps.shape[0]):
        name = KINDS[kind[r]]
        x, y = ps[r, g1], ps[r, g2]
        both = np.concatenate([x, y])
        info = [h for h in range(H) if (~np.isnan(x[s1 == h])).any() and (~np.isnan(y[s2 == h])).any()]
        k1 = sum(int((~np.isnan(x[s1 == h])).sum()) for h in info)
        k2 = sum(int((~np.isnan(y[s2 == h])).sum()) for h in info)
        assert ref["tested"][r] == (k1 >= 3 and k2 >= 3), (r, name)
        if name in ("no NaN", "6 % NaN", "a stratum emptied on one side"):
            assert ref["grid"][r] == (r < len(KINDS)), (r, name)
        if name in ("no NaN", "all values equal", "signed zeros"):
            assert ref["tested"][r] and not np.isnan(both).any()
        if name == "every stratum emptied on one side":
            assert not info and not ref["tested"][r]
        if name == "3 v 3 informative":
            assert (k1, k2) == (3, 3) and info == [0] and ref["tested"][r]
        if name == "2 v 3 informative":
            assert (k1, k2) == (2, 3) and not ref["tested"][r]
            if H > 1 and total >= 33:
                assert (~np.isnan(both)).sum() > 8
        if name in ("informative strata fully tied", "all values equal") and ref["tested"][r]:
            assert ref["z"][r] == 0.0 and ref["p"][r] == 1.0 and ref["cond"][r] == 0.0
        if name == "signed zeros" and total >= 12:
            assert (np.signbit(both) & (both == 0)).any() and (~np.signbit(both) & (both == 0)).any()
        if name == "subnormals and FLT_MAX":
            v = np.abs(both)
            assert (v == np.finfo(np.float32).max).sum() >= 2 and (v < np.finfo(np.float32).tiny).sum() >= total - 3
    t = ref["tested"].astype(bool)
    assert t.sum() >= 10 and ref["cond"][t].max() <= COND_MAX and (ref["p"][t] >= P_FLOOR).all()


# ---------------------------------------------------------------- the library
@gpu
@pytest.mark.parametrize("H", HS)
def test_strata_parity(ctx, H):
    """every row kind, mixed in one table, at every total: both kernels, every lane-group width, 64 | 65"""
    worst = dict(z_err=0.0, p_err=0.0, cond=0.0, tested=0, below=0)
    for total in TOTALS:
        n1, n2 = split(total)
        ps, g1, g2, s1, s2, _ = table(n1, n2, H)
        got = ctx.ranksum_strata(ps, g1, g2, s1, s2)
        out = check(got, reference(n1, n2, H), f"total={total} H={H}", plain=ctx.ranksum(ps, g1, g2), quiet=True)
        for k in ("z_err", "p_err", "cond"):
            worst[k] = max(worst[k], out[k])
        worst["tested"] += out["tested"]
        worst["below"] += out["below"]
    print(f"H={H}: {len(TOTALS)} tables, {worst}")


@gpu
@pytest.mark.parametrize("n1,n2", [(1024, 1024), (4096, 4096), (4096, 3), (3, 4096)])
@pytest.mark.parametrize("H", [1, 8, 64])
def test_large_groups(ctx, n1, n2, H):
    """the workgroup kernel's largest sizes and most lopsided lists, a handful of rows each"""
    kinds = (0, 1, 2, 8)
    ps, g1, g2, s1, s2, _ = table(n1, n2, H, 2, kinds)
    check(ctx.ranksum_strata(ps, g1, g2, s1, s2), reference(n1, n2, H, 2, kinds), f"{n1} v {n2} H={H}",
          plain=ctx.ranksum(ps, g1, g2))


@gpu
@pytest.mark.parametrize("H", [63, 64])
def test_one_column_per_cell(ctx, H):
    """H strata of one column a side: every stratum is a pair, N_h = 2"""
    rng = np.random.default_rng(H)
    perm = rng.permutation(2 * H + 2).astype(np.int32)
    g1, g2 = perm[:H].copy(), perm[H: 2 * H].copy()
    s1, s2 = rng.permutation(H).astype(np.int32), rng.permutation(H).astype(np.int32)
    v = rng.integers(0, 1001, size=(24, 2 * H + 2)) / 1000.0
    v[:, g1] += 0.1 * rng.random((24, 1))
    ps = (np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32)       # rows 0..11 on the grid,
    ps[12:] += rng.random((12, 2 * H + 2), dtype=np.float32) * np.float32(1e-4)      # rows 12..23 off it
    ps[3::4][rng.random((6, 2 * H + 2)) < 0.1] = np.nan
    ps[5, g2[s2 < H - 3]] = np.nan                   # three pairs left
    ps[6, g2[s2 < H - 2]] = np.nan                   # two: not tested
    ref = VR.table_reference(ps, g1, g2, s1, s2)
    assert ref["tested"][5] == 1 and ref["tested"][6] == 0 and ref["tested"].sum() == 23
    check(ctx.ranksum_strata(ps, g1, g2, s1, s2), ref, f"one column per cell, H={H}", plain=ctx.ranksum(ps, g1, g2))


@gpu
@pytest.mark.parametrize("total,H", [(7, 2), (16, 3), (40, 5), (64, 5), (65, 5), (300, 17), (2000, 64)])
def test_numbering_and_group_order_do_not_matter(ctx, total, H):
    """permuting the stratum ids: bit-identical z and p; swapping g1 / g2 with strat1 / strat2: -z and the same p"""
    n1, n2 = split(total)
    kinds = None if total <= 65 else (0, 1, 2, 8)
    ps, g1, g2, s1, s2, _ = table(n1, n2, H, 2, kinds)
    got = ctx.ranksum_strata(ps, g1, g2, s1, s2)
    rng = np.random.default_rng(total)
    ids = np.arange(H, dtype=np.int32)
    drawn = rng.permutation(H).astype(np.int32)
    for perm in (ids[::-1], np.roll(ids, 1), drawn if (drawn != ids).any() else np.roll(ids, -1)):
        assert (perm != ids).any() and np.array_equal(np.sort(perm), ids)
        again = ctx.ranksum_strata(ps, g1, g2, perm[s1], perm[s2])
        for name in OUTS:
            assert np.array_equal(np.asarray(again[name]).view(np.uint8), np.asarray(got[name]).view(np.uint8)), (name, perm)
    swapped = ctx.ranksum_strata(ps, g2, g1, s2, s1)
    assert np.array_equal(swapped["tested"], got["tested"]) and got["tested"].sum() >= 4
    assert np.array_equal(swapped["z"], -got["z"]) and np.array_equal(swapped["p"], got["p"])
    assert np.all(same_f32(swapped["med1"], got["med2"])) and np.all(same_f32(swapped["mean2"], got["mean1"]))


@gpu
def test_tiny_calls(ctx):
    """lists too short for any row to be tested give zeros; n = 0 is a no-op"""
    ps = np.tile(np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], np.float32), (5, 1))
    for g1, g2 in (([0, 1], [2, 3, 4]), ([0], [1]), ([0, 1, 2, 3], [4, 5])):
        got = ctx.ranksum_strata(ps, g1, g2, [0] * len(g1), [0] * len(g2))
        assert not any(got[name].any() for name in OUTS)
    got = ctx.ranksum_strata(ps, [0, 1, 2], [3, 4, 5], [0, 0, 0], [0, 0, 0])
    assert got["tested"].tolist() == [1] * 5 and np.all(got["z"] < 0)
    empty = ctx.ranksum_strata(np.zeros((0, 7), np.float32), [0, 1, 2], [3, 4, 5], [0, 0, 0], [0, 0, 0])
    assert all(empty[name].shape == (0,) for name in OUTS)


ERROR_CASES = ("n_strata 0", "n_strata 65", "id -1", "id n_strata", "n1 0", "n1 4097", "column in both lists", "index equal to s")


def _error_call(ctx, case, dev):
    """-> (return code, outputs after, outputs before)"""
    n, s = 3, 12
    g1, g2 = np.array([0, 1, 2, 3], np.int32), np.array([4, 5, 6, 7], np.int32)
    s1, s2 = np.array([0, 1, 0, 1], np.int32), np.array([0, 1, 1, 0], np.int32)
    n1, H = 4, 2
    if case == "n_strata 0":
        H = 0
    elif case == "n_strata 65":
        H = STRATA_LIMIT + 1
    elif case == "id -1":
        s2[1] = -1
    elif case == "id n_strata":
        s1[2] = H
    elif case == "n1 0":
        n1 = 0
    elif case == "n1 4097":
        n1, s = GROUP_LIMIT + 1, GROUP_LIMIT + 1 + 8
        g1, s1 = np.arange(8, 8 + n1, dtype=np.int32), np.zeros(n1, np.int32)
    elif case == "column in both lists":
        g2[2] = g1[0]
    elif case == "index equal to s":
        g2[3] = s
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, dt) for i, (name, dt) in enumerate(VR.FIELDS)}
    before = {x: v.copy() for x, v in outs.items()}
    if not dev:
        return RS.raw_call(ctx, "sdice_ranksum_strata", ps, (g1, n1, g2, g2.size, s1, s2, H), outs, OUTS), outs, before
    held = [ctx.to_device(v, v.dtype) for v in (ps, g1, g2, s1, s2)] + [ctx.to_device(outs[x], outs[x].dtype) for x in OUTS]
    try:
        rc = ctx.lib.sdice_ranksum_strata_dev(ctx.h, n, s, held[0].ptr, held[1].ptr, n1, held[2].ptr, g2.size, held[3].ptr,
                                              held[4].ptr, H, *[a.ptr for a in held[5:]])
        ctx.sync()
        return rc, {x: a.to_host() for x, a in zip(OUTS, held[5:])}, before
    finally:
        for a in held:
            a.free()


@gpu
@pytest.mark.parametrize("case", ERROR_CASES)
def test_errors_leave_the_outputs_untouched(ctx, case):
    """SDICE_ERR_ARG before any launch, a message, outputs untouched, through the host call; through the _dev call the
    cases it can see (the counts: the lists are device memory there)"""
    rc, outs, before = _error_call(ctx, case, dev=False)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    message = ctx.lib.sdice_last_error()
    assert message and b"sdice_ranksum_strata" in message
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "n1 4097":
        assert b"4096" in message and b"4097" in message
    if case in ("n_strata 0", "n_strata 65", "n1 0", "n1 4097"):
        rc, outs, before = _error_call(ctx, case, dev=True)
        assert rc == -1 and ctx.lib.sdice_last_error(), case
        for x in outs:
            assert np.array_equal(outs[x], before[x]), (case, x, "dev")
    # the context still works
    ok = ctx.ranksum_strata(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5],
                            [0, 0, 1], [0, 1, 0])
    assert ok["tested"].tolist() == [1, 1]


@gpu
def test_engine_refuses_ids_of_another_length(ctx):
    with pytest.raises(ValueError, match="one stratum id per listed column"):
        ctx.ranksum_strata(np.zeros((2, 9), np.float32), [0, 1, 2], [3, 4, 5], [0, 0], [0, 0, 0])


# ---------------------------------------------------------------- command line
BATCHES = ("centre A", "B", "prep-3")


def _write_cli_inputs(tmp_path):
    """60 rows x (9 v 9) samples in 3 labelled batches + 2 samples outside the manifests (one without a label); the
    manifests' order is not the table's, batch "B" has samples of set 1 only on some rows' kept values"""
    rng = np.random.default_rng(707)
    n, s = 60, 20
    samples, _ = RS.ps_names(n, s)
    batch = np.array([j % 3 for j in range(18)] + [0, 1])
    set1 = np.array([0, 2, 4, 6, 8, 10, 12, 14, 16])
    set2 = np.array([1, 3, 5, 7, 9, 11, 13, 15, 17])
    v = rng.random((n, s)) * 0.6 + 0.15 * batch[None, :]
    v[:, set1] += 0.12 * rng.standard_normal((n, 1))
    v = np.clip(v, 0, 1)
    v[:10] = np.round(v[:10] * 5) / 5                                                    # heavy ties
    text = np.where(rng.random((n, s)) < 0.08, "nan", np.char.mod("%.3f", v))
    text[10:13] = "0.500"                                                                 # all-equal rows stay in the table
    text[13:16, set2[1:]] = "nan"                                                         # one value left in set 2: rows dropped
    text[16:18][:, set2[batch[set2] != 1]] = "nan"                                        # set 2 kept in batch B only
    path, (m1, m2), names = RS.write_ps_inputs(tmp_path, text, [([samples[j] for j in set1[::-1]], "A"),
                                                             ([samples[j] for j in rng.permutation(set2)], "B")])
    lab = tmp_path / "batches.tsv"
    lab.write_text("".join(f"{samples[j]}\t{BATCHES[batch[j]]}\n" for j in rng.permutation(19)))       # samp19: no label
    matrix = text.astype(np.float64).astype(np.float32)
    return path, m1, m2, str(lab), names, matrix, set1.astype(np.int32), set2.astype(np.int32), batch


def _cells(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [ln.split("\t") for ln in text[:-1].split("\n")]


@gpu
@pytest.mark.parametrize("gtf", [False, True])
def test_cli_strata(ctx, golden_dir, tmp_path, gtf):
    """compare_sample_sets --strata on 60 rows, 3 labelled batches: header, the tested rows in table order with their
    event names, float32 cells bit-equal after parsing, p within the bar of the referee, corrected = ctx.bh of the printed
    p column, the GTF columns those of the host annotation code"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, lab, names, matrix, g1, g2, batch = _write_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(argparse.Namespace(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=False,
                                    exact=False, strata=lab, annotation=anno, outputFile=out), ctx=ctx)
    # table order; ids by first appearance over g1 then g2 -- any numbering gives the same z and p
    ref = VR.table_reference(matrix, g1, g2, batch[g1], batch[g2])
    keep = np.flatnonzero(ref["tested"])
    assert 50 <= keep.size < 60 and {10, 11, 12} <= set(keep.tolist()) and not {13, 14, 15} & set(keep.tolist())
    assert ref["cond"].max() <= COND_MAX
    got = _cells(out)
    header = "event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected".split("\t")
    assert got[0] == header + (["gene", "overlapping", "transcript_id"] if gtf else []) and len(got) == keep.size + 1
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    printed_p = np.array([float(g[6]) for g in got[1:]])
    q = ctx.bh(printed_p)
    for i, (g, r) in enumerate(zip(got[1:], keep)):
        assert g[0] == names[r] and len(g) == (11 if gtf else 8)
        for cell, name in zip(g[1:6], ("mean1", "mean2", "med1", "med2", "delta")):
            assert same_f32(np.float32(float(cell)), ref[name][r]), (g, name, ref[name][r])
        assert str(np.float64(float(g[6]))) == g[6] and str(np.float64(float(g[7]))) == g[7]
        assert abs(float(g[6]) - ref["p"][r]) <= P_RTOL * ref["p"][r] and ref["p"][r] >= P_FLOOR, (g, ref["p"][r])
        assert float(g[7]) == q[i], (g, q[i])
        assert "\t".join([""] + g[8:]) == sfx[i] or not gtf
    # rows 16, 17: set 2 is kept in batch B alone, so only batch B is informative
    assert {16, 17} <= set(np.flatnonzero(np.isnan(matrix[:, g2[batch[g2] != 1]]).all(axis=1)).tolist())


@gpu
def test_cli_without_the_flag_is_unchanged(ctx, golden_dir, tmp_path):
    """the golden two-set run, with the flag absent and with strata=None: every byte of
    tests/golden/compare/expected_out_device.tsv, what the command wrote for these inputs on an MI355X before it had any
    of its added flags.  expected_out.tsv beside it cannot serve for a comparison of bytes -- it holds scipy's p-values
    and statsmodels' BH, an ulp or two from the device's in 242 of its 297 lines, before this flag as after (DESIGN.md
    section 7) -- so its cells are held by the rule of tests/test_gpu_cli.py: text and float32 cells as strings, p-value
    and corrected to 1e-6 relative."""
    from splicedice_amd import compare_sample_sets as css
    d = os.path.join(golden_dir, "compare")
    outs = []
    for extra in ({}, dict(paired=False, exact=False, moreManifests=None, strata=None)):
        outs.append(str(tmp_path / f"cmp{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "in_allPS.tsv"), manifest1=os.path.join(d, "m1.tsv"),
                                        manifest2=os.path.join(d, "m2.tsv"), annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    recorded = open(os.path.join(d, "expected_out_device.tsv"), "rb").read()
    assert open(outs[0], "rb").read() == recorded and open(outs[1], "rb").read() == recorded
    got, want = _cells(outs[1]), _cells(os.path.join(d, "expected_out.tsv"))
    assert len(got) == len(want) and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert g[:6] == w[:6]
        np.testing.assert_allclose([float(x) for x in g[6:]], [float(x) for x in w[6:]], rtol=1e-6)
