"""GPU: sdice_jonckheere (Jonckheere-Terpstra trend test across k ordered sample sets) and compare_sample_sets -mx --trend
against the exact referee (tests/jonckheere_referee.py: J2, M2 and the variance numerator as integers, z and p from mpmath
at 50 digits), numpy and sdice_kruskal.

Bars: tested, medians, means and delta equal as bits to numpy's and to ctx.kruskal's on the same
call; j equal as float64; |z - z_ref| <= 1e-12 max(1, |z_ref|) and exactly 0 where the referee's variance numerator is 0;
p within 1e-9 relative wherever the referee's p >= 1e-280 and below 2e-280 under that; untested rows all-zero.  On the
random parity tables the cells under the p floor are at most 1 % of the tested rows (asserted)."""
import argparse
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jonckheere_referee as JR  # noqa: E402
import kset_fixtures as KF  # noqa: E402
import rank_support as RS  # noqa: E402
from kset_fixtures import CHS, PALETTE_S, _edge_rows, _zero_sum_rows, draw_sets, palette, palette_index  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import N_LIMIT, P_FLOOR, P_RTOL, chunk_table_rows  # noqa: E402
from rank_support import bits as _bits, on_grid as _on_grid, scatter as _scatter, twin as _twin  # noqa: E402

pytestmark = pytest.mark.gpu

Z_TOL = 1e-12
KS = (2, 3, 4, 5, 8, 16, 33, 64)
SIZE_RANGES = ((3, 6), (3, 40), (3, 300))
SHAPES = ("uniform", "shifted", "ties", "cluster", "trend")
FLOAT_FIELDS = ("med", "mean", "delta")
OUTS = ("tested", "p", "z", "j", "med", "mean", "delta")


def _table(rng, sets, s, hi, rows_per_shape, grid):
    return KF.table(rng, sets, s, hi, rows_per_shape, grid, SHAPES, lambda shape, r: r % 3 == 2 and shape in ("uniform", "trend"))


# ------------------------------------------------------------------------------ comparison
def _check(got, ref, label, kw=None):
    """every bar on every row -> (tested rows, cells below the p floor, worst z error, worst relative p error)"""
    t = RS.check_common(got, ref, FLOAT_FIELDS, ("p", "z", "j"), label)
    if kw is not None:
        assert np.array_equal(got["tested"], kw["tested"]), label
        for name in FLOAT_FIELDS:
            RS.assert_same_bits(got[name], kw[name], (label, name, "kruskal"))
    bad = np.flatnonzero(got["j"] != ref["j"])
    assert bad.size == 0, (label, "j", bad[:5].tolist(), got["j"][bad[:5]], ref["j"][bad[:5]])
    z, zr = got["z"][t], ref["z"][t]
    err_z = np.abs(z - zr) / np.maximum(1.0, np.abs(zr))
    worst_z = float(err_z.max()) if err_z.size else 0.0
    zero = ref["zero_num"][t]
    p = got["p"][t]
    print(f"{label}: rows {t.size} tested {int(t.sum())} worst z err {worst_z:.3g} largest |z| {np.abs(zr).max() if zr.size else 0:.3g}",
          end=" ")
    assert worst_z <= Z_TOL, (label, "z", worst_z)
    assert not _bits(z)[zero].any() and np.all(p[zero] == 1.0), (label, "zero numerator")
    below, worst_p = RS.check_p(p, ref["p"][t], label)
    return int(t.sum()), below, worst_z, worst_p


def _both(ctx, ps, sets, grid, label):
    """the host call against the referee, numpy and ctx.kruskal on the same arguments"""
    got = ctx.jonckheere(ps, sets)
    return got, _check(got, JR.table_reference(ps, sets, grid), label, kw=ctx.kruskal(ps, sets))


# ------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "general"])
def test_parity(ctx, grid):
    """every k x size range x value shape (the trend shape among them), NaNs, rows with a starved set: 3-decimal PS values
    (the histogram kernel) and float32 values off the grid with random mantissas and exact duplicates (the sorting
    kernel; keys of the referee are the dense rank of the float32 values)"""
    rng = np.random.default_rng(1811 + grid)
    tested = below = 0
    for k in KS:
        for lo, hi in SIZE_RANGES:
            sets, s = draw_sets(rng, k, lo, hi)
            assert sum(g.size for g in sets) <= N_LIMIT
            ps = _table(rng, sets, s, hi, 3, grid)
            assert bool(np.all(_on_grid(ps[:, np.concatenate(sets)]))) == grid
            _, (a, b, _, _) = _both(ctx, ps, sets, grid, f"{'grid' if grid else 'general'} k={k} sizes {lo}..{hi}")
            tested += a
            below += b
    assert tested > 250, tested
    RS.check_floor_share(tested, below, "parity")


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "general"])
def test_every_set_count(ctx, grid):
    """every k = 2..64 with sets of 3..5 columns, five rows each (one per value shape): the lane-per-set bookkeeping at each k"""
    rng = np.random.default_rng(1813 + grid)
    for k in range(2, 65):
        sets, s = draw_sets(rng, k, 3, 5, spare=2)
        ps = _table(rng, sets, s, 5, 1, grid)
        _both(ctx, ps, sets, grid, f"k={k}")


# ------------------------------------------------------------------------------ edge values
def test_edge_values(ctx):
    """signed zeros tie, subnormals are distinct, one ulp off the grid, values that clamp, sets of exactly 3 (the rows of
    the Kruskal-Wallis sweeps, each grid row also with one value moved off the grid), a set of ten -0.0"""
    ps, sets, names = _edge_rows()
    _both(ctx, ps, sets, False, "edge rows")
    zs, zsets = _zero_sum_rows()
    _both(ctx, zs, zsets, False, "a set of ten -0.0")
    r = names.index("-0.0 among +0.0 (one tie group)")
    ref = JR.row_reference(ps[r], sets, False)
    assert ref["j"] == JR.row_reference(np.abs(ps[r]), sets, False)["j"]            # the signed zeros tie
    r = names.index("subnormals next to 0.0 (distinct values)")
    flushed = np.where(np.abs(ps[r]) < np.finfo(np.float32).tiny, np.float32(0), ps[r])
    assert JR.row_reference(flushed, sets, False)["z"] != JR.row_reference(ps[r], sets, False)["z"]   # and the subnormals do not


@pytest.mark.filterwarnings("ignore:overflow encountered")      # numpy's own mean of FLT_MAX values
def test_edge_rows_off_the_grid(ctx):
    """FLT_MAX; one value off the grid in an otherwise 3-decimal row sends the row to the sorting kernel, which gives the J
    of the row's dense-rank restatement; all-equal rows; rows where every set is internally constant"""
    f = np.float32
    big = np.finfo(np.float32).max
    sets = [np.arange(0, 5, dtype=np.int32), np.arange(5, 9, dtype=np.int32), np.arange(9, 15, dtype=np.int32)]
    rng = np.random.default_rng(1814)
    base = (rng.integers(0, 1001, size=15) / 1000.0).astype(np.float32)
    moved = base.copy()
    moved[7] = np.nextafter(base[7], f(2))
    rows = np.stack([
        np.array([big, -big, 0.5, 0.25, big, 0.1, big, -big, 0.3, 0.2, 0.9, big, -big, 0.0, 0.7], np.float32),
        base, moved,
        np.full(15, 0.5, np.float32), np.full(15, f(0.1234567)), np.full(15, big), np.full(15, -0.0, np.float32),
        np.repeat(np.array([0.2, 0.6, 0.4], np.float32), [5, 4, 6]),                    # every set constant, on the grid
        np.repeat(np.array([0.2000001, 0.6, 0.4], np.float32), [5, 4, 6]),              # and off it
        np.repeat(np.array([0.3, 0.3, 0.7], np.float32), [5, 4, 6]),                    # two sets share their constant
    ])
    rows[3, 2] = np.nan
    got, _ = _both(ctx, rows, sets, False, "off-grid edge rows")
    assert got["tested"].all()
    assert np.all(_on_grid(base)) and not np.all(_on_grid(moved))
    dense = (np.unique(moved, return_inverse=True)[1] / 1000.0).astype(np.float32)      # the row restated on the grid
    again = ctx.jonckheere(np.stack([dense]), sets)
    assert got["j"][2] == again["j"][0] and _bits(got["z"])[2] == _bits(again["z"])[0] and _bits(got["p"])[2] == _bits(again["p"])[0]
    for r in (3, 4, 5, 6):          # (row 5: np.median of an even count of FLT_MAX is inf, and so is delta, as numpy's)
        assert got["z"][r] == 0.0 and got["p"][r] == 1.0 and (got["delta"][r] == 0.0 or r == 5), r
    assert got["j"][3] == (4 * 4 + 4 * 6 + 4 * 6) / 2 and got["j"][4] == (5 * 4 + 5 * 6 + 4 * 6) / 2
    assert got["j"][7] == 5 * 4 + 5 * 6 and got["z"][7] > 0                            # 0.2 < 0.6, 0.2 < 0.4, 0.6 > 0.4
    assert _bits(got["z"])[8] == _bits(got["z"])[7] and _bits(got["p"])[8] == _bits(got["p"])[7]
    assert got["j"][9] == 5 * 4 / 2 + 5 * 6 + 4 * 6


# ------------------------------------------------------------------------------ limits
LIMIT_SPLITS = {"2 x 8192": [8192, 8192], "64 x 256": [256] * 64, "8191 + 8193": [8191, 8193], "3 + 8192": [3, 8192]}


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "general"])
@pytest.mark.parametrize("split", list(LIMIT_SPLITS))
def test_rows_at_the_limit(ctx, split, grid):
    """16384 selected columns, the most a call accepts (and a set of exactly 3 beside one of 8192): four rows.  The
    variance numerator needs its 128 bits here and a set above 8192 values its two-piece mean."""
    sizes = LIMIT_SPLITS[split]
    rng = np.random.default_rng(1815 + len(sizes) + sizes[0])
    s = sum(sizes)
    perm = rng.permutation(s).astype(np.int32)
    sets = [np.sort(g) for g in np.split(perm, np.cumsum(sizes)[:-1])]
    v = rng.random((4, s))
    for i, g in enumerate(sets):                                     # row 0: a trend; row 1: none; row 2: few levels; row 3: NaNs
        v[0, g] = 0.5 + 0.02 * (i / (len(sets) - 1) - 0.5) + 0.2 * rng.standard_normal(g.size)
    v[2] = rng.choice([0.1, 0.5, 0.9], size=s)
    ps = (np.rint(np.clip(v, 0, 1) * 1000.0) / 1000.0).astype(np.float32)
    if not grid:
        ps = ps * np.float32(0.9) + np.float32(0.0123)               # same order, same ties (see _twin)
        ps[1] = rng.random(s, dtype=np.float32) * np.float32(3) - np.float32(1)
        ps[1, rng.integers(0, s, 500)] = ps[1, rng.integers(0, s, 500)]
    ps[3, rng.random(s) < 0.02] = np.nan
    if sizes[0] == 3:
        ps[3, sets[0]] = ps[0, sets[0]]                              # the set of 3 keeps its 3
    _both(ctx, ps, sets, grid, f"{split} {'grid' if grid else 'general'}")


# ------------------------------------------------------------------------------ symmetries
@functools.lru_cache(maxsize=None)
def _symmetry_table():
    rng = np.random.default_rng(1816)
    sets, s = draw_sets(rng, 5, 4, 12, spare=4)
    grid = _table(rng, sets, s, 12, 7, True)[:32]
    off = _table(rng, sets, s, 12, 7, False)[:32]
    return np.ascontiguousarray(np.concatenate([grid, off])), sets, s


def test_reversed_set_order(ctx):
    """the sets in reversed order: -z, the same p and J -> sum_{i<j} n_i n_j - J, bit for bit"""
    ps, sets, s = _symmetry_table()
    a, b = ctx.jonckheere(ps, sets), ctx.jonckheere(ps, sets[::-1])
    t = a["tested"].astype(bool)
    assert np.array_equal(a["tested"], b["tested"]) and 40 < t.sum() < 64 and (a["z"] != 0).sum() > 40
    assert np.array_equal(_bits(b["z"][t]), _bits(-a["z"][t])) and np.array_equal(_bits(a["p"]), _bits(b["p"]))
    kept = np.stack([(~np.isnan(ps[:, g])).sum(axis=1) for g in sets])
    m2 = (kept.sum(axis=0) ** 2 - (kept ** 2).sum(axis=0)) // 2
    assert np.array_equal((a["j"] + b["j"])[t], m2[t].astype(np.float64))
    for name in ("med", "mean"):
        assert np.array_equal(_bits(b[name]), _bits(a[name][::-1]))
    assert np.array_equal(_bits(a["delta"]), _bits(b["delta"]))


def test_relabelled_columns(ctx):
    """the same values at other column indices (the sets following their columns): identical outputs"""
    ps, sets, s = _symmetry_table()
    perm = np.random.default_rng(1817).permutation(s)
    moved = np.empty_like(ps)
    moved[:, perm] = ps                                              # column c is now column perm[c]
    a, b = ctx.jonckheere(ps, sets), ctx.jonckheere(moved, [perm[g].astype(np.int32) for g in sets])
    for name in a:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name


def test_two_sets_equal_the_stratified_rank_sum_test_with_one_stratum(ctx):
    """k = 2: z = -z of ctx.ranksum_strata with one stratum (tie-corrected Mann-Whitney; its z > 0 when set 1 is larger)
    within 1e-12, same tested mask, medians and means"""
    ps, sets, s = _symmetry_table()
    g1, g2 = np.concatenate(sets[:2]), np.concatenate(sets[2:])
    jt = ctx.jonckheere(ps, [g1, g2])
    st = ctx.ranksum_strata(ps, g1, g2, np.zeros(g1.size, np.int32), np.zeros(g2.size, np.int32))
    assert np.array_equal(jt["tested"], st["tested"]) and jt["tested"].sum() > 50
    assert np.all(np.abs(jt["z"] + st["z"]) <= 1e-12 * np.maximum(1.0, np.abs(st["z"])))
    assert np.all(np.abs(jt["p"] - st["p"]) <= P_RTOL * st["p"])
    assert np.array_equal(jt["med"][0], st["med1"]) and np.array_equal(jt["med"][1], st["med2"])
    assert np.array_equal(jt["mean"][0], st["mean1"]) and np.array_equal(jt["mean"][1], st["mean2"])


# ------------------------------------------------------------------------------ row-count paths
@functools.lru_cache(maxsize=None)
def _palette_reference():
    rows, sets, _ = palette()
    return JR.table_reference(rows, sets, False)


def _dev_outputs(ctx, n, k, with_j=True):
    shapes = dict(tested=((n,), np.uint8), p=((n,), np.float64), z=((n,), np.float64), j=((n,), np.float64),
                  med=((k, n), np.float32), mean=((k, n), np.float32), delta=((n,), np.float32))
    if not with_j:
        del shapes["j"]
    return {name: ctx.empty(shape, dtype).memset(0x5A) for name, (shape, dtype) in shapes.items()}


@pytest.mark.parametrize("ch", CHS)
def test_rows_per_wave(ctx, ch):
    """ch rows per wave in the grid kernel (and, for ch = 64 and 32, the sorting kernel's grid-stride loop over chunks of
    256 rows with KW_REDO rows among tested, untested and grid rows): every row of every output against the referee on
    the palette of the Kruskal-Wallis sweeps, scattered through its index.  The ch = 64 table also goes through
    sdice_jonckheere_dev with the J output absent: the other outputs equal the host call's bit for bit."""
    from splicedice_amd.engine import kruskal_sets
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    rows, sets, _ = palette()
    idx = palette_index(n)
    ps = np.ascontiguousarray(rows[idx])
    got = ctx.jonckheere(ps, sets)
    _check(got, _scatter(_palette_reference(), idx), f"ch={ch} n={n} on {cus} CUs")
    if ch != 64:
        return
    assert n > 256 * 8 * cus
    cols, set_ptr = kruskal_sets(sets, PALETTE_S)
    d_ps, d_cols = ctx.to_device(ps), ctx.to_device(cols)
    out = _dev_outputs(ctx, n, 3, with_j=False)
    try:
        ctx.jonckheere_dev(d_ps, d_cols, set_ptr, out)
        for name in out:
            bad = np.argwhere(_bits(out[name].to_host()) != _bits(got[name]))
            assert bad.size == 0, ("sdice_jonckheere_dev without J", name, len(bad), bad[:5].tolist())
    finally:
        for d in (d_ps, d_cols, *out.values()):
            d.free()


def test_fewer_rows_than_a_chunk_no_rows_and_row_slices(ctx):
    """5 rows (less than any wave chunk), n = 0 through both entry points, and row slices of a resident table through
    sdice_jonckheere_dev with an offset: the slice's outputs are the host call's on those rows"""
    from splicedice_amd.engine import kruskal_sets
    rows, sets, _ = palette()
    ref = _palette_reference()
    pick = np.array([3, 45, 90, 130, 170])
    _check(ctx.jonckheere(rows[pick], sets), _scatter(ref, pick), "5 rows")
    empty = ctx.jonckheere(np.zeros((0, PALETTE_S), np.float32), sets)
    assert empty["tested"].shape == (0,) and empty["med"].shape == (3, 0)
    cols, set_ptr = kruskal_sets(sets, PALETTE_S)
    none = C.c_void_p(None)
    rc = ctx.lib.sdice_jonckheere_dev(ctx.h, 0, PALETTE_S, none, none, set_ptr.ctypes.data_as(C.c_void_p), 3, *[none] * 7)
    assert rc == 0
    n = rows.shape[0]
    d_ps, d_cols = ctx.to_device(rows), ctx.to_device(cols)
    try:
        for a, m in ((0, 1), (7, 64), (100, 180), (n - 3, 3)):
            out = _dev_outputs(ctx, m, 3)
            try:
                ctx.jonckheere_dev(d_ps.offset(a * PALETTE_S, (m, PALETTE_S)), d_cols, set_ptr, out)
                got = {name: out[name].to_host() for name in out}
            finally:
                for d in out.values():
                    d.free()
            _check(got, _scatter(ref, np.arange(a, a + m)), f"rows {a}..{a + m}")
    finally:
        d_ps.free()
        d_cols.free()


# ------------------------------------------------------------------------------ the p ladder
def test_p_ladder(ctx):
    """8 sets of 128, the shift between neighbouring sets growing row by row until the sets are in perfect order: p walks
    from about 1 down through 1e-280 (z = 37.4 for 8 x 100 in perfect order).  1e-9 relative above the floor, below 2e-280
    under it; the off-grid twin through the sorting kernel gives the same z and p bit for bit."""
    rng = np.random.default_rng(1818)
    k, m, steps = 8, 128, 40
    perm = rng.permutation(k * m)
    sets = [np.sort(perm[i * m: (i + 1) * m]).astype(np.int32) for i in range(k)]
    width = np.r_[0.0, np.geomspace(0.002, 1.0 / k, steps - 1)]
    ps = np.empty((steps, k * m), np.float32)
    for t in range(steps):
        v = rng.random(k * m) * (1.0 / k)
        for i, g in enumerate(sets):
            v[g] += i * width[t]
        ps[t] = (np.rint(v * 1000.0) / 1000.0).astype(np.float32)
        if t % 5 == 4:
            ps[t, rng.random(k * m) < 0.01] = np.nan
    ref = JR.table_reference(ps, sets, True)
    assert ref["p"].max() > 0.05 and (ref["p"] < P_FLOOR).sum() >= 2 and ((ref["p"] >= P_FLOOR) & (ref["p"] < 1e-200)).any()
    for lo, hi in ((1e-3, 1.0), (1e-20, 1e-3), (1e-100, 1e-20), (1e-200, 1e-100)):
        assert ((ref["p"] >= lo) & (ref["p"] < hi)).any(), (lo, hi)
    got = ctx.jonckheere(ps, sets)
    _check(got, ref, "p ladder", kw=ctx.kruskal(ps, sets))
    tw = ctx.jonckheere(_twin(ps, np.concatenate(sets)), sets)
    for name in ("tested", "p", "z", "j"):
        assert np.array_equal(_bits(tw[name]), _bits(got[name])), name


# ------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("case", ["k=1", "k=65", "empty set", "N over the limit", "column in two sets"])
def test_errors_leave_the_outputs_untouched(ctx, case):
    n = 3
    if case == "k=1":
        s, cols, set_ptr, k = 10, np.arange(5), [0, 5], 1
    elif case == "k=65":
        s, cols, set_ptr, k = 200, np.arange(195), np.arange(0, 196, 3), 65
    elif case == "empty set":
        s, cols, set_ptr, k = 10, np.arange(8), [0, 4, 4, 8], 3
    elif case == "N over the limit":
        s, cols, set_ptr, k = N_LIMIT + 1, np.arange(N_LIMIT + 1), [0, 8000, N_LIMIT + 1], 2
    else:
        s, cols, set_ptr, k = 10, [0, 1, 2, 3, 4, 2], [0, 3, 6], 2
    ps = np.full((n, s), 0.5, dtype=np.float32)
    kk = max(k, 2)
    outs = dict(tested=np.full(n, 7, np.uint8), p=np.full(n, -3.0), z=np.full(n, -4.0), j=np.full(n, -8.0),
                med=np.full((kk, n), -5.0, np.float32), mean=np.full((kk, n), -6.0, np.float32), delta=np.full(n, -7.0, np.float32))
    before = {x: v.copy() for x, v in outs.items()}
    rc = RS.raw_call(ctx, "sdice_jonckheere", ps, (cols, set_ptr, k), outs, OUTS)
    assert rc < 0, case
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    if case == "N over the limit":
        assert b"16384" in ctx.lib.sdice_last_error() and b"sdice_jonckheere" in ctx.lib.sdice_last_error()
    # the context still works
    ok = ctx.jonckheere(np.full((2, 9), 0.25, np.float32), [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    assert ok["tested"].tolist() == [1, 1] and ok["p"].tolist() == [1.0, 1.0]


def test_engine_refuses_a_column_in_two_sets_before_any_launch(ctx):
    with pytest.raises(ValueError, match="one set only"):
        ctx.jonckheere(np.zeros((2, 9), np.float32), [[0, 1, 2], [3, 4, 5], [6, 7, 0]])


# ------------------------------------------------------------------------------ command line
def _write_cli_inputs(tmp_path):
    """120 rows x 20 samples, three manifests (dose 0 < dose 1 < dose 2; the second names a sample the table lacks, two
    columns belong to no set): rising, falling and flat rows, heavy ties, all-equal rows, rows with a starved set"""
    rng = np.random.default_rng(1819)
    n, s = 120, 20
    samples, _ = RS.ps_names(n, s)
    member = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, -1, -1])
    slope = rng.uniform(-0.25, 0.25, size=(n, 1)) * (np.arange(n)[:, None] % 3 != 0)
    v = np.clip(0.5 + slope * (member[None, :] - 1) + 0.12 * rng.standard_normal((n, s)), 0, 1)
    v[:20] = np.round(v[:20] * 4) / 4                                      # heavy ties
    text = np.where(rng.random((n, s)) < 0.07, "nan", np.char.mod("%.3f", v))
    text[20:26] = "0.500"                                                  # all-equal rows stay in the table
    text[30:36][:, np.flatnonzero(member == 1)[1:]] = "nan"                # the second set keeps one value: rows dropped
    groups = [[samples[j] for j in np.flatnonzero(member == i)] for i in range(3)]
    groups[1] = groups[1][::-1] + ["not_in_the_table"]
    path, manifests, names = RS.write_ps_inputs(tmp_path, text, [(g, "A") for g in groups])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, manifests, [np.flatnonzero(member == i) for i in range(3)], names, matrix


@pytest.mark.parametrize("gtf", [False, True])
def test_cli_trend(ctx, golden_dir, tmp_path, gtf):
    """compare_sample_sets -mx --trend on a 120 x 20 table and three manifests: byte for byte the table formatted here from
    the referee's values (numpy's float32 cells, the referee's z and p, the oracle's BH of that p) with the writer's rules;
    and, cell by cell, the -mx table of the same inputs in every column but z / H, p-value and corrected"""
    from splicedice_amd import compare_sample_sets as css
    table, manifests, sets, names, matrix = _write_cli_inputs(tmp_path)
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    outs = {}
    for trend in (True, False):
        outs[trend] = str(tmp_path / f"out{int(trend)}.tsv")
        css.run_with(argparse.Namespace(psiSPLICEDICE=table, manifest1=manifests[0], manifest2=manifests[1],
                                        moreManifests=manifests[2:], trend=trend, annotation=anno, outputFile=outs[trend]), ctx=ctx)
    ref = JR.table_reference(matrix, sets, True)
    keep = np.flatnonzero(ref["tested"])
    assert 100 < keep.size < 120 and set(range(20, 26)) <= set(keep.tolist()) and not set(range(30, 36)) & set(keep.tolist())
    assert (ref["z"][keep] > 2).sum() > 5 and (ref["z"][keep] < -2).sum() > 5
    q = O.bh_fdr(ref["p"][keep])
    header = ["event"] + [f"mean{i}" for i in (1, 2, 3)] + [f"median{i}" for i in (1, 2, 3)] + ["delta", "z", "p-value", "corrected"]
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if gtf else [""] * keep.size
    lines = ["\t".join(header + (["gene", "overlapping", "transcript_id"] if gtf else []))]
    for i, r in enumerate(keep):
        cells = [*ref["mean"][:, r], *ref["med"][:, r], ref["delta"][r], np.float64(ref["z"][r]), np.float64(ref["p"][r]),
                 np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + sfx[i])
    want = ("\n".join(lines) + "\n").encode()
    got = open(outs[True], "rb").read()
    if got != want:                                                  # name the first cell that differs
        for a, b in zip(got.decode().split("\n"), want.decode().split("\n")):
            assert a == b, (a, b)
    assert got == want
    trend_cells = [ln.split("\t") for ln in got.decode()[:-1].split("\n")]
    plain_cells = [ln.split("\t") for ln in open(outs[False]).read()[:-1].split("\n")]
    assert len(trend_cells) == len(plain_cells) and plain_cells[0][8] == "H" and trend_cells[0][8] == "z"
    for a, b in zip(trend_cells, plain_cells):
        assert a[:8] == b[:8] and a[11:] == b[11:] and len(a) == len(b) == (14 if gtf else 11)
