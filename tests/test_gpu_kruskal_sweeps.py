"""Kruskal-Wallis sweeps: sdice_kruskal against the exact referee (tests/kruskal_referee.py) and numpy at the set counts,
rows-per-wave choices, p tails and edge values that the random parity tables of test_gpu_kruskal.py do not reach.

- set counts: a swept set keeps EVERY count 3..G (G up to 4096) beside two small companions, first, in the middle and
  last in the selection; large sets (G up to 16376, the most a call takes beside two sets of 4) at the counts where the
  pairwise-sum plan, the compaction rounds and the leaf table step.  Above 8192 kept values np.sum is NOT one pairwise
  tree: numpy adds pieces of np.getbufsize() = 8192 values, each by the tree, left to right (KR.numpy_sum);
- rows per wave: tables of 64 x compute_units x ch rows for ch = 64, 32, 8, 2 built from a palette of row kinds, every
  row of every output compared; the ch = 64 table also runs through sdice_kruskal_dev without the H output;
- p: for every k = 2..64 a ladder of rows whose p walks from about 0.5 to below the 1e-280 floor, against chi2.sf from
  mpmath at 50 digits (KR.p_exact);
- edge values: signed zeros, subnormals, values one ulp off the grid, values that clamp to keys 0 and 1000, a set of 3.

Every 3-decimal table also runs as its off-grid twin `row * 0.9 + 0.0123` (same order, same ties), which the sorting
kernel takes: H and p of the two kernels are bit-identical, both finish from the same integers.

Bars: tested, med, mean, delta bit-exact against numpy; H within 1e-12 relative of the exact
rational; p within 1e-9 relative where the referee's p >= 1e-280 and p < 2e-280 below that.

The tests without the gpu mark check the fixtures on the CPU: numpy's order restated, the counts realised, the share of
rows that tells numpy's order from one whole-array tree, the palette arrangement, the p bands per df, scipy against
mpmath."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kruskal_referee as KR  # noqa: E402
import rank_support as RS  # noqa: E402
from kset_fixtures import (CHS, KINDS, PALETTE_S, PER_KIND, _edge_rows, _zero_sum_rows, palette, palette_index)  # noqa: E402
from rank_support import (N_LIMIT, NOMINAL_CUS, P_FLOOR, PLACEMENTS, _kept_positions, _values, chunk_table_rows, tree_sum)  # noqa: E402
from rank_support import bits as _bits, on_grid as _on_grid, scatter as _scatter, twin as _twin  # noqa: E402

gpu = pytest.mark.gpu

H_RTOL = 1e-12
FLAVOURS = ("q3", "cont")           # 3-decimal values: the histogram kernel; random ** 4: the sorting kernel


# ------------------------------------------------------------------------------ comparison
def _check(got, ref, label, nv=None, p_ref=None):
    """every bar on every row -> (worst relative H error, worst relative p error at or above the floor);
    p_ref: the referee's p where it is not ref["p"] (floats; mpmath's on the ladder); nv: the kept values of the swept
    set per row, named in a failure message"""
    t = RS.check_common(got, ref, ("med", "mean", "delta"), ("p", "h"), label,
                        where=None if nv is None else lambda rows: ("kept values of the swept set", nv[rows].tolist()))
    h, hr = got["h"][t], ref["hf"][t]
    err_h = np.abs(h - hr) / np.where(hr > 0, hr, 1.0)
    worst_h = float(err_h.max()) if err_h.size else 0.0
    print(f"{label}: rows {t.size} tested {int(t.sum())} worst H rel {worst_h:.3g}", end=" ")
    assert worst_h <= H_RTOL, (label, "H", worst_h)
    return worst_h, RS.check_p(got["p"][t], (ref["p"] if p_ref is None else p_ref)[t], label)[1]


def _numpy_fields(ps, sets):
    """tested, med, mean, delta of every row by numpy alone (the rules of KR.row_reference without H and p)"""
    n, k = ps.shape[0], len(sets)
    out = dict(tested=np.zeros(n, np.uint8), med=np.zeros((k, n), np.float32), mean=np.zeros((k, n), np.float32),
               delta=np.zeros(n, np.float32))
    for r in range(n):
        kept = [ps[r, g] for g in sets]
        kept = [v[~np.isnan(v)] for v in kept]
        if any(v.size < 3 for v in kept):
            continue
        out["tested"][r] = 1
        out["med"][:, r] = [np.median(v) for v in kept]
        out["mean"][:, r] = [np.mean(v) for v in kept]
        out["delta"][r] = out["med"][:, r].max() - out["med"][:, r].min()
    return out


def _check_twin(ctx, ps, sets, got, label, nv=None):
    """the table's off-grid twin through the sorting kernel: H and p bit-identical to the grid kernel's (both kernels hand
    the same integers N, sum(t^3 - t) and D_i to kw_finish, the k quotients sorted before they are added), the float32
    fields bit-exact against numpy on the twin's own values"""
    tw = _twin(ps, np.concatenate(sets))
    got_tw = ctx.kruskal(tw, sets)
    want = _numpy_fields(tw, sets)
    for name in ("tested", "med", "mean", "delta"):
        bad = np.argwhere(got_tw[name] != want[name])
        rows = bad[:, -1]
        assert bad.size == 0, (label, "twin", name, len(bad), rows[:8].tolist(), None if nv is None else nv[rows[:8]].tolist())
    for name in ("h", "p"):
        bad = np.flatnonzero(_bits(got_tw[name]) != _bits(got[name]))
        assert bad.size == 0, (label, "twin", name, bad.size, bad[:5].tolist(), got_tw[name][bad[:5]], got[name][bad[:5]])
    return got_tw


# ------------------------------------------------------------------------------ A/B fixtures: the set-count sweep
SMALL_G = (8, 63, 64, 65, 128, 129, 1024, 1025, 4096)
LARGE_G = (7232, 7233, 8192, 8193, 14464, 14465, 16376)      # 113 * 64 and 113 * 128: where the leaf table steps


def large_counts(G):
    """the kept counts of a large swept set: small ones, the first counts of every pairwise depth, around the piece of
    8192, G - 1 and G, and 40 seeded random counts above 8192 when G has that many"""
    c = [3, 7, 8, 9, 127, 128, 129]
    for d in range(1, 8):
        c += [120 * 2 ** d + 8, 120 * 2 ** d + 9, 120 * 2 ** d + 10]
    c += [8191, 8192, 8193, 8199, 8200, 8201, 8320, 8321, G - 1, G]
    if G - 8192 >= 40:
        c += np.random.default_rng(G).choice(np.arange(8193, G + 1), 40, replace=False).tolist()
    return tuple(sorted({int(x) for x in c if 3 <= x <= G}))


def kw_sweep_table(G, flavour, slot, companions=(5, 4), counts=None):
    """-> (ps float32[rows, G + 9], sets, nv).  Three sets: a swept set of G columns and two companions; the columns
    interleave in table order (a seeded permutation, each set's columns ascending); the swept set is set number `slot`
    of the selection.  Row plan as sweep_table of the rank-sum sweeps: the swept set keeps every count of `counts`
    (default 3..G) in two rows with different NaN placements, the companions keep 3..all of their columns; the first
    row keeps 2 values of the swept set and the last row 2 of the first companion (both untested).  nv[r] is the swept
    set's kept count."""
    ca, cb = companions
    rng = np.random.default_rng(G * 8191 + slot * 31 + (flavour == "q3"))
    s = G + ca + cb
    perm = rng.permutation(s)
    swept, a, b = (np.sort(x).astype(np.int32) for x in (perm[:G], perm[G:G + ca], perm[G + ca:]))
    counts = range(3, G + 1) if counts is None else counts
    plan = [(2, ca, cb, 0)]
    for i, c in enumerate(counts):
        na, nb = 3 + i % (ca - 2), cb - i % (cb - 2)
        plan += [(c, na, nb, i % 4), (c, na, nb, (i + 2) % 4)]
    plan.append((G, 2, cb, 1))
    ps = np.full((len(plan), s), np.nan, np.float32)
    for r, (c, na, nb, pl) in enumerate(plan):
        ps[r, swept[_kept_positions(G, c, PLACEMENTS[pl], rng)]] = _values(rng, c, flavour)
        ps[r, a[_kept_positions(ca, na, PLACEMENTS[(pl + 1) % 4], rng)]] = _values(rng, na, flavour)
        ps[r, b[_kept_positions(cb, nb, PLACEMENTS[(pl + 2) % 4], rng)]] = _values(rng, nb, flavour)
    sets = [a, b]
    sets.insert(slot, swept)
    return ps, sets, np.array([c for c, _, _, _ in plan])


def _large_table(G, flavour):
    return kw_sweep_table(G, flavour, LARGE_G.index(G) % 3, companions=(4, 4), counts=large_counts(G))


def _assert_plan(ps, sets, nv, slot, G, companions, want_counts):
    s = G + sum(companions)
    assert ps.shape[1] == s and np.array_equal(np.sort(np.concatenate(sets)), np.arange(s))
    assert [g.size for g in sets] == list(np.insert(np.array(companions), slot, G))
    kept = [(~np.isnan(ps[:, g])).sum(axis=1) for g in sets]
    sw = kept.pop(slot)
    assert np.array_equal(sw, nv) and set(sw.tolist()) == {2} | set(want_counts)
    assert sw[0] == 2 and kept[0][-1] == 2 and np.all(sw[1:] >= 3)
    assert np.all(kept[0][:-1] >= 3) and np.all(kept[1] >= 3)
    assert {3, companions[0]} <= set(kept[0].tolist()) and {3, companions[1]} <= set(kept[1].tolist())
    assert np.all(np.unique(sw[1:-1], return_counts=True)[1] == 2)          # two NaN placements per count
    want = KR.row_reference(ps[0], sets, False)["tested"], KR.row_reference(ps[-1], sets, False)["tested"]
    assert want == (0, 0)


@pytest.mark.parametrize("G", SMALL_G)
def test_kw_sweep_table_realises_every_count(G):
    slot = SMALL_G.index(G) % 3
    ps, sets, nv = kw_sweep_table(G, "cont", slot)
    _assert_plan(ps, sets, nv, slot, G, (5, 4), range(3, G + 1))
    assert ps.shape[0] == 2 * (G - 2) + 2


@pytest.mark.parametrize("G", LARGE_G)
def test_kw_large_table_realises_its_counts(G):
    """the listed counts where not above G; the pairwise depths 7 and 8 of a whole-set tree (first needed at 7689 and
    15369 values) and both sides of the 8192 piece are there when G allows"""
    counts = large_counts(G)
    ps, sets, nv = _large_table(G, "q3")
    _assert_plan(ps, sets, nv, LARGE_G.index(G) % 3, G, (4, 4), counts)
    assert G + 8 <= N_LIMIT and {3, 7, 8, 9, 127, 128, 129, 248, 249, 250, 3848, 3849, 3850, G - 1, G} <= set(counts)
    assert all(c <= G for c in counts)
    if G >= 8321:
        assert {7688, 7689, 7690, 8191, 8192, 8193, 8199, 8200, 8201, 8320, 8321} <= set(counts)
        assert sum(c > 8192 for c in counts) >= 40
    if G == 16376:
        assert {15368, 15369, 15370} <= set(counts) and G + 8 == N_LIMIT


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_numpy_sums_pieces_of_8192_left_to_right(flavour):
    """np.sum of more than 8192 contiguous float32 values is the pairwise tree of every piece of np.getbufsize() values,
    the pieces added left to right, and np.mean is that sum divided by float32(n).  A numpy that sums differently shows
    itself here and not as a kernel failure."""
    assert np.getbufsize() == KR.SUM_PIECE == 8192
    rng = np.random.default_rng(8192 + (flavour == "q3"))
    lengths = np.r_[8193, 8199, 8200, 8201, 8320, 8321, 16376, 16383, 16384, rng.integers(8193, 16385, size=120)]
    for n in lengths.tolist():
        x = _values(rng, n, flavour)
        assert KR.numpy_sum(x) == np.sum(x), n
        assert np.mean(x) == KR.numpy_sum(x) / np.float32(n), n
        table = np.stack([x, x[::-1]])                            # a row of a 2-D table, as a kernel's caller holds it
        assert np.mean(table, axis=1)[0] == np.mean(x), n
    for n in rng.integers(4097, 8193, size=40).tolist() + [7688, 7689, 8191, 8192]:
        x = _values(rng, n, flavour)                              # one piece: the whole-array tree
        assert tree_sum(x) == np.sum(x) == KR.numpy_sum(x), n


# observed on the committed seeds (numpy 2.2.6): the whole-array tree differs from np.mean on 80 of 300 (q3) and
# 97 of 300 (cont) rows whose swept set keeps more than 8192 values; the floors are half of those shares
WHOLE_TREE_SHARE_FLOOR = {"q3": 0.13, "cont": 0.16}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_large_tables_tell_the_piecewise_sum_from_one_tree(flavour):
    """Over the rows of the large-set fixtures that keep more than 8192 values, one pairwise tree over the whole set (what
    the kernels did before they summed in pieces) misses np.mean on a share of rows large enough that such a kernel fails
    the sweep; the restated piecewise sum never does."""
    n = diff = 0
    for G in LARGE_G:
        ps, sets, nv = _large_table(G, flavour)
        swept = sets[LARGE_G.index(G) % 3]
        for r in np.flatnonzero(nv > KR.SUM_PIECE):
            x = ps[r, swept]
            x = x[~np.isnan(x)]
            want = np.mean(x)
            assert KR.numpy_sum(x) / np.float32(x.size) == want
            n += 1
            diff += tree_sum(x) / np.float32(x.size) != want
    print(f"{flavour}: whole-array tree differs from np.mean on {diff} of {n} rows above 8192 values")
    assert n >= 280
    assert diff >= WHOLE_TREE_SHARE_FLOOR[flavour] * n, (diff, n)


# ------------------------------------------------------------------------------ B on the GPU
def _run_sweep(ctx, ps, sets, nv, flavour, label):
    got = ctx.kruskal(ps, sets)
    ref = KR.table_reference(ps, sets, flavour == "q3")
    assert not ref["tested"][0] and not ref["tested"][-1] and ref["tested"][1:-1].all()
    _check(got, ref, label, nv)
    if flavour == "q3":
        _check_twin(ctx, ps, sets, got, label, nv)


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("G", SMALL_G)
def test_kruskal_set_count_sweep(ctx, G, flavour):
    """the swept set at every kept count 3..G, the slots rotating over G and flavour"""
    slot = (SMALL_G.index(G) + FLAVOURS.index(flavour)) % 3
    ps, sets, nv = kw_sweep_table(G, flavour, slot)
    _run_sweep(ctx, ps, sets, nv, flavour, f"sweep G={G} {flavour} slot {slot}")


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("G", LARGE_G)
def test_kruskal_large_set_sweep(ctx, G, flavour):
    """sets of up to 16376 columns beside two of 4: above 8192 kept values the mean follows np.mean only when the set is
    summed in numpy's pieces of 8192.  With one whole-set tree (kruskal.hip before the pieces) this test fails on `mean`
    at counts above 8192 for both flavours."""
    ps, sets, nv = _large_table(G, flavour)
    _run_sweep(ctx, ps, sets, nv, flavour, f"large G={G} {flavour} slot {LARGE_G.index(G) % 3}")


# ------------------------------------------------------------------------------ C: rows per wave
def test_palette_kinds_are_what_they_claim():
    rows, sets, kind = palette()
    ref = KR.table_reference(rows, sets, False)
    cols = np.concatenate(sets)
    assert cols.size == 15 and np.unique(cols).size == 15 and [g.size for g in sets] == [4, 5, 6]
    for r in range(rows.shape[0]):
        name = KINDS[kind[r]]
        sel = rows[r, cols]
        assert bool(np.all(_on_grid(sel))) == ("off" not in name), (r, name)
        assert ref["tested"][r] == (not name.endswith("starved")), (r, name)
        if name.startswith("all equal"):
            assert np.unique(sel).size == 1 and ref["hf"][r] == 0.0 and ref["p"][r] == 1.0
        if name == "grid with NaNs":
            assert np.isnan(sel).any()
    assert np.unique(rows, axis=0).shape[0] > 270              # a few hundred distinct rows
    t = ref["tested"].astype(bool) & (ref["hf"] > 0)
    assert ref["p"][t].min() >= P_FLOOR and np.unique(ref["hf"][t]).size > 100


@pytest.mark.parametrize("ch", CHS)
def test_palette_index_arrangement(ch):
    """for a nominal 256 compute units: the table selects ch and its last chunk is partial; every 64-row chunk mixes at
    least three kinds; every kind occurs at chunk positions 0 and 63, beyond row 256 * 8 * compute_units when the table
    reaches there, and in the partial last chunk as far as it has rows for them"""
    n = chunk_table_rows(ch, NOMINAL_CUS)
    idx = palette_index(n)
    kind = idx // PER_KIND
    assert idx.min() >= 0 and idx.max() < len(KINDS) * PER_KIND and np.unique(idx).size == len(KINDS) * PER_KIND
    full = kind[: n - n % 64].reshape(-1, 64)
    distinct = (np.diff(np.sort(full, axis=1), axis=1) != 0).sum(axis=1) + 1
    assert distinct.min() >= 3
    assert set(full[:, 0].tolist()) == set(full[:, 63].tolist()) == set(range(len(KINDS)))
    last = kind[n - n % ch:]
    assert 0 < last.size < ch and np.unique(last).size == min(last.size, len(KINDS))
    if ch == 64:
        stride_rows = 256 * 8 * NOMINAL_CUS                     # where the sorting kernel's grid-stride loop starts
        assert n > stride_rows and n * PALETTE_S * 4 < 90e6
        assert set(kind[stride_rows:].tolist()) == set(range(len(KINDS)))


@gpu
@pytest.mark.parametrize("ch", CHS)
def test_kruskal_rows_per_wave(ctx, ch):
    """ch rows per wave in the grid kernel (and, for ch = 64 and 32, the sorting kernel's grid-stride loop over chunks of
    256 rows with KW_REDO rows among tested, untested and grid rows): every row of every output against the referee on
    the palette, scattered through the index.  The ch = 64 table also goes through sdice_kruskal_dev with the H output
    absent: tested, p, med, mean and delta equal the host call's bit for bit."""
    from splicedice_amd.engine import kruskal_sets
    cus = ctx.device_info()["compute_units"]
    n = chunk_table_rows(ch, cus)
    rows, sets, _ = palette()
    idx = palette_index(n)
    ps = np.ascontiguousarray(rows[idx])
    got = ctx.kruskal(ps, sets)
    _check(got, _scatter(KR.table_reference(rows, sets, False), idx), f"ch={ch} n={n} on {cus} CUs")
    if ch != 64:
        return
    assert n > 256 * 8 * cus
    cols, set_ptr = kruskal_sets(sets, PALETTE_S)
    d_ps, d_cols = ctx.to_device(ps), ctx.to_device(cols)
    shapes = dict(tested=((n,), np.uint8), p=((n,), np.float64), med=((3, n), np.float32), mean=((3, n), np.float32),
                  delta=((n,), np.float32))
    out = {name: ctx.empty(shape, dtype).memset(0x5A) for name, (shape, dtype) in shapes.items()}
    try:
        ctx.kruskal_dev(d_ps, d_cols, set_ptr, out)
        for name in shapes:
            dev = out[name].to_host()
            bad = np.argwhere(dev.view(np.uint8) != got[name].view(np.uint8))
            assert bad.size == 0, ("sdice_kruskal_dev without H", name, len(bad), bad[:5].tolist())
    finally:
        for d in (d_ps, d_cols, *out.values()):
            d.free()


# ------------------------------------------------------------------------------ D: the p ladder
LADDER_KS = tuple(range(2, 65))
LADDER_STEPS = 48
LADDER_N = 4096
P_BANDS = ((1e-3, 1.0), (1e-20, 1e-3), (1e-100, 1e-20), (1e-200, 1e-100), (1e-280, 1e-200))


def ladder_table(k):
    """-> (ps float32[48, N], sets): k equal sets over N = k * (4096 // k) columns, 3-decimal values.  Set i's values lie
    in the i-th of k bands of keys; in row t a seeded share 1 - g_t of the columns has its values shuffled among them.
    The separated share g_t rises geometrically, so that H (about g^2 times its largest value N (1 - 1 / k^2)) rises
    from about df to the largest the row allows.  Every fifth row has NaNs."""
    rng = np.random.default_rng(4096 + k)
    m = LADDER_N // k
    N = k * m
    width = 1001 // k
    perm = rng.permutation(N)
    sets = [np.sort(perm[i * m: (i + 1) * m]).astype(np.int32) for i in range(k)]
    h_max = N * (1.0 - 1.0 / k ** 2)
    g = np.geomspace(0.7 * np.sqrt((k - 1) / h_max), 1.0, LADDER_STEPS)
    ps = np.empty((LADDER_STEPS, N), np.float32)
    for t in range(LADDER_STEPS):
        keys = np.empty(N, np.int64)
        for i, cols in enumerate(sets):
            keys[cols] = i * width + rng.integers(0, width, size=m)
        mix = rng.choice(N, int(round((1.0 - g[t]) * N)), replace=False)
        keys[mix] = keys[rng.permutation(mix)]
        ps[t] = (keys / 1000.0).astype(np.float32)
        if t % 5 == 4:
            ps[t, rng.random(N) < 0.01] = np.nan
    return ps, sets


@functools.lru_cache(maxsize=None)
def ladder_reference(k):
    """-> (table reference of ladder_table(k), p_exact of every row as mpmath numbers)"""
    ps, sets = ladder_table(k)
    refs = [KR.row_reference(ps[t], sets, True) for t in range(ps.shape[0])]
    assert all(r["tested"] for r in refs)
    ref = dict(tested=np.ones(len(refs), np.uint8), hf=np.array([r["hf"] for r in refs]), p=np.array([r["p"] for r in refs]),
               med=np.stack([r["med"] for r in refs], axis=1), mean=np.stack([r["mean"] for r in refs], axis=1),
               delta=np.array([r["delta"] for r in refs], np.float32))
    return ref, [KR.p_exact(r["h"], k - 1) for r in refs]


@pytest.mark.parametrize("k", LADDER_KS)
def test_ladder_covers_every_p_band(k):
    """from the referee alone: the exact p of the ladder's rows falls in every band down to 1e-280 and at least once
    below it; H starts near df"""
    ref, pe = ladder_reference(k)
    for lo, hi in P_BANDS:
        assert any(lo <= p < hi or (hi == 1.0 and p == 1.0) for p in pe), (k, lo, hi)
    assert any(p < P_FLOOR for p in pe), k
    assert ref["hf"].min() < 3 * (k - 1) + 10 and np.all(ref["hf"] > 0)


def test_scipy_chi2_sf_against_mpmath_on_the_ladder():
    """scipy's chi2.sf(float(H), df), the p referee of test_gpu_kruskal.py and of the sweeps above, within 1e-12
    relative of mpmath's 50-digit value on every ladder row with p >= 1e-280, for every df = 1..63"""
    worst = (0.0, None)
    cells = 0
    for k in LADDER_KS:
        ref, pe = ladder_reference(k)
        for t, p in enumerate(pe):
            if p < P_FLOOR:
                continue
            err = float(abs(ref["p"][t] - p) / p)
            cells += 1
            if err > worst[0]:
                worst = (err, (k - 1, ref["hf"][t], float(p)))
    print(f"scipy chi2.sf against mpmath: {cells} cells, worst relative difference {worst[0]:.3g} at (df, H, p) = {worst[1]}")
    assert cells > 30 * len(LADDER_KS)
    assert worst[0] <= 1e-12, worst


@gpu
def test_kruskal_p_ladder_every_df(ctx):
    """both kernels (the 3-decimal rows and their off-grid twins) on the ladder of every k = 2..64: H within 1e-12 of the
    exact rational, p within 1e-9 of mpmath's chi2.sf where that is >= 1e-280 and below 2e-280 where it is not; prints
    the worst relative p error per parity of df"""
    worst_h = 0.0
    worst_p = {0: 0.0, 1: 0.0}
    for k in LADDER_KS:
        ps, sets = ladder_table(k)
        ref, pe = ladder_reference(k)
        p_ref = np.array([float(p) for p in pe])               # below the float64 range: 0.0, under the floor either way
        got = ctx.kruskal(ps, sets)
        eh, ep = _check(got, ref, f"ladder k={k}", p_ref=p_ref)
        _check_twin(ctx, ps, sets, got, f"ladder k={k}")
        worst_h = max(worst_h, eh)
        worst_p[(k - 1) & 1] = max(worst_p[(k - 1) & 1], ep)
    print(f"p ladder: worst H rel {worst_h:.3g}; worst p rel for even df {worst_p[0]:.3g}, for odd df {worst_p[1]:.3g}")


# ------------------------------------------------------------------------------ E: edge values
def test_edge_rows_are_what_they_claim():
    ps, sets, names = _edge_rows()
    ref = KR.table_reference(ps, sets, False)
    assert ref["tested"].all() and len(names) == 7 + 4
    grid = np.all(_on_grid(ps), axis=1)
    on_grid = ("-0.0 among +0.0 (one tie group)", "only -0.0 in every set but one", "a set keeps exactly 3",
               "every set keeps exactly 3, ties")
    for r, name in enumerate(names):
        assert grid[r] == (name in on_grid), name
        assert (name + " / sorted" in names) == (name in on_grid), name
    r = names.index("subnormals next to 0.0 (distinct values)")
    assert np.unique(ps[r]).size == 9 and (ps[r] == 0).sum() == 5 and np.all(np.abs(ps[r]) <= np.finfo(np.float32).tiny)
    r = names.index("-0.0 among +0.0 (one tie group)")
    assert (ps[r] == 0).sum() == 11 and np.signbit(ps[r]).sum() == 6
    assert not _bits(ref["mean"][1, r: r + 1])[0] and not _bits(ref["med"][1, r: r + 1])[0]     # numpy: +0.0 of -0.0 values
    r = names.index("one ulp above and one ulp below a grid value, the grid value beside them")
    assert np.unique(ps[r, :6]).size == 6 and np.unique(ps[r, 6:11]).size == 5
    r = names.index("just outside [0, 1]: clamp to keys 0 and 1000")
    assert ps[r].max() > 1 and ps[r].min() < 0 and np.rint(ps[r].max() * 1000) == 1000 and np.rint(ps[r].min() * 1000) == 0
    kept = (~np.isnan(ps[names.index("a set keeps exactly 3")]))
    assert kept[:6].sum() == 3 and kept[6:11].sum() == 4 and kept[11:].sum() == 3
    zs, zsets = _zero_sum_rows()
    zref = KR.table_reference(zs, zsets, False)
    assert np.all(_on_grid(zs[0])) and not np.all(_on_grid(zs[1])) and zref["tested"].all()
    assert np.signbit(zs[:, :10]).all() and not _bits(zref["mean"][0]).any() and not _bits(zref["med"][0]).any()


@gpu
def test_kruskal_edge_values(ctx):
    """signed zeros, subnormals, one ulp off the grid, values that clamp, sets of exactly 3: every field bit-exact against
    numpy (a zero mean or median is +0.0 as numpy's) and the referee on dense-rank keys"""
    ps, sets, names = _edge_rows()
    got = ctx.kruskal(ps, sets)
    ref = KR.table_reference(ps, sets, False)
    for r, name in enumerate(names):
        one = {x: v[..., r: r + 1] for x, v in got.items()}
        want = {x: v[..., r: r + 1] for x, v in ref.items()}
        _check(one, want, name)
    zs, zsets = _zero_sum_rows()
    _check(ctx.kruskal(zs, zsets), KR.table_reference(zs, zsets, False), "a set of ten -0.0")
