"""Dense loci: clustering (cluster_fast.hip), PS on the device path with reach words (ps.hip) and the shard pipelines
that cluster their own range (distributed.py), on fixtures whose degrees, reaches and tile totals are known in closed
form and sit on both sides of every threshold at which the kernels change code path:

  cluster_fast.hip  a row list longer than KMAX = 16 (16-bit list in LDS -> the row walks global memory again), a
                    neighbour more than 32 767 rows away, backward walks past HB = 256 rows before the 512-row tile and
                    forward walks past HF = 128 rows after it, `exact` off (one junction longer than the chromosome
                    span), a tile list total above STAGE = 11 x 512 (unstaged tile), reach words saturating at 255;
  ps.hip            tile list total above 16 R (gen-1) or min(16 R, 3 T) (gen-2), (degree + 1) x tile max count >= 2^24
                    or degree >= 254 (fast item -> slow item), neighbours beyond the halo capacity.

The clustering reference is oracle.cluster_csr; the PS reference is oracle.calculate_psi_vectorised's arithmetic with
the exclusion sums taken as an int64 sparse product (pinned against the oracle on small fixtures by a CPU test).
Tests without the gpu mark check the fixtures themselves and run without a GPU.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_loci_fixtures import (  # noqa: E402
    ASYNC_DENSE, ASYNC_FITS, CLUSTER_FIXTURES, F24, HB, HF, KMAX, NB_T, PS_FIXTURES, S, STAGE, STAR_CAP, T_PS,
    _Layout, _row_reach, _tile_totals, counts, junctions, oracle_csr, ps_reference,
)
from oracle import oracle_np as O  # noqa: E402


# ------------------------------------------------------------------------------ CPU: the fixtures reach their thresholds
def test_fixtures_are_in_row_order_and_distinct():
    for name in PS_FIXTURES:
        row_of, row_ptr, col = oracle_csr(name)
        assert np.array_equal(row_of, np.arange(row_of.size)), name
        cr, left, right, st = junctions(name)
        assert (left >= 0).all() and (right >= left).all()
        keys = np.stack([cr, left, right, st]).astype(np.int64)
        assert np.unique(keys, axis=1).shape[1] == cr.size, name


def test_fixture_degrees_reaches_and_tile_totals():
    deg = {name: np.diff(oracle_csr(name)[1]) for name in PS_FIXTURES}
    reach = {name: _row_reach(*oracle_csr(name)[1:]) for name in PS_FIXTURES}
    # KMAX: lists of 16, 17 and 18 entries, interior rows 16 and 18
    assert {KMAX, KMAX + 1, KMAX + 2} <= set(deg["kmax"].tolist()) and deg["kmax"].max() == KMAX + 2
    assert (deg["kmax"] == KMAX + 1).sum() >= 4
    # STAGE: 10.9 / 11 / 11.1 entries per row around 5632
    assert _tile_totals(oracle_csr("stage")[1], NB_T).tolist() == [5580, 5630, 5632, 5634, 5684, 5632]
    # HF, HB and the reach words: reaches 127 .. 129 and 255 .. 257 (degree 2 x reach inside a ladder)
    assert {HF - 1, HF, HF + 1} <= set(reach["hf"].tolist()) and reach["hf"].max() == HF + 1
    assert {HB - 1, HB, HB + 1} <= set(reach["hb"].tolist()) and deg["hb"].max() == 2 * (HB + 1)
    # stars: long rows of degree 252 .. 256 and 300, short rows of degree 1
    assert sorted(deg["star"][deg["star"] > 1].tolist()) == [252, 253, 254, 255, 256, 300]
    assert set(deg["star"].tolist()) == {0, 1, 252, 253, 254, 255, 256, 300}
    # giant span: distances beyond 32 767 rows, and a length that turns `exact` off for every window
    cr, left, right, _ = junctions("giant")
    assert reach["giant"].max() == 40000 and deg["giant"].max() == 40000
    assert all((right - left).max() > np.ptp(left[cr == c]) for c in np.unique(cr))
    # mixed strands: strands alternate row by row; chromosome changes inside 512-row tiles
    cr, _, _, st = junctions("strands")
    assert np.array_equal(st, np.tile([0, 1], st.size // 2))
    changes = np.flatnonzero(np.diff(cr)) + 1
    assert changes.size == 4 and (changes % NB_T != 0).all()
    # fans: tiles above STAGE, degree 999
    assert (_tile_totals(oracle_csr("fans")[1], NB_T) > STAGE).sum() >= 3 and deg["fans"].max() == 999
    assert 0 < _tile_totals(oracle_csr("fans")[1], NB_T)[0] <= STAGE
    # PS list totals at the LDS staging bounds
    t64 = _tile_totals(oracle_csr("nk64")[1], 64).tolist()
    assert t64[:9] == [500, 1024, 1025, 1023, 1024, 1026, 1025, 1024, 700]
    t256 = _tile_totals(oracle_csr("nk256")[1], 256).tolist()
    assert t256[:9] == [1000, 3072, 3073, 3071, 4096, 4097, 4095, 3072, 2000]
    assert 3 * T_PS == 3072 and 16 * 256 == 4096


def test_async_list_classes():
    fits = lambda f: oracle_csr(f)[2].size <= 16 * oracle_csr(f)[0].size + 1024      # noqa: E731
    assert all(fits(f) for f in ASYNC_FITS) and not any(fits(f) for f in ASYNC_DENSE)
    assert set(ASYNC_FITS) | set(ASYNC_DENSE) == set(PS_FIXTURES)


def test_giant_fixture_has_rows_of_17_earlier_neighbours():
    """with `exact` off every backward walk runs in global memory, where a list entry past the 16th is not kept: rows
    whose 17 entries are all earlier rows depend on the KMAX redo alone"""
    row_of, row_ptr, col = oracle_csr("giant")
    rows = np.repeat(np.arange(row_of.size), np.diff(row_ptr))
    later = np.bincount(rows[col > rows], minlength=row_of.size)
    rows17 = np.flatnonzero((np.diff(row_ptr) == 17) & (later == 0))
    assert ((np.diff(row_ptr) == 16) & (later == 0)).sum() >= 3
    staged = np.flatnonzero(_tile_totals(row_ptr, NB_T) <= STAGE)
    assert np.isin(np.unique(rows17 // NB_T), staged).sum() >= 2


def _fast_item_block(c, row_ptr, col, R, r, halo=16):
    """why row r may not take the gen-2 fast item under ps.tile_rows R (ps.hip): the conditions other than the degree
    cutoff -- tile list total within min(16 R, 3 T), (degree + 1) x window max count < 2^24, every neighbour inside
    the tile -- as a list of the ones that fail (the window max count is taken over `halo` more rows on either side)"""
    lo = r // R * R
    hi = min(lo + R, row_ptr.size - 1)
    deg = int(row_ptr[r + 1] - row_ptr[r])
    nb = col[row_ptr[r]:row_ptr[r + 1]]
    cmax = int(c[max(lo - halo, 0):hi + halo].max())
    out = []
    if row_ptr[hi] - row_ptr[lo] > min(16 * R, 3 * T_PS):
        out.append("list total")
    if (deg + 1) * cmax >= F24:
        out.append("count bound")
    if nb.size and (nb.min() < lo or nb.max() >= hi):
        out.append("neighbour outside the tile")
    return out


def test_star_fixture_straddles_the_degree_cutoff():
    """under ps.tile_rows 256 the long rows of degree 252 and 253 meet every condition of the fast item, and those of
    degree 254 and 255 every one but `degree < 254`: only the cutoff sends them to the slow item.  Their sums come
    within 3 % of 2^24 (32-bit sums, float32 quotient on the fast side)"""
    _, row_ptr, col = oracle_csr("star")
    c = counts("star")
    deg = np.diff(row_ptr)
    for k in (252, 253, 254, 255):
        r = int(np.flatnonzero(deg == k)[0])
        assert r % 256 == 0
        assert _fast_item_block(c, row_ptr, col, 256, r) == [], k
        assert int(c[r, 0]) + int(c[col[row_ptr[r]:row_ptr[r + 1]], 0].sum()) == (k + 1) * STAR_CAP > 0.97 * F24
    r = int(np.flatnonzero(deg == 256)[0])               # (its last short row is the next tile's first)
    assert _fast_item_block(c, row_ptr, col, 256, r) == ["neighbour outside the tile"]
    r = int(np.flatnonzero(deg == 300)[0])
    assert "count bound" in _fast_item_block(c, row_ptr, col, 256, r)


def _cmax_tiles():
    """per 64-row tile of the "cmax" fixture: (max over rows of (degree + 1) x tile max count, largest incl + excl,
    whether that largest sum is odd)"""
    row_ptr, col = oracle_csr("cmax")[1:]
    c = counts("cmax")
    _, excl = ps_reference(c, row_ptr, col)
    tot = excl + c
    deg = np.diff(row_ptr)
    out = []
    for a in range(0, c.shape[0], 64):
        cm = int(c[a:a + 64].max())
        out.append((int((deg[a:a + 64] + 1).max()) * cm, int(tot[a:a + 64].max()), int(tot[a:a + 64].max()) % 2 == 1))
    return out


def test_cmax_fixture_straddles_the_fast_item_bound():
    tiles = _cmax_tiles()
    assert len(tiles) == 12
    assert all(t == (F24 - 1, F24 - 1, True) for t in tiles[0:4])
    assert all(t == (F24, F24, False) for t in tiles[4:8])
    assert all(t == (F24 + 33, F24 + 33, True) for t in tiles[8:12])
    # the third regime's sums are all odd and above 2^24
    row_ptr, col = oracle_csr("cmax")[1:]
    c = counts("cmax")
    tot = ps_reference(c, row_ptr, col)[1] + c
    big = tot[512:768][np.diff(row_ptr)[512:768] == 16]
    assert (big > F24).all() and (big % 2 == 1).all()


def test_cmax_fixture_catches_a_float32_quotient_past_the_bound():
    """what the fast item computes (exact 32-bit sums, a correctly rounded float32 quotient of float32 operands) equals
    the reference up to (degree + 1) x cmax = 2^24 - 1, and differs from it somewhere in the 2^24 + 33 regime: a fast
    path one step too loose cannot pass the GPU test"""
    row_ptr, col = oracle_csr("cmax")[1:]
    c = counts("cmax")
    ps, excl = ps_reference(c, row_ptr, col)
    with np.errstate(invalid="ignore", divide="ignore"):
        f32 = c.astype(np.float32) / (c.astype(np.int64) + excl).astype(np.float32)
    assert np.array_equal(f32[:256], ps[:256], equal_nan=True)
    assert (f32[512:768] != ps[512:768]).sum() >= 10


@pytest.mark.parametrize("name", ["kmax", "stage", "star", "strands", "nk64", "cmax"])
def test_sparse_ps_reference_equals_oracle(name):
    _, row_ptr, col = oracle_csr(name)
    c = counts(name)
    ps, excl = ps_reference(c, row_ptr, col)
    want_ps, want_excl = O.calculate_psi_vectorised(c, row_ptr, col)
    assert np.array_equal(excl, want_excl)
    assert np.array_equal(ps, want_ps, equal_nan=True)
    assert np.isnan(ps).any() or name == "cmax"


def test_sparse_ps_reference_beyond_2_32():
    _, row_ptr, col = oracle_csr("star")
    c = counts("star")
    ps, excl = ps_reference(c, row_ptr, col)
    assert excl.max() > 2 ** 32
    r = int(np.flatnonzero(np.diff(row_ptr) == 300)[0])
    assert excl[r, :4].min() > 2 ** 32                # (columns 0 .. 3 hold counts near 2^24)
    assert np.array_equal(excl[r], c[col[row_ptr[r]:row_ptr[r + 1]]].astype(np.int64).sum(0))


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("name", ["kmax", "hb", "star", "giant"])
def test_shard_plan_junctions_equals_csr_plan(name, world):
    from splicedice_amd import shard
    _, row_ptr, col = oracle_csr(name)
    plan = shard.shard_plan_junctions(*junctions(name), world)
    assert plan == shard.shard_plan(row_ptr, col, world)
    if name == "giant":                    # the halo of the giant junction's rank covers its whole chromosome
        assert max(p["ext_hi"] - p["ext_lo"] for p in plan) > 40000


def test_shard_ladder_is_denser_than_an_asynchronous_list():
    row_of, row_ptr, col = shard_problem()[1]
    n = row_of.size
    assert col.size > 16 * n + 1024
    from splicedice_amd import shard
    plan = shard.shard_plan_junctions(*shard_problem()[0], 3)
    assert plan == shard.shard_plan(row_ptr, col, 3)
    for p in plan:
        rows = p["ext_hi"] - p["ext_lo"]
        assert row_ptr[p["ext_hi"]] - row_ptr[p["ext_lo"]] > 16 * rows + 1024
    assert sum((p["ext_lo"] < p["own_lo"]) + (p["ext_hi"] > p["own_hi"]) for p in plan) >= 2        # shards with halos


# ------------------------------------------------------------------------------ GPU: clustering
def _check_csr(got, want, what):
    for g, w, part in zip(got, want, ("row_of", "row_ptr", "col")):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {part}"


@pytest.mark.gpu
@pytest.mark.parametrize("lds_cap", [0, 64])
@pytest.mark.parametrize("nb_grid", [0, 3])
@pytest.mark.parametrize("name", CLUSTER_FIXTURES + ("nk256", "cmax"))
def test_cluster_dense_vs_oracle(ctx, name, nb_grid, lds_cap):
    with ctx.params({"cluster.nb_grid": nb_grid, "cluster.lds_cap": lds_cap}):
        got = ctx.cluster(*junctions(name))
    _check_csr(got, oracle_csr(name), name)


def _dev_cluster(c, name, sync):
    d = [c.to_device(x) for x in junctions(name)]
    n = d[0].shape[0]
    d_row_of, d_row_ptr = c.empty(n, np.int32), c.empty(n + 1, np.int64)
    d_col, nnz = c.cluster_dev(*d, d_row_of, d_row_ptr, sync=sync)
    return d, d_row_of, d_row_ptr, d_col, nnz


def _dev_result(d_row_of, d_row_ptr, d_col, nnz):
    return d_row_of.to_host(), d_row_ptr.to_host(), d_col.offset(0, (nnz,)).to_host() if nnz else np.zeros(0, np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ASYNC_FITS)
def test_cluster_dev_async_chain(ctx, name):
    """cluster_dev (asynchronous) -> cluster_status on the session context, where the list fits its 16 n + 1024
    entries; the chain is then checked synchronously too"""
    want = oracle_csr(name)
    _, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(ctx, name, sync=False)
    assert nnz is None
    nnz, reach = ctx.cluster_status()
    assert nnz == want[2].size
    assert reach == int(_row_reach(*want[1:]).max())
    _check_csr(_dev_result(d_row_of, d_row_ptr, d_col, nnz), want, name)
    _, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(ctx, name, sync=True)
    _check_csr(_dev_result(d_row_of, d_row_ptr, d_col, nnz), want, name)


@pytest.mark.gpu
def test_cluster_dev_async_fresh_context():
    """a context whose list has never grown: an asynchronous call on a range denser than 16 entries per row reports the
    capacity at the next sync; a synchronous call grows the list (to nnz + nnz / 8 + 1024, and it never shrinks) and
    is exact; asynchronous calls that fit are exact"""
    from splicedice_amd.engine import Context, SdiceError
    c = Context(0)
    try:
        cap = 0
        failed = 0
        for name in ASYNC_DENSE:
            want = oracle_csr(name)
            n, nnz_want = want[0].size, want[2].size
            cap = max(cap, 16 * n + 1024)
            _, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(c, name, sync=False)
            if nnz_want > cap:
                with pytest.raises(SdiceError, match="capacity"):
                    c.sync()
                rp = d_row_ptr.to_host()
                assert (np.diff(rp) >= 0).all() and rp[-1] <= cap          # clamped to the buffer
                failed += 1
            else:
                assert c.cluster_status()[0] == nnz_want
                _check_csr(_dev_result(d_row_of, d_row_ptr, d_col, nnz_want), want, name)
            _, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(c, name, sync=True)
            assert nnz == nnz_want
            _check_csr(_dev_result(d_row_of, d_row_ptr, d_col, nnz), want, name)
            if nnz_want > cap:
                cap = nnz_want + nnz_want // 8 + 1024
            _, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(c, name, sync=False)     # now it fits
            assert c.cluster_status() == (nnz_want, int(_row_reach(*want[1:]).max()))
            _check_csr(_dev_result(d_row_of, d_row_ptr, d_col, nnz_want), want, name)
        assert failed == 4                   # (kmax fits the list that strands grew)
    finally:
        c.close()


# ------------------------------------------------------------------------------ GPU: PS on the device path
@functools.lru_cache(maxsize=None)
def _ps_want(name):
    ps, excl = ps_reference(counts(name), *oracle_csr(name)[1:])
    return ps, excl, O.quantize3_fast(ps)


@pytest.mark.gpu
@pytest.mark.parametrize("gen1", [0, 1])
@pytest.mark.parametrize("name", PS_FIXTURES)
def test_ps_dev_on_device_lists(ctx, name, gen1):
    """cluster_dev -> ps_dev on the context's own list (the only way the reach words are used), bit for bit: PS with
    its NaNs, int64 exclusion sums; reach words on and off, the fused '.3f' store on and off, tiles auto / 64 / 256"""
    want_ps, want_excl, want_q = _ps_want(name)
    n = want_ps.shape[0]
    cnt = counts(name)
    d, d_row_of, d_row_ptr, d_col, nnz = _dev_cluster(ctx, name, sync=True)
    assert nnz == oracle_csr(name)[2].size
    d_counts = ctx.to_device(cnt, np.int32)
    d_excl, d_ps = ctx.empty((n, S), np.int64), ctx.empty((n, S), np.float32)
    bad = []
    for use_reach in (1, 0):
        for q3 in (0, 1):
            for tile_rows in (0, 64, 256):
                knobs = {"ps.gen1": gen1, "ps.use_reach": use_reach, "ps.quantize3": q3, "ps.tile_rows": tile_rows}
                with ctx.params(knobs):
                    d_excl.memset(0xFF)
                    d_ps.memset(0xFF)
                    ctx.ps_dev(d_counts, d_row_ptr, d_col, d_excl, d_ps)
                    ps, excl = d_ps.to_host(), d_excl.to_host()
                if not np.array_equal(excl, want_excl):
                    bad.append((knobs, "excl", np.argwhere(excl != want_excl)[:4].tolist()))
                w = want_q if q3 else want_ps
                if not np.array_equal(ps, w, equal_nan=True):
                    diff = ~((ps == w) | (np.isnan(ps) & np.isnan(w)))
                    bad.append((knobs, "ps", np.argwhere(diff)[:4].tolist()))
    assert not bad, bad


# ------------------------------------------------------------------------------ GPU: shard pipelines on a fresh context
SHARD_N, SHARD_M, SHARD_S = 20000, 20, 24


@functools.lru_cache(maxsize=None)
def shard_problem():
    """a ladder of 20 000 rows of degree 40 (an asynchronous clustering sizes its list at 16 per row) and its counts"""
    lay = _Layout().ladder(SHARD_N // 2, SHARD_M)
    lay.new_chrom()
    lay.ladder(SHARD_N - SHARD_N // 2, SHARD_M)
    junc = lay.arrays()
    csr = O.cluster_csr(*junc)
    rng = np.random.default_rng(20)
    cnt = rng.integers(0, 30, (SHARD_N, SHARD_S)).astype(np.int32)
    cnt[rng.random(SHARD_N) < 0.05] = 0
    return junc, csr, cnt


SHARD_SAMPLE = np.sort(np.random.default_rng(22).choice(SHARD_N, 1500, replace=False))


@functools.lru_cache(maxsize=None)
def _shard_compare_want():
    """compare_rows of the oracle on a fixed sample of rows (rows are independent up to BH)"""
    junc, (_, row_ptr, col), cnt = shard_problem()
    ps = O.quantize3_fast(ps_reference(cnt, row_ptr, col)[0])
    return O.compare_rows(ps[SHARD_SAMPLE], np.arange(0, 12, dtype=np.int32), np.arange(12, 24, dtype=np.int32))


def _check_compare(out, want, lo, hi):
    """out: rows [lo, hi); want: the oracle on SHARD_SAMPLE"""
    sel = (SHARD_SAMPLE >= lo) & (SHARD_SAMPLE < hi)
    rows = SHARD_SAMPLE[sel] - lo
    assert rows.size > 100
    t = want["tested"][sel].astype(bool)
    assert np.array_equal(out["tested"][rows], want["tested"][sel])
    for k in ("z", "med1", "med2", "mean1", "mean2", "delta"):
        assert np.array_equal(out[k][rows][t], want[k][sel][t]), k
    np.testing.assert_allclose(out["p"][rows][t], want["p"][sel][t], rtol=1e-9, atol=0)
    tt = out["tested"].astype(bool)
    np.testing.assert_allclose(out["corrected"][tt], O.bh_fdr(out["p"][tt]), rtol=1e-9, atol=0)


@pytest.mark.gpu
def test_compare_shards_own_dense_ranges_on_a_fresh_context(ctx):
    """CompareShard in junction mode on a context whose list has never grown (3-way plan, two steps each) equals CSR
    mode and the oracle; then quant_compare_sharded with junctions_ext at world 1 on the same context"""
    from splicedice_amd import distributed, shard
    from splicedice_amd.engine import Context
    junc, (_, row_ptr, col), cnt = shard_problem()
    n, s = SHARD_N, SHARD_S
    g1, g2 = np.arange(0, 12, dtype=np.int32), np.arange(12, 24, dtype=np.int32)
    want = _shard_compare_want()
    plan = shard.shard_plan_junctions(*junc, 3)
    fresh = Context(0)
    try:
        for part in plan:
            a, b = part["ext_lo"], part["ext_hi"]
            ext, jext = np.ascontiguousarray(cnt[a:b]), tuple(x[a:b] for x in junc)
            rp, cl = shard.local_csr(row_ptr, col, part)
            got = {}
            for mode in ("junctions", "csr"):
                sh = distributed.CompareShard(fresh, distributed.SingleComm(), n, s, [part], g1, g2)
                try:
                    sh.load(ext, junctions=jext) if mode == "junctions" else sh.load(ext, rp, cl)
                    sh.step()
                    sh.step()
                    fresh.sync()
                    got[mode] = sh.result()
                finally:
                    sh.free()
            for k, v in got["csr"].items():
                assert np.array_equal(v, got["junctions"][k], equal_nan=True), k
            _check_compare(got["junctions"], want, part["own_lo"], part["own_hi"])
        plan1 = shard.shard_plan_junctions(*junc, 1)
        out = distributed.quant_compare_sharded(fresh, distributed.SingleComm(), cnt, None, None, g1, g2, plan=plan1,
                                                junctions_ext=junc)
    finally:
        fresh.close()
    _check_compare(out, want, 0, n)
    ref = distributed.quant_compare_sharded(ctx, distributed.SingleComm(), cnt, row_ptr, col, g1, g2)
    for k in ("tested", "p", "z", "corrected", "med1", "med2", "mean1", "mean2", "delta"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k


@pytest.mark.gpu
def test_pairwise_shards_own_dense_ranges_on_a_fresh_context(ctx):
    """PairwiseShard (fisher, correction "none") in junction mode on a context whose list has never grown equals CSR
    mode, its exclusion sums equal the reference and its p-values the oracle's; then pairwise_sharded with
    junctions_ext at world 1 on the same context"""
    from splicedice_amd import distributed, shard
    from splicedice_amd.engine import Context
    junc, (_, row_ptr, col), cnt = shard_problem()
    n, s = SHARD_N, 6
    cnt6 = np.ascontiguousarray(cnt[:, :s])
    _, want_excl = ps_reference(cnt6, row_ptr, col)
    rng = np.random.default_rng(21)
    sample = np.sort(rng.choice(n, 150, replace=False))
    want_p = O.fisher_pairs(cnt6[sample], want_excl[sample])
    plan = shard.shard_plan_junctions(*junc, 3)
    fresh = Context(0)
    try:
        for part in plan:
            a, b = part["ext_lo"], part["ext_hi"]
            lo, hi = part["own_lo"], part["own_hi"]
            ext, jext = np.ascontiguousarray(cnt6[a:b]), tuple(x[a:b] for x in junc)
            rp, cl = shard.local_csr(row_ptr, col, part)
            got = {}
            for mode in ("junctions", "csr"):
                sh = distributed.PairwiseShard(fresh, distributed.SingleComm(), n, s, [part], "none", "fisher")
                try:
                    sh.load(ext, junctions=jext) if mode == "junctions" else sh.load(ext, rp, cl)
                    sh.step()
                    sh.step()
                    got[mode] = sh.result()
                    excl = sh.d_excl.to_host()[lo - a:hi - a]
                finally:
                    sh.free()
                assert np.array_equal(excl, want_excl[lo:hi]), mode
            assert np.array_equal(got["csr"], got["junctions"])
            mine = sample[(sample >= lo) & (sample < hi)]
            np.testing.assert_allclose(got["junctions"][mine - lo], want_p[np.searchsorted(sample, mine)], rtol=1e-9, atol=0)
        plan1 = shard.shard_plan_junctions(*junc, 1)
        out = distributed.pairwise_sharded(fresh, distributed.SingleComm(), cnt6, None, None, correction="none", plan=plan1,
                                           junctions_ext=junc)
    finally:
        fresh.close()
    assert out["own"] == (0, n)
    np.testing.assert_allclose(out["p"][sample], want_p, rtol=1e-9, atol=0)
    ref = distributed.pairwise_sharded(ctx, distributed.SingleComm(), cnt6, row_ptr, col, correction="none")
    assert np.array_equal(out["p"], ref["p"])
