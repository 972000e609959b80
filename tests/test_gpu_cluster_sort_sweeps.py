"""The sort stage of the fast clustering (sample_rank_kernel, bucket_scatter_kernel, bucket_sort_kernel of
cluster_fast.hip) on every path a bucket can take, at the thresholds between them, under every knob that steers it,
and through its whole-chain fallback.

The path table (classes A..H) is in test_cluster_sort_cpu.py, which proves on the host that the fixtures of
cluster_sort_fixtures.py reach every class under the knobs set here.  All checks are integer equality:
  * row_of and row_ptr whole against cluster_referee (one lexsort; closed-form degrees);
  * col against cluster_referee.row_list (brute force over all rows) for 256 seeded rows, the first and the last
    row of every bucket of the plan, and rows 0 and n - 1; small sparse tables also whole against oracle_np.cluster_csr;
  * the same three arrays from the generic chain (cluster.generic = 1), whole, bit for bit.

Not tested: the sample sort's refusal branch (a sub-bucket above 1024 keys falls back to the network).  Which keys
share a sub-bucket follows from the bucket's slot order, i.e. from the order in which the scatter kernel's atomics
land, so no input drives it deterministically, and a statistical test is not wanted.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_referee as CR  # noqa: E402
import cluster_sort_fixtures as FX  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd import synth  # noqa: E402
from splicedice_amd.engine import SdiceError  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = {"cluster.generic": 1}
TOUCHED = set()                       # every knob this module sets; the last test reads them all back


def _params(ctx, knobs):
    TOUCHED.update(knobs)
    return ctx.params(knobs)


# ---------------------------------------------------------------------------------------------- references, built once
_tables, _refs = {}, {}


def _table(key, make):
    if key not in _tables:
        a = make()
        for x in a:
            x.setflags(write=False)
        _tables[key] = a
    return _tables[key]


def _fixture(name):
    return _table(("fx", name), lambda: FX.build(name))


def _gene(n, seed, **kw):
    return _table(("gene", n, seed, tuple(sorted(kw.items()))), lambda: synth.make_junctions(n, seed, **kw))


class _Ref:
    def __init__(self, a):
        self.row_of = CR.row_order(*a)
        self.row_ptr = CR.row_ptr(*a)
        self.lister = CR.RowLister(*a)
        self.n = a[0].size


def _ref(key, a):
    if key not in _refs:
        _refs[key] = _Ref(a)
    return _refs[key]


def _check_rows(got, ref, plan, seed, what):
    """col of the sampled rows against the brute-force lists"""
    row_ptr, col = got[1], got[2]
    n = ref.n
    rng = np.random.default_rng([seed, 0x5A])
    picked = [rng.integers(0, n, size=min(256, n)), [0, n - 1]]
    if plan is not None:
        full = plan.count > 0
        picked += [plan.start[full], plan.start[full] + plan.count[full] - 1]
    for r in np.unique(np.concatenate(picked)).tolist():
        want = ref.lister(r)
        assert np.array_equal(col[row_ptr[r]:row_ptr[r + 1]], want), (what, "row", r)


def _check(ctx, key, a, knobs, plan=None, whole=False, generic=True):
    """fast path under `knobs` against the referee (and the oracle when `whole`), generic chain against the fast path"""
    ref = _ref(key, a)
    with _params(ctx, knobs):
        got = ctx.cluster(*a)
        assert np.array_equal(got[0], ref.row_of), (key, "row_of")
        assert np.array_equal(got[1], ref.row_ptr), (key, "row_ptr")
        assert got[2].size == ref.row_ptr[-1]
        _check_rows(got, ref, plan, 11, key)
        if generic:
            with _params(ctx, GENERIC):
                gen = ctx.cluster(*a)
            for g, w, what in zip(gen, got, ("row_of", "row_ptr", "col")):
                assert np.array_equal(g, w), (key, "generic", what)
    if whole:
        for g, w, what in zip(got, O.cluster_csr(*a), ("row_of", "row_ptr", "col")):
            assert np.array_equal(g, w), (key, "oracle", what)
    return got


def _same(got, want, what):
    for g, w, part in zip(got, want, ("row_of", "row_ptr", "col")):
        assert np.array_equal(g, w), (what, part)


class _Dev:
    """one table on the device, with result buffers"""

    def __init__(self, ctx, a):
        self.ctx, self.n = ctx, a[0].size
        self.d = [ctx.to_device(x) for x in a]
        self.row_of, self.row_ptr = ctx.empty(self.n, np.int32), ctx.empty(self.n + 1, np.int64)

    def run(self, sync=True):
        self.d_col, nnz = self.ctx.cluster_dev(*self.d, self.row_of, self.row_ptr, sync=sync)
        if not sync:
            return None
        return self.row_of.to_host(), self.row_ptr.to_host(), self.d_col.to_host()

    def finish(self):
        """resolve an asynchronous run -> the three arrays"""
        nnz, _ = self.ctx.cluster_status()
        return self.row_of.to_host(), self.row_ptr.to_host(), self.d_col.offset(0, (nnz,)).to_host()


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_every_bucket_class(ctx, name):
    """Each fixture under its knobs; test_cluster_sort_cpu.py shows that together they reach classes A..H (the class-H
    fixture is answered by the generic chain: the synchronous fallback)."""
    f = FX.FIXTURES[name]
    a = _fixture(name)
    _check(ctx, ("fx", name), a, f["knobs"], plan=FX.plan(name), whole=f["whole"])


# ---------------------------------------------------------------------------------------------- 2
SINGLE = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]


@pytest.mark.parametrize("sample_sort", [1, 0])
def test_single_bucket_sizes(ctx, sample_sort):
    """One bucket (n <= bucket_mean: no sample, no splitter) at the sizes around a wave, SS_MIN = 512, the sample
    sort's 16 x 64 sub-bucket grid and the last size before a second bucket; with the LDS sample sort and with the
    network.  Then bucket_mean = 256 at 255 / 256 / 257: the step from one bucket to two (S = 2 * spb sample keys)."""
    for n in SINGLE:
        a = _gene(n, 200 + n, n_chrom=2)
        plan = CR.sort_plan(a[0], a[1], a[2])
        assert plan.B == 1
        _check(ctx, ("single", n), a, {"cluster.sample_sort": sample_sort}, plan=plan, whole=True)
    for n, B in [(255, 1), (256, 1), (257, 2)]:
        a = _gene(n, 300 + n, n_chrom=2)
        plan = CR.sort_plan(a[0], a[1], a[2], bucket_mean=256)
        assert plan.B == B and plan.S == (0 if B == 1 else 24)
        _check(ctx, ("mean256", n), a, {"cluster.sample_sort": sample_sort, "cluster.bucket_mean": 256}, plan=plan, whole=True)


# ---------------------------------------------------------------------------------------------- 3
def test_sample_sort_off_equals_on(ctx):
    """cluster.sample_sort = 0 (the workgroup-wide network for every packed bucket) gives the arrays of the default on
    a gene-shaped table and on the fixtures whose largest bucket sits at 2081, 6400 (class C) and 6401 (class D)"""
    cases = [(("gene", 70_000, 52), _gene(70_000, 52), {})]
    cases += [(("fx", name), _fixture(name), FX.FIXTURES[name]["knobs"]) for name in ("two_buckets_2081", "group_6400", "group_6401")]
    for key, a, knobs in cases:
        on = _check(ctx, key, a, knobs, generic=False)
        with _params(ctx, {**knobs, "cluster.sample_sort": 0}):
            off = ctx.cluster(*a)
        _same(off, on, (key, "sample_sort 0"))


# ---------------------------------------------------------------------------------------------- 4
def test_bucket_mean_and_spb_grid(ctx):
    """Every (bucket_mean, spb) pair, in and out of range, gives the arrays of the default knobs: out-of-range values
    fall back to the defaults, in-range ones only move the bucket borders (some pairs, spb = 2 with small buckets
    among them, overflow a slot and are answered by the generic chain)."""
    tables = [(("gene", 40_000, 53), _gene(40_000, 53), True), (("gene1", 70_000, 54), _gene(70_000, 54, n_chrom=1), False)]
    for key, a, whole in tables:
        base = _check(ctx, key, a, {}, whole=whole)
        dev = _Dev(ctx, a)
        for bm in (0, 255, 256, 512, 1000, 2048, 2049):
            for spb in (0, 1, 2, 3, 8, 12, 64, 65):
                with _params(ctx, {"cluster.bucket_mean": bm, "cluster.spb": spb}):
                    _same(dev.run(), base, (key, bm, spb))


# ---------------------------------------------------------------------------------------------- 5
SWITCH = 1 << 19


@pytest.mark.parametrize("n", [SWITCH, SWITCH + 1])
def test_scatter_tile_switch(ctx, n):
    """bucket_scatter_kernel<512> (tiles of 2048 keys) up to 2^19 junctions, <1024> (4096) beyond"""
    a = _gene(n, 55)
    _check(ctx, ("gene", n, 55), a, {}, plan=CR.sort_plan(a[0], a[1], a[2]))


# ---------------------------------------------------------------------------------------------- 6
def test_slot_overflow_falls_back(ctx):
    over, below = _fixture(FX.OVERFLOW), _fixture(FX.BELOW_OVERFLOW)
    knobs = FX.FIXTURES[FX.OVERFLOW]["knobs"]
    ref = _ref(("fx", FX.OVERFLOW), over)
    plan = FX.plan(FX.OVERFLOW)
    assert plan.overflow and plan.count.max() == plan.slot_cap + 1
    ctx.prof_enable(1)
    try:
        with _params(ctx, knobs):
            # synchronous: the generic chain redoes everything -- and only one key above the capacity
            ctx.prof_reset()
            got = ctx.cluster(*over)
            assert ctx.prof_query("bucket_sort_kernel")[0] == 1          # the fast path was selected ...
            assert ctx.prof_query("radix_hist_kernel")[0] > 0            # ... and gave way to the radix chain
            assert np.array_equal(got[0], ref.row_of) and np.array_equal(got[1], ref.row_ptr)
            _check_rows(got, ref, plan, 12, "overflow")
            ctx.prof_reset()
            got_below = ctx.cluster(*below)
            assert ctx.prof_query("bucket_sort_kernel")[0] == 1
            assert ctx.prof_query("radix_hist_kernel")[0] == 0           # slot_cap keys in a slot of slot_cap: no overflow
            rb = _ref(("fx", FX.BELOW_OVERFLOW), below)
            assert np.array_equal(got_below[0], rb.row_of) and np.array_equal(got_below[1], rb.row_ptr)
    finally:
        ctx.prof_enable(0)
    with _params(ctx, knobs):
        dev, ok = _Dev(ctx, over), _Dev(ctx, below)
        dev.row_ptr.memset(0xFF)
        assert dev.run(sync=False) is None
        with pytest.raises(SdiceError, match="bucket overflowed"):
            ctx.sync()
        assert not dev.row_ptr.to_host().any()                           # every list empty: safe for a dependent launch
        ctx.sync()                                                       # the report was consumed
        _same(dev.run(), got, "synchronous call after the report")
        # the overflow survives a valid asynchronous chain enqueued behind it (sticky status word)
        dev.run(sync=False)
        ok.run(sync=False)
        with pytest.raises(SdiceError, match="bucket overflowed"):
            ctx.sync()
        ctx.sync()
        ok.run(sync=False)
        _same(ok.finish(), got_below, "asynchronous chain after the report")


# ---------------------------------------------------------------------------------------------- 7
def _expect_duplicate(ctx, a, knobs, what):
    with _params(ctx, knobs):
        with pytest.raises(SdiceError, match="duplicate"):
            ctx.cluster(*a)
        dev = _Dev(ctx, a)
        dev.run(sync=False)
        with pytest.raises(SdiceError, match="duplicate"):
            ctx.sync()
        assert not dev.row_ptr.to_host().any(), what
        ctx.sync()


DUP_CASES = [("A", "gene300k_spb2"), ("C", "group_6400"), ("D", "group_6401"), ("E", "group_8193"), ("F", "wide_4096"),
             ("G", "wide_4097")]


@pytest.mark.parametrize("cls,name", DUP_CASES)
def test_duplicates_in_every_sort_path(ctx, cls, name):
    """One junction copied over another of the same bucket: the duplicate scan behind every sort must see it (packed
    keys behind A, C, D; the unpacked scan on the LDS buffer behind F and on the HBM slot behind E, G).  The bucket
    and its class come from sort_plan on the modified table."""
    f = FX.FIXTURES[name]
    a = [x.copy() for x in _fixture(name)]
    plan = FX.plan(name)
    b = int(plan.buckets(cls)[np.argmax(plan.count[plan.buckets(cls)])])
    members = np.setdiff1d(np.flatnonzero(plan.bucket_of == b), plan.sample_pos)
    rng = np.random.default_rng(70 + ord(cls))
    i, j = rng.choice(members, size=2, replace=False)
    for x in a:
        x[j] = x[i]
    after = FX.plan(name, a)
    assert after.bucket_of[i] == after.bucket_of[j] == b and after.cls[b] == cls and after.count[b] == plan.count[b]
    _expect_duplicate(ctx, a, f["knobs"], (cls, name))


def test_duplicate_across_a_scan_stride(ctx):
    """the two copies at sorted positions i and i + 1 of a bucket with i % 1024 == 1023: the pair that the last thread
    of the 1024-thread duplicate scan compares with the first key of the next stride"""
    src = _gene(70_000, 52)
    plan = CR.sort_plan(src[0], src[1], src[2])
    order = np.argsort(_ref(("gene", 70_000, 52), src).row_of)            # input index of every row
    done = 0
    for b in np.flatnonzero(plan.count > 1100)[:2]:
        r = int(plan.start[b]) + 1023
        i, j = int(order[r]), int(order[r + 1])
        if i in plan.sample_pos or j in plan.sample_pos:
            continue
        a = [x.copy() for x in src]
        for x in a:
            x[j] = x[i]
        after = CR.sort_plan(a[0], a[1], a[2])
        assert np.array_equal(after.count, plan.count) and after.bucket_of[i] == after.bucket_of[j] == b
        rows_after = CR.row_order(*a)                                     # (ties keep the input order: i, j adjacent)
        assert sorted([rows_after[i], rows_after[j]]) == [r, r + 1]
        _expect_duplicate(ctx, a, {}, ("stride", int(b)))
        done += 1
    assert done >= 1


# ---------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("kind", ["right_below_left", "negative_chrom", "strand_2"])
def test_invalid_in_a_late_tile(ctx, kind):
    """an invalid junction as the only key of the last scatter tile (index 2^19 of 2^19 + 1, tiles of 4096)"""
    n = SWITCH + 1
    src = _gene(n, 55)
    a = [x.copy() for x in src]
    if kind == "right_below_left":
        a[2][n - 1] = a[1][n - 1] - 1
    elif kind == "negative_chrom":
        a[0][n - 1] = -1
    else:
        a[3][n - 1] = 2
    with pytest.raises(SdiceError, match="invalid junction"):
        ctx.cluster(*a)
    dev = _Dev(ctx, a)
    dev.run(sync=False)
    with pytest.raises(SdiceError, match="invalid junction"):
        ctx.sync()
    assert not dev.row_ptr.to_host().any()
    ref = _ref(("gene", n, 55), src)
    got = ctx.cluster(*src)
    assert np.array_equal(got[0], ref.row_of) and np.array_equal(got[1], ref.row_ptr)
    _check_rows(got, ref, None, 13, kind)


# ---------------------------------------------------------------------------------------------- 9
def test_radix_rounds_knob(ctx):
    """sort.rounds = 4 (tiles of 1024 keys), 12 (3072) and 7 (out of range: 12) give identical results wherever the
    radix sort runs: both radix clustering chains, the junction union, BH on the radix path"""
    a = _gene(70_000, 52)
    ref = _ref(("gene", 70_000, 52), a)
    rng = np.random.default_rng(91)
    keys = rng.integers(0, 1 << 62, size=300_000, dtype=np.uint64)
    keys[rng.integers(0, keys.size, size=60_000)] = keys[rng.integers(0, keys.size, size=60_000)]     # repeats
    want_keys = np.unique(keys)
    p = np.maximum(rng.random(100_000) ** 3, 1e-300)
    p[rng.integers(0, p.size, size=5000)] = p[rng.integers(0, p.size, size=5000)]                      # ties
    want_q = O.bh_fdr(p)

    def run_all():
        out = {}
        for path in ("cluster.generic", "cluster.legacy"):
            with _params(ctx, {path: 1}):
                out[path] = ctx.cluster(*a)
        out["unique"] = ctx.sort_unique_u64(keys)
        with _params(ctx, {"bh.vector_path": 1}):
            out["bh"] = ctx.bh(p)
        return out

    base = run_all()
    for path in ("cluster.generic", "cluster.legacy"):
        assert np.array_equal(base[path][0], ref.row_of) and np.array_equal(base[path][1], ref.row_ptr)
        _check_rows(base[path], ref, None, 14, path)
    _same(base["cluster.legacy"], base["cluster.generic"], "legacy vs generic")
    assert np.array_equal(base["unique"], want_keys)
    print("bh radix path vs oracle_np.bh_fdr: max relative difference",
          float(np.max(np.abs(base["bh"] - want_q) / want_q)))
    assert np.array_equal(base["bh"], want_q)
    for rounds in (4, 12, 7):
        with _params(ctx, {"sort.rounds": rounds}):
            got = run_all()
        for path in ("cluster.generic", "cluster.legacy"):
            _same(got[path], base[path], (path, rounds))
        assert np.array_equal(got["unique"], base["unique"]), rounds
        assert np.array_equal(got["bh"].view(np.uint64), base["bh"].view(np.uint64)), rounds
    # (the last test of the module) every knob that was touched reads its default again
    table, name, dflt = {}, ctypes.c_char_p(), ctypes.c_int64()
    while ctx.lib.sdice_param_info(len(table), ctypes.byref(name), ctypes.byref(dflt)) == 0:
        table[name.value.decode()] = dflt.value
    assert {"sort.rounds", "cluster.generic", "cluster.legacy", "bh.vector_path"} <= TOUCHED
    for knob in sorted(TOUCHED):
        assert ctx.get_param(knob) == table[knob], knob
