"""A catalogue of small calls for test_gpu_call_order.py (helper module, no tests in here): one case per _dev entry point
and path that works in memory the context keeps between calls, at the smallest shape that still reaches that path.

A case has
  name      the key in CASES
  knobs     the parameters its run is made under (ctx.params)
  arena     True when its entry point allocates from the context arena (the test then looks for its traces there)
  inputs    host arrays from a fixed seed, built once and never written to
  run(ctx)  the call(s) through the _dev forms on outputs filled with 0x5A first -> {field: ndarray}
  outputs   the names of the fields run() returns
  want      {field: ndarray} from the referee the project already has for the operation, computed once
  check(got) the comparison of that operation's own test file, copied with a pointer to where it stands; most are bit for
            bit, the others carry that file's tolerance and no other

test_call_order_fixtures_cpu.py shows without a GPU that no case is degenerate.

Every _dev entry point of engine.py is here except: allgather_dev, alltoall_dev, comm_fork / comm_join (they need more than
one device and keep nothing in the context's scratch), copy2d_dev (one hipMemcpy2DAsync: no scratch, no state) and
pair_table (sdice_pair_list_pack_dev), which the two pair-list cases call to make their input.  sort_unique_u64 has a
host form only and is called through it.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_sort_fixtures as FX  # noqa: E402
import dunn_fixtures as DF  # noqa: E402
import dunn_referee as DR  # noqa: E402
import exact_referee as ER  # noqa: E402
import jonckheere_referee as JR  # noqa: E402
import kruskal_referee as KR  # noqa: E402
import ks_referee as KS  # noqa: E402
import large_path_fixtures as LP  # noqa: E402
import pair_fixtures as PF  # noqa: E402
import rank_support as RS  # noqa: E402
import sample_matrix_referee as SM  # noqa: E402
import scoring_referee as SC  # noqa: E402
import shift_referee as SH  # noqa: E402
import signedrank_referee as SR  # noqa: E402
import spearman_referee as SP  # noqa: E402
import strata_referee as VR  # noqa: E402
from bh_fixtures import bh_columns_values, bh_values  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd import synth  # noqa: E402
from splicedice_amd.engine import (GRAM_FIELDS, JONCKHEERE_FIELDS, KRUSKAL_DUNN_FIELDS, KRUSKAL_FIELDS, KS_FIELDS,  # noqa: E402
                                   RANKSUM_EXACT_FIELDS, RANKSUM_FIELDS, SHIFT_FIELDS, SPEARMAN_FIELDS, field_shapes,
                                   kruskal_sets, spearman_order)

FILL = 0x5A
F32 = ("med1", "med2", "mean1", "mean2", "delta")
CASES = {}


class Case:
    def __init__(self, name, make, run, want, check, outputs, knobs=None, arena=True, constant=()):
        self.name, self.knobs, self.arena, self.constant = name, dict(knobs or {}), arena, tuple(constant)
        self.outputs = tuple(outputs)
        self._make, self._run, self._want, self._check = make, run, want, check

    @functools.cached_property
    def inputs(self):
        x = self._make()
        for a in x.values():
            for b in (a if isinstance(a, (tuple, list)) else (a,)):
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
        return x

    @functools.cached_property
    def want(self):
        return self._want(self.inputs)

    def run(self, ctx, knobs=None):
        """under the case's knobs, or under `knobs` in their place"""
        with ctx.params(self.knobs if knobs is None else knobs):
            return self._run(ctx, self.inputs)

    def check(self, got, label=""):
        self._check(got, self.want, (self.name, label))


def _case(name, make, run, want, check, outputs, **kw):
    assert name not in CASES
    CASES[name] = Case(name, make, run, want, check, outputs, **kw)


def _alloc(ctx, spec):
    """{name: (shape, dtype)} -> device arrays holding FILL in every byte"""
    return {name: ctx.empty(shape, dtype).memset(FILL) for name, (shape, dtype) in spec.items()}


def _collect(outs, *held):
    """host copies of the outputs (the copy synchronises); the outputs and the inputs in `held` are freed"""
    got = {name: d.to_host() for name, d in outs.items()}
    for d in (*outs.values(), *held):
        d.free()
    return got


def _same(got, want, label, fields):
    for name in fields:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name)
        assert np.array_equal(RS.bits(got[name]), RS.bits(want[name])), (label, name)


# ================================================================================================ clustering, then PS
PS_COLS = 8            # a multiple of 4: rows of 16-byte vectors, the tile kernel that reads the block reach (ps.hip)
CLUSTER_LARGE, CLUSTER_SMALL = 5000, 300
# cluster_fast.hip, fast_plan: B = ceil(n / 2048) buckets and S = B * spb sample keys when B > 1, else S = 0.  With S > 0
# the rank kernel clears the status block; with S = 0 (n <= 2048) a memset does (sdice_cluster_dev).
CLUSTER_ONE_BUCKET_MAX = 2048


def cluster_inputs(n, seed):
    return dict(junctions=FX.gene(n, seed, n_chrom=3), counts=synth.make_counts(n, PS_COLS, seed + 1))


def cluster_device(ctx, junctions):
    """-> (the four device inputs, row_of, row_ptr) with the two outputs filled"""
    n = junctions[0].size
    return [ctx.to_device(a) for a in junctions], ctx.empty(n, np.int32).memset(FILL), ctx.empty(n + 1, np.int64).memset(FILL)


def ps_on(ctx, counts, d_row_ptr, d_col):
    """sdice_ps_dev on a count table in row order -> (ps, excl) on the host"""
    d_counts = ctx.to_device(counts)
    out = _alloc(ctx, dict(ps=(counts.shape, np.float32), excl=(counts.shape, np.int64)))
    ctx.ps_dev(d_counts, d_row_ptr, d_col, out["excl"], out["ps"])
    return _collect(out, d_counts)


def run_cluster_ps(ctx, x):
    d_in, d_row_of, d_row_ptr = cluster_device(ctx, x["junctions"])
    d_col, _ = ctx.cluster_dev(*d_in, d_row_of, d_row_ptr)
    got = dict(row_of=d_row_of.to_host(), row_ptr=d_row_ptr.to_host(), col=d_col.to_host())
    got.update(ps_on(ctx, x["counts"], d_row_ptr, d_col))          # the context's own col: the reach bytes are used
    for d in (*d_in, d_row_of, d_row_ptr):
        d.free()
    return got


def want_cluster_ps(x):
    row_of, row_ptr, col = O.cluster_csr(*x["junctions"])
    ps, excl = O.calculate_psi_vectorised(x["counts"], row_ptr, col)
    return dict(row_of=row_of, row_ptr=row_ptr, col=col, ps=ps, excl=excl)


def check_cluster_ps(got, want, label):
    """whole against oracle_np.cluster_csr (test_gpu_cluster_sort_sweeps.py:104, `whole`); PS as __graft_entry__.smoke holds
    it: excl equal, ps equal with NaN where the oracle has NaN"""
    for name in ("row_of", "row_ptr", "col", "excl"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (label, name)
    assert got["ps"].dtype == np.float32 and np.array_equal(got["ps"], want["ps"], equal_nan=True), (label, "ps")


for _name, _n, _knobs in (("cluster->ps", CLUSTER_LARGE, {}), ("cluster->ps one bucket", CLUSTER_SMALL, {}),
                          ("cluster generic->ps", CLUSTER_LARGE, {"cluster.generic": 1})):
    _case(_name, functools.partial(cluster_inputs, _n, 40 + _n), run_cluster_ps, want_cluster_ps, check_cluster_ps,
          ("row_of", "row_ptr", "col", "ps", "excl"), knobs=_knobs)


# ================================================================================================ junction union
def _unique_inputs():
    keys, _ = LP.junction_keys(10_000)
    return dict(keys=keys)


_case("sort_unique_u64", _unique_inputs, lambda ctx, x: dict(keys=ctx.sort_unique_u64(x["keys"])),
      lambda x: dict(keys=np.unique(x["keys"])),                       # (test_gpu_cluster_sort_sweeps.py:344, :364)
      lambda got, want, label: _same(got, want, label, ("keys",)), ("keys",))


# ================================================================================================ BH
BH_RADIX_M, BH_SAMPLESORT_M = 5000, 16_385


def _bh_inputs(m):
    rng = np.random.default_rng(m)
    return dict(p=bh_values(m, rng), tested=(rng.random(m) < 0.67).astype(np.uint8))


def _run_bh(ctx, x):
    d_p = ctx.to_device(x["p"])
    out = _alloc(ctx, dict(q=(x["p"].shape, np.float64)))
    ctx.bh_dev(d_p, out["q"])
    return _collect(out, d_p)


def _run_bh_masked(ctx, x):
    """both mask forms: a tested array, and p < 0 for the absent entries"""
    d_p, d_t = ctx.to_device(x["p"]), ctx.to_device(x["tested"])
    d_neg = ctx.to_device(np.where(x["tested"] != 0, x["p"], -1.0))
    out = _alloc(ctx, dict(q_mask=(x["p"].shape, np.float64), q_negative=(x["p"].shape, np.float64)))
    ctx.bh_masked_dev(d_p, d_t, out["q_mask"])
    ctx.bh_masked_dev(d_neg, None, out["q_negative"])
    return _collect(out, d_p, d_t, d_neg)


def _want_bh_masked(x):
    q = np.zeros(x["p"].size)
    q[x["tested"] != 0] = O.bh_fdr(x["p"][x["tested"] != 0])
    return dict(q_mask=q, q_negative=q)


# (bit for bit: test_gpu_count_sweeps.py, test_bh_vector_paths_bit_exact)
for _path, _m, _tag in ((1, BH_RADIX_M, "radix"), (2, BH_SAMPLESORT_M, "sample sort")):
    _case(f"bh vector {_tag}", functools.partial(_bh_inputs, _m), _run_bh, lambda x: dict(q=O.bh_fdr(x["p"])),
          lambda got, want, label: _same(got, want, label, ("q",)), ("q",), knobs={"bh.vector_path": _path})
    _case(f"bh vector {_tag} masked", functools.partial(_bh_inputs, _m), _run_bh_masked, _want_bh_masked,
          lambda got, want, label: _same(got, want, label, ("q_mask", "q_negative")), ("q_mask", "q_negative"),
          knobs={"bh.vector_path": _path})


def _bh_columns_inputs(n, pitch, c0, cols):
    return dict(table=bh_columns_values(n, pitch, np.random.default_rng(n + pitch)), c0=c0, cols=cols)


def _run_bh_columns(ctx, x):
    table, c0, cols = x["table"], x["c0"], x["cols"]
    n, pitch = table.shape
    d = ctx.to_device(table)
    if cols == pitch:
        ctx.bh_columns_dev(d)
    else:
        ctx.bh_columns_pitched_dev(d.offset(c0, (n * pitch - c0,)), n, cols, pitch)
    return _collect(dict(table=d))


def _want_bh_columns(x):
    want, c0, cols = x["table"].copy(), x["c0"], x["cols"]
    want[:, c0:c0 + cols] = O.bh_columns(x["table"][:, c0:c0 + cols])
    return dict(table=want)


# (bit for bit, the columns outside the range untouched: test_gpu_count_sweeps.py, test_bh_columns_pitched_range)
BH_COLUMNS_SAMPLESORT = "bh columns sample sort"
for _name, _shape, _knobs in (("bh columns radix", (1025, 4, 0, 4), {"bh.columns_path": 1}),
                              (BH_COLUMNS_SAMPLESORT, (5000, 20, 0, 20), {"bh.columns_path": 2}),
                              ("bh columns sample sort three groups", (5000, 20, 0, 20), {"bh.columns_path": 2, "bh.max_group": 8}),
                              ("bh columns pitched", (1025, 9, 3, 4), {})):
    _case(_name, functools.partial(_bh_columns_inputs, *_shape), _run_bh_columns, _want_bh_columns,
          lambda got, want, label: _same(got, want, label, ("table",)), ("table",), knobs=_knobs)


# ================================================================================================ pair tests
PAIR_PALETTES = ("zeros", "ties", "small", "thousands", "big", "tiny", "edge", "under")
PAIR_S = 6
PAIR_LIST = np.array([[0, 1], [4, 2], [0, 1], [5, 3], [1, 0]], np.int32)        # reversed pairs and a repeat


@functools.lru_cache(maxsize=None)
def pair_reference():
    return PF.PaletteRef(PAIR_PALETTES)


def _pair_inputs(listed):
    incl, excl, pid, pi = pair_reference().rows(PAIR_S, reps=8, seed=3)            # 8 palettes x 8 rows = 64
    return dict(incl=incl, excl=excl, pid=pid, pi=pi, **({"pairs": PAIR_LIST} if listed else {}))


def _pair_ids(x):
    ref = pair_reference()
    if "pairs" in x:
        return ref.ids[x["pid"][:, None], x["pi"][:, x["pairs"][:, 0]], x["pi"][:, x["pairs"][:, 1]]]
    return ref.pair_ids(x["pid"], x["pi"])


def _run_pairs(chi2, ctx, x):
    d_incl, d_excl = ctx.to_device(x["incl"]), ctx.to_device(x["excl"])
    tab = ctx.pair_table(PAIR_S, x["pairs"]) if "pairs" in x else None
    m = len(x["pairs"]) if "pairs" in x else PAIR_S * (PAIR_S - 1) // 2
    out = _alloc(ctx, dict(p=((x["incl"].shape[0], m), np.float64), **({"n_bad": (1, np.int64)} if chi2 else {})))
    if chi2:
        ctx.chi2_pairs_dev(d_incl, d_excl, out["p"], out["n_bad"], pairs=tab)
    else:
        ctx.fisher_pairs_dev(d_incl, d_excl, out["p"], pairs=tab)
    return _collect(out, d_incl, d_excl, *([tab] if tab is not None else []))


def _want_pairs(chi2, x):
    ref = pair_reference()
    p, rtol = ref.chi2() if chi2 else ref.fisher()
    ids = _pair_ids(x)
    want = dict(p=p[ids], rtol=rtol[ids])
    if chi2:
        want["n_bad"] = np.array([np.isnan(p)[ids].sum()], np.int64)
    return want


def _check_pairs(got, want, label):
    """pair_fixtures._check_fisher / _check_chi2 (pair_fixtures.py:193-201): every element within its table's rtol of the
    per-table reference, NaN where scipy refuses the table, n_bad their number"""
    if "n_bad" in want:
        assert got["n_bad"].dtype == np.int64 and np.array_equal(got["n_bad"], want["n_bad"]), (label, got["n_bad"])
    each = np.arange(want["p"].size, dtype=np.int64).reshape(want["p"].shape)
    PF.assert_p_match(got["p"], each, want["p"].reshape(-1), want["rtol"].reshape(-1), label)


for _test, _chi2 in (("fisher", False), ("chi2", True)):
    for _form, _listed in (("pairs", False), ("pair_list", True)):
        # (chi2.hip takes nothing from the arena; fisher.hip the built pair table, its row counter and row flags)
        _case(f"{_test}_{_form}", functools.partial(_pair_inputs, _listed), functools.partial(_run_pairs, _chi2),
              functools.partial(_want_pairs, _chi2), _check_pairs, ("p", "n_bad") if _chi2 else ("p",), arena=not _chi2)


# ================================================================================================ sample_gram
GRAM_TILE = 64         # gram.hip, GR_TILE: from 65 listed columns on there is a second tile, and the sums of the samples of
                       # an off-diagonal tile wait in two scratch matrices (q1, q2) that the call zeroes


def _gram_inputs(s, m):
    rng = np.random.default_rng(77 + m)
    return dict(ps=SM.random_table(rng, 200, s), cols=rng.permutation(s)[:m].astype(np.int32))


def _run_gram(ctx, x):
    d_ps, d_cols = ctx.to_device(x["ps"]), ctx.to_device(x["cols"])
    m = x["cols"].size
    out = _alloc(ctx, field_shapes(GRAM_FIELDS, (m, m)))
    ctx.sample_gram_dev(d_ps, d_cols, out)
    return _collect(out, d_ps, d_cols)


# (entry for entry: test_gpu_sample_matrix.py:21, check)
for _name, _s, _m in (("sample_gram", 15, 12), ("sample_gram two tiles", 72, GRAM_TILE + 2)):
    _case(_name, functools.partial(_gram_inputs, _s, _m), _run_gram, lambda x: SM.gram(x["ps"], x["cols"]),
          lambda got, want, label: _same(got, want, label, [f[0] for f in GRAM_FIELDS]), [f[0] for f in GRAM_FIELDS])


# ================================================================================================ the row tests
ROWS, ROW_COLS = 200, 40
G1, G2 = np.arange(0, 18, dtype=np.int32), np.arange(20, 39, dtype=np.int32)         # 18 v 19 columns
PAIR_A, PAIR_B = np.arange(0, 18, dtype=np.int32), np.arange(20, 38, dtype=np.int32)  # 18 pairs
N_STRATA = 3
SETS = [np.arange(0, 12, dtype=np.int32), np.arange(14, 27, dtype=np.int32), np.arange(27, 40, dtype=np.int32)]   # k = 3


@functools.lru_cache(maxsize=None)
def row_table():
    """float32 [200, 40]: 3-decimal values, the first 20 columns shifted row by row (so the tests have something to find),
    10 % NaN; every ninth row 45 % NaN (few enough values for the exact forms), every thirteenth 96 % (not tested), one
    row all NaN; every fifth row moved off the grid by rank_support.twin's map, so both kernels of each test run"""
    rng = np.random.default_rng(4201)
    v = rng.random((ROWS, ROW_COLS)) * 0.8 + 0.1
    v[:, :20] += 0.12 * rng.standard_normal((ROWS, 1))
    ps = (np.rint(np.clip(v, 0.0, 1.0) * 1000.0) / 1000.0).astype(np.float32)
    r = np.arange(ROWS)
    nan_frac = np.where(r % 13 == 6, 0.96, np.where(r % 9 == 4, 0.45, 0.10))
    ps[rng.random((ROWS, ROW_COLS)) < nan_frac[:, None]] = np.nan
    ps[17] = np.nan
    off = r % 5 == 2
    ps[off] = ps[off] * np.float32(0.9) + np.float32(0.0123)
    ps.setflags(write=False)
    return ps


@functools.lru_cache(maxsize=None)
def spearman_design():
    rng = np.random.default_rng(4202)
    return rng.permutation(ROW_COLS)[:30].astype(np.int32), rng.integers(0, 6, size=30).astype(np.float64)      # tied covariate


def _run_rows(entry, fields, lists, extra, ctx, x, k=None):
    """entry(d_ps, *device lists, *extra, out) on the row table"""
    d_ps = ctx.to_device(x["ps"])
    held = [ctx.to_device(v) for v in lists]
    out = _alloc(ctx, field_shapes(fields, ROWS, k))
    getattr(ctx, entry)(d_ps, *held, *extra, out)
    return _collect(out, d_ps, *held)


def _rows(name, entry, fields, lists, want, check, extra=(), k=None, run=None, **kw):
    # (the row tests reset the arena and take nothing from it)
    _case(name, lambda: dict(ps=row_table()), run or functools.partial(_run_rows, entry, fields, lists, extra, k=k),
          want, check, [f[0] for f in fields], arena=False, **kw)


def _check_ranksum(got, want, label):
    """test_gpu_count_sweeps.py:90 (_check_ranksum): tested equal, the float32 fields and z bit-exact on tested rows and
    zero elsewhere, p within 1e-9"""
    assert np.array_equal(got["tested"], want["tested"]), label
    t = want["tested"].astype(bool)
    for k in F32:
        bad = np.flatnonzero(got[k][t] != want[k][t])
        assert bad.size == 0, (label, k, bad.size, np.flatnonzero(t)[bad[:5]])
        assert not got[k][~t].any(), (label, k)
    assert np.array_equal(got["z"][t], want["z"][t]), (label, "z")
    np.testing.assert_allclose(got["p"][t], want["p"][t], rtol=RS.P_RTOL, atol=0)


_rows("ranksum", "ranksum_dev", RANKSUM_FIELDS, (G1, G2), lambda x: O.compare_rows(x["ps"], G1, G2), _check_ranksum)


Z_TOL = 1e-12          # test_gpu_strata.py:30, test_gpu_signedrank.py:28 (Z_RTOL), test_gpu_jonckheere.py:29
COND_MAX = 100.0       # test_gpu_strata.py:31


def _check_strata(got, ref, label):
    """test_gpu_strata.py:156 (check, without the plain call)"""
    t = RS.check_common(got, ref, F32, ("tested", "p", "z") + F32, label)
    cond = float(ref["cond"][t].max()) if t.any() else 0.0
    assert cond <= COND_MAX, (label, cond)
    z, zr = got["z"][t], ref["z"][t]
    err_z = np.abs(z - zr) / np.maximum(1.0, np.abs(zr))
    assert np.all(err_z <= Z_TOL), (label, float(err_z.max()))
    assert np.all(z[ref["cond"][t] == 0] == 0), label
    below, _ = RS.check_p(got["p"][t], ref["p"][t], label, quiet=True)
    RS.check_floor_share(int(t.sum()), below, label)


_rows("ranksum_strata", "ranksum_strata_dev", RANKSUM_FIELDS, (G1, G2, G1 % N_STRATA, G2 % N_STRATA),
      lambda x: VR.table_reference(x["ps"], G1, G2, G1 % N_STRATA, G2 % N_STRATA), _check_strata, extra=(N_STRATA,))


def _z_relative(got, ref, t, label):
    """the z bar of test_gpu_signedrank.py:132-137"""
    z, zr = got["z"][t], ref["z"][t]
    assert np.all(z[zr == 0] == 0), label
    err_z = np.abs(z - zr) / np.where(zr != 0, np.abs(zr), 1.0)
    assert np.all(err_z <= Z_TOL), (label, float(err_z.max()) if err_z.size else 0.0)


def _check_signedrank(got, ref, label):
    """test_gpu_signedrank.py:129 (check)"""
    t = RS.check_common(got, ref, F32, ("p", "z"), label)
    _z_relative(got, ref, t, label)
    below, _ = RS.check_p(got["p"][t], ref["p"][t], label, quiet=True)
    RS.check_floor_share(int(t.sum()), below, label)


_rows("signedrank", "signedrank_dev", RANKSUM_FIELDS, (PAIR_A, PAIR_B),
      lambda x: SR.table_reference(x["ps"], PAIR_A, PAIR_B), _check_signedrank)


def _want_exact(paired, x):
    c1, c2 = (PAIR_A, PAIR_B) if paired else (G1, G2)
    base = SR.table_reference(x["ps"], c1, c2) if paired else O.compare_rows(x["ps"], c1, c2)
    exact, p = ER.table_reference(x["ps"], c1, c2, paired)
    return dict(base, exact=exact, p_exact=p)


def _check_exact(paired, got, want, label):
    """test_gpu_exact.py:193 (check): the marks equal the referee's, none on an untested row; on the marked rows p IS the
    referee's exact p; every other field, and p on the unmarked rows, is held to the bars of the plain call"""
    assert got["exact"].dtype == np.uint8 and np.array_equal(got["exact"], want["exact"]), (label, "exact")
    assert not want["exact"][want["tested"] == 0].any(), label
    on = want["exact"] == 1
    bad = np.flatnonzero(got["p"][on] != want["p_exact"][on])
    assert bad.size == 0, (label, "exact p", np.flatnonzero(on)[bad[:5]])
    plain = dict(got, p=np.where(on, want["p"], got["p"]))             # (the asymptotic p of a marked row is not an output)
    (_check_signedrank if paired else _check_ranksum)(plain, want, label)


_rows("ranksum_exact", "ranksum_exact_dev", RANKSUM_EXACT_FIELDS, (G1, G2), functools.partial(_want_exact, False),
      functools.partial(_check_exact, False))
_rows("signedrank_exact", "signedrank_exact_dev", RANKSUM_EXACT_FIELDS, (PAIR_A, PAIR_B), functools.partial(_want_exact, True),
      functools.partial(_check_exact, True))


def _run_ks(exact, ctx, x):
    d_ps, d_g1, d_g2 = ctx.to_device(x["ps"]), ctx.to_device(G1), ctx.to_device(G2)
    out = _alloc(ctx, field_shapes(KS_FIELDS, ROWS))
    ctx.ks_dev(d_ps, d_g1, d_g2, out, exact=exact)
    return _collect(out, d_ps, d_g1, d_g2)


def _check_ks(got, ref, label):
    """test_gpu_ks.py:35 (check, without the plain call)"""
    t = RS.check_common(got, ref, F32, ("tested", "p", "d") + F32 + ("exact",), label)
    RS.assert_same_bits(got["d"], ref["d"], (label, "d"))
    assert got["exact"].dtype == np.uint8 and np.array_equal(got["exact"], ref["exact"]), (label, "exact marks")
    ex = ref["exact"].astype(bool)
    RS.assert_same_bits(got["p"][ex], ref["p"][ex], (label, "exact p"))
    below, _ = RS.check_p(got["p"][t], ref["p"][t], label, quiet=True)
    RS.check_floor_share(int(t.sum()), below, label)


_rows("ks", None, KS_FIELDS, (), lambda x: KS.table_reference(x["ps"], G1, G2, False), _check_ks,
      run=functools.partial(_run_ks, False), constant=("exact",))          # (without exact every mark is 0: test_gpu_ks.py:100)
_rows("ks exact", None, KS_FIELDS, (), lambda x: KS.table_reference(x["ps"], G1, G2, True), _check_ks,
      run=functools.partial(_run_ks, True))


SHIFT_CONF = 0.95      # (the default of shift_dev, which the case leaves in force)
# (bit for bit on every field of shift_referee.OUTS, as test_gpu_shift.py:30, check, holds them)
_rows("shift", "shift_dev", SHIFT_FIELDS, (G1, G2), lambda x: SH.table_reference(x["ps"], G1, G2, SH.zq_of(SHIFT_CONF)),
      lambda got, want, label: _same(got, want, label, SH.OUTS))


def _run_sets(entry, fields, ctx, x):
    cols, set_ptr = kruskal_sets(SETS, ROW_COLS)
    d_ps, d_cols = ctx.to_device(x["ps"]), ctx.to_device(cols)
    out = _alloc(ctx, field_shapes(fields, ROWS, len(SETS)))
    getattr(ctx, entry)(d_ps, d_cols, set_ptr, out)
    return _collect(out, d_ps, d_cols)


H_RTOL = 1e-12         # test_gpu_kruskal.py:23


def _check_kruskal(got, ref, label):
    """test_gpu_kruskal.py:34 (_check)"""
    t = RS.check_common(got, ref, ("med", "mean", "delta"), ("p", "h"), label)
    h, hr = got["h"][t], ref["hf"][t]
    err_h = np.abs(h - hr) / np.where(hr > 0, hr, 1.0)
    assert np.all(err_h <= H_RTOL), (label, float(err_h.max()))
    RS.check_p(got["p"][t], ref["p"][t], label, quiet=True)


def _check_jonckheere(got, ref, label):
    """test_gpu_jonckheere.py:42 (_check, without the kruskal call)"""
    t = RS.check_common(got, ref, ("med", "mean", "delta"), ("p", "z", "j"), label)
    bad = np.flatnonzero(got["j"] != ref["j"])
    assert bad.size == 0, (label, "j", bad[:5].tolist())
    z, zr = got["z"][t], ref["z"][t]
    err_z = np.abs(z - zr) / np.maximum(1.0, np.abs(zr))
    assert (float(err_z.max()) if err_z.size else 0.0) <= Z_TOL, (label, "z")
    zero = ref["zero_num"][t]
    p = got["p"][t]
    assert not RS.bits(z)[zero].any() and np.all(p[zero] == 1.0), (label, "zero numerator")
    RS.check_p(p, ref["p"][t], label, quiet=True)


# (the keys of both referees: the dense rank of the float32 values, which serves rows on and off the grid alike)
_rows("kruskal", None, KRUSKAL_FIELDS, (), lambda x: KR.table_reference(x["ps"], SETS, False), _check_kruskal,
      run=functools.partial(_run_sets, "kruskal_dev", KRUSKAL_FIELDS))
_rows("jonckheere", None, JONCKHEERE_FIELDS, (), lambda x: JR.table_reference(x["ps"], SETS, False), _check_jonckheere,
      run=functools.partial(_run_sets, "jonckheere_dev", JONCKHEERE_FIELDS))


def _want_dunn(x):
    """dunn_referee.table_reference, its per-row list `exact` (mpmath numbers and Fractions, for dunn_referee.close_pairs) as
    an object vector: a reference is arrays throughout"""
    want = DR.table_reference(x["ps"], SETS, False)
    exact = np.empty(ROWS, dtype=object)
    for r, e in enumerate(want["exact"]):
        exact[r] = e
    return dict(want, exact=exact)


def _check_dunn(got, ref, label):
    """test_gpu_dunn.py:34 (check): the Kruskal-Wallis fields by the bars of the kruskal case, the pair fields by
    dunn_fixtures.check_pairs"""
    _check_kruskal(got, ref, label)
    DF.check_pairs(got, ref, label)


_rows("kruskal_dunn", None, KRUSKAL_DUNN_FIELDS, (), _want_dunn, _check_dunn,
      run=functools.partial(_run_sets, "kruskal_dunn_dev", KRUSKAL_DUNN_FIELDS))


def _run_spearman(ctx, x):
    cols, xg = spearman_order(*spearman_design())
    d_ps, d_cols, d_xg = ctx.to_device(x["ps"]), ctx.to_device(cols), ctx.to_device(xg)
    out = _alloc(ctx, field_shapes(SPEARMAN_FIELDS, ROWS))
    ctx.spearman_dev(d_ps, d_cols, d_xg, out)
    return _collect(out, d_ps, d_cols, d_xg)


def _want_spearman(x):
    cols, cov = spearman_design()
    order = np.argsort(cov, kind="stable")                             # (test_gpu_spearman.py:154, sorted_design)
    return SP.table_reference(x["ps"], cols[order], cov[order])


RHO_RTOL = 1e-12       # test_gpu_spearman.py:28


def _check_spearman(got, ref, label):
    """test_gpu_spearman.py:166 (check)"""
    bad = np.flatnonzero(got["n_kept"] != ref["n_kept"])
    assert bad.size == 0 and got["n_kept"].dtype == np.int32, (label, "n_kept", bad[:5])
    t = RS.check_common(got, ref, ("med", "mean"), ("p", "rho"), label)
    r, rr = got["rho"][t], ref["rho"][t]
    edge = (rr == 0) | (np.abs(rr) == 1)
    assert np.array_equal(r[edge], rr[edge]), (label, "rho at 0 / +-1")
    err_r = np.abs(r - rr) / np.where(rr != 0, np.abs(rr), 1.0)
    p = got["p"][t]
    assert np.all(p[np.abs(rr) == 1] == 0) and np.all(p[rr == 0] == 1), (label, "p at the edges")
    assert np.all(err_r <= RHO_RTOL), (label, float(err_r.max()) if err_r.size else 0.0)
    RS.check_p(p, ref["p"][t], label, quiet=True)


_rows("spearman", None, SPEARMAN_FIELDS, (), _want_spearman, _check_spearman, run=_run_spearman)


# ================================================================================================ little or no scratch
def _similarity_inputs():
    rng = np.random.default_rng(91)                                    # (the table of test_gpu_similarity_sweeps.py:30)
    ps = np.round(rng.random((300, 12)), 3)
    ps[rng.random(ps.shape) < 0.1] = np.nan
    return dict(ps=ps, mid=np.round(rng.random(300), 3), sign=rng.integers(-1, 2, size=300).astype(np.int8))


def _run_similarity(ctx, x):
    held = [ctx.to_device(x[k]) for k in ("ps", "mid", "sign")]
    out = _alloc(ctx, dict(scores=(x["ps"].shape[1], np.int64), counts=(x["ps"].shape[1], np.int64)))
    ctx.similarity_dev(*held, out["scores"], out["counts"])
    return _collect(out, *held)


# (integer equality: test_gpu_similarity_sweeps.py:36, _check)
_case("similarity", _similarity_inputs, _run_similarity,
      lambda x: dict(zip(("scores", "counts"), SC.similarity_counts(x["ps"], x["mid"], x["sign"]))),
      lambda got, want, label: _same(got, want, label, ("scores", "counts")), ("scores", "counts"), arena=False)


def _rowstats_inputs(dtype):
    rng = np.random.default_rng(92)
    data = np.round(rng.random((300, 40)), 3).astype(dtype)
    data[rng.random(data.shape) < 0.15] = np.nan
    data[5, :] = np.nan
    return dict(data=data, idx=rng.permutation(40)[:33].astype(np.int32))


def _run_rowstats(ctx, x):
    d_data, d_idx = ctx.to_device(x["data"]), ctx.to_device(x["idx"])
    n, dt = x["data"].shape[0], x["data"].dtype
    out = _alloc(ctx, dict(mean=(n, dt), std=(n, dt), n_nan=(n, np.int32)))
    ctx.rowstats_dev(d_data, d_idx, out["mean"], out["std"], out["n_nan"])
    return _collect(out, d_data, d_idx)


def _check_rowstats(got, want, label):
    """test_gpu_rowstats_sweeps.py:31 (assert_rowstats): scoring_referee.same_bits on every field"""
    for name in ("mean", "std", "n_nan"):
        bad = np.flatnonzero(~SC.same_bits(got[name], want[name]))
        assert bad.size == 0, (label, name, bad[:6].tolist())


for _dtype in (np.float32, np.float64):
    _case(f"rowstats {np.dtype(_dtype).name}", functools.partial(_rowstats_inputs, _dtype), _run_rowstats,
          lambda x: dict(zip(("mean", "std", "n_nan"), SC.rowstats_rows(x["data"], x["idx"]))), _check_rowstats,
          ("mean", "std", "n_nan"), arena=False)


def _run_quantize3(ctx, x):
    d = ctx.to_device(x["ps"])
    ctx.quantize3_dev(d)
    return _collect(dict(ps=d))


# (bit for bit: test_gpu_large_paths.py:346)
_case("quantize3", lambda: dict(ps=LP.quantize_values(5000)), _run_quantize3, lambda x: dict(ps=O.quantize3_fast(x["ps"])),
      lambda got, want, label: _same(got, want, label, ("ps",)), ("ps",), arena=False)
