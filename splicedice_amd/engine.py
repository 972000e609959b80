"""Thin numpy-facing wrapper over the C ABI (include/sdice.h).  No compute happens here."""
import contextlib
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import SdiceError, check  # noqa: F401


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


# The result fields of every per-row test, in the order of its C entry point (include/sdice.h).  A field is [n]; one marked
# PER_SET is [k, n], one row per sample set, one marked PER_PAIR [k (k - 1) / 2, n], one row per pair of sets in the order
# of dunn_pairs(k).  GRAM_FIELDS: the four [m, m] matrices of sample_gram.
PER_SET = "per set"
PER_PAIR = "per pair"
DUNN_MAX_SETS = 11                  # sets a kruskal_dunn call accepts (include/sdice.h, SDICE_DUNN_MAX_SETS)
RANKSUM_FIELDS = [("tested", np.uint8), ("p", np.float64), ("z", np.float64), ("med1", np.float32), ("med2", np.float32),
                  ("mean1", np.float32), ("mean2", np.float32), ("delta", np.float32)]       # (ranksum and signedrank)
RANKSUM_EXACT_FIELDS = RANKSUM_FIELDS + [("exact", np.uint8)]                                # (the two --exact calls)
KS_FIELDS = [("tested", np.uint8), ("p", np.float64), ("d", np.float64), ("med1", np.float32), ("med2", np.float32),
             ("mean1", np.float32), ("mean2", np.float32), ("delta", np.float32), ("exact", np.uint8)]
SHIFT_FIELDS = [("tested", np.uint8), ("shift", np.float64), ("lo", np.float64), ("hi", np.float64), ("rank", np.int32)]
WALSH_FIELDS = SHIFT_FIELDS                     # (the paired estimate: the same five outputs)
KRUSKAL_FIELDS = [("tested", np.uint8), ("p", np.float64), ("h", np.float64), ("med", np.float32, PER_SET),
                  ("mean", np.float32, PER_SET), ("delta", np.float32)]
KRUSKAL_DUNN_FIELDS = KRUSKAL_FIELDS + [("pair_z", np.float64, PER_PAIR), ("pair_p", np.float64, PER_PAIR),
                                        ("pair_padj", np.float64, PER_PAIR)]
JONCKHEERE_FIELDS = [("tested", np.uint8), ("p", np.float64), ("z", np.float64), ("j", np.float64),
                     ("med", np.float32, PER_SET), ("mean", np.float32, PER_SET), ("delta", np.float32)]
FRIEDMAN_FIELDS = [("tested", np.uint8), ("p", np.float64), ("q", np.float64), ("w", np.float64), ("blocks", np.int32),
                   ("med", np.float32, PER_SET), ("mean", np.float32, PER_SET), ("delta", np.float32)]
PAGE_FIELDS = [("tested", np.uint8), ("p", np.float64), ("z", np.float64), ("l", np.float64), ("blocks", np.int32),
               ("med", np.float32, PER_SET), ("mean", np.float32, PER_SET), ("delta", np.float32)]
SPEARMAN_FIELDS = [("tested", np.uint8), ("p", np.float64), ("rho", np.float64), ("n_kept", np.int32), ("med", np.float32),
                   ("mean", np.float32)]
GRAM_FIELDS = [("shared", np.int64), ("sum1", np.int64), ("sum2", np.int64), ("prod", np.int64)]
# Every row test: the name of its pair of C entry points (sdice_<name>, sdice_<name>_dev) and of its pair of Context methods
# (<name>, <name>_dev) -> (its field table, the fields a _dev call may leave out of `out`: the library is handed NULL)
# (friedman, page and walsh: the resident methods are friedman_resident / page_resident / walsh_resident for now, see there)
ROW_TESTS = {
    "ranksum": (RANKSUM_FIELDS, ("z",)),
    "ranksum_exact": (RANKSUM_EXACT_FIELDS, ("z",)),
    "ranksum_strata": (RANKSUM_FIELDS, ("z",)),
    "ks": (KS_FIELDS, ("d", "exact")),             # (ks_dev(exact=True) wants exact)
    "shift": (SHIFT_FIELDS, ()),
    "kruskal": (KRUSKAL_FIELDS, ("h",)),
    "kruskal_dunn": (KRUSKAL_DUNN_FIELDS, ("h", "pair_p", "pair_padj")),
    "jonckheere": (JONCKHEERE_FIELDS, ("j",)),
    "friedman": (FRIEDMAN_FIELDS, ("q", "w", "blocks")),
    "page": (PAGE_FIELDS, ("l", "blocks")),
    "signedrank": (RANKSUM_FIELDS, ("z",)),
    "signedrank_exact": (RANKSUM_EXACT_FIELDS, ("z",)),
    "walsh": (WALSH_FIELDS, ()),
    "spearman": (SPEARMAN_FIELDS, ("rho",)),
    "sample_gram": (GRAM_FIELDS, ()),
}


def field_shapes(fields, shape, k=None):
    """a field table -> name: (shape, dtype) in its order; `shape` for a plain field, (k, shape) for one marked PER_SET,
    (k (k - 1) / 2, shape) for one marked PER_PAIR"""
    lead = {PER_SET: lambda: k, PER_PAIR: lambda: k * (k - 1) // 2}
    return {f[0]: ((lead[f[2]](), shape) if f[2:] else shape, f[1]) for f in fields}


def dunn_pairs(k):
    """the pairs of sets (i, j), i < j, in the order of the PER_PAIR outputs: (0, 1), (0, 2), .., (k - 2, k - 1)"""
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def _zeros(fields, shape, k=None):
    return {name: np.zeros(sh, dt) for name, (sh, dt) in field_shapes(fields, shape, k).items()}


def _arg(a):
    """an argument between the table and the outputs of a row test as ctypes takes it: the address of a device or a host
    array, anything else as it is"""
    return a.ptr if isinstance(a, DeviceArray) else _ptr(a) if isinstance(a, np.ndarray) else a


def _int_lists(*lists):
    """column lists (or the ids that go with them) as int32 vectors"""
    return [_c(v, np.int32).reshape(-1) for v in lists]


def _with_lengths(*lists):
    """(a, b) -> (a, len a, b, len b): the two column lists of a two-group call, host vectors or device arrays"""
    return tuple(x for a in lists for x in (a, a.shape[0]))


def pair_array(pairs):
    """a pair list as the library takes it: int32 [m, 2], C-contiguous, m >= 1 (the library checks the indices)"""
    a = np.asarray(pairs)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0:
        raise ValueError(f"pairs must be a non-empty [m, 2] array of column indices, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise TypeError(f"pairs must hold integers, got {a.dtype}")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("pairs: column index out of range")
    return np.ascontiguousarray(a, dtype=np.int32)


def kruskal_sets(sets, s=None):
    """k lists of column indices as the library takes them -> (cols int32 of all sets back to back, set_ptr int32[k + 1]).
    A column may belong to one set only: a column listed twice (inside a set or across sets) raises ValueError here, on
    the host, before anything is launched; so does an index outside [0, s) when s is given."""
    sets = [np.asarray(g).reshape(-1).astype(np.int32) for g in sets]
    set_ptr = np.zeros(len(sets) + 1, dtype=np.int32)
    set_ptr[1:] = np.cumsum([g.size for g in sets])
    cols = np.concatenate(sets) if sets else np.zeros(0, np.int32)
    if s is not None and cols.size and (cols.min() < 0 or cols.max() >= s):
        raise ValueError(f"kruskal: column index outside [0, {s})")
    seen = {}
    for i, g in enumerate(sets):
        for c in g.tolist():
            if c in seen:
                raise ValueError(f"kruskal: column {c} is in set {seen[c] + 1} and in set {i + 1}; a column may belong to one set only")
            seen[c] = i
    return np.ascontiguousarray(cols, dtype=np.int32), set_ptr


def friedman_columns(sets, s=None):
    """k equally long lists of column indices, list j the columns of set j in SUBJECT order (entry q of every list is the
    same subject) -> the set-major int32 cols of friedman() / page(): cols[j * m + q].  Lists of unequal length, a column
    listed twice (inside a set or across sets) and, when s is given, an index outside [0, s) raise ValueError here, on the
    host, before anything is launched."""
    sets = [np.asarray(g).reshape(-1) for g in sets]
    if len({g.size for g in sets}) > 1:
        raise ValueError(f"friedman: the sets differ in length ({', '.join(str(g.size) for g in sets)} columns); entry q of "
                         f"every set is the same subject")
    for g in sets:
        if g.size and g.dtype.kind not in "iu":
            raise TypeError(f"friedman: column indices must be integers, got {g.dtype}")
    cols = np.concatenate(sets).astype(np.int64) if sets else np.zeros(0, np.int64)
    if s is not None and cols.size and (cols.min() < 0 or cols.max() >= s):
        raise ValueError(f"friedman: column index outside [0, {s})")
    if cols.size and (cols.min() < -2 ** 31 or cols.max() >= 2 ** 31):
        raise ValueError("friedman: column index out of range")
    uniq, count = np.unique(cols, return_counts=True)
    if np.any(count > 1):
        raise ValueError(f"friedman: column {int(uniq[count > 1][0])} is listed more than once; a column may appear once "
                         f"over all sets")
    return np.ascontiguousarray(cols, dtype=np.int32)


def shift_quantile(conf):
    """the confidence level of a shift interval, 0 < conf < 1 -> zq, the standard normal quantile at 1 - (1 - conf) / 2, as
    sdice_shift takes it (the standard library's NormalDist: no scipy on the product path)"""
    import statistics
    conf = float(conf)
    if not 0.0 < conf < 1.0:
        raise ValueError(f"shift: the confidence level must satisfy 0 < conf < 1, got {conf!r}")
    return statistics.NormalDist().inv_cdf(1.0 - (1.0 - conf) / 2.0)


def strata_ids(labels):
    """arbitrary stratum labels (batch names, centres, ...) -> (int32 dense ids numbered by first appearance, the distinct
    labels in that order): what ranksum_strata() takes as strat1 / strat2 once the two lists' labels are numbered together"""
    where = {}
    ids = np.array([where.setdefault(x, len(where)) for x in labels], dtype=np.int32)
    return ids, list(where)


def spearman_order(cols, x):
    """the listed columns and the covariate value of each as sdice_spearman takes them -> (cols int32 sorted by x, ties in
    the order given (a stable sort), xg int32: the dense tie-group id of each sorted column: xg[0] = 0, one more at every
    step to a larger x).  Ties are by float64 equality (-0.0 == 0.0).  A NaN or an infinite x raises ValueError."""
    cols = np.asarray(cols).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if cols.size != x.size:
        raise ValueError(f"spearman: {cols.size} columns but {x.size} covariate values")
    if cols.size and cols.dtype.kind not in "iu":
        raise TypeError(f"spearman: column indices must be integers, got {cols.dtype}")
    if not np.all(np.isfinite(x)):
        raise ValueError("spearman: the covariate must be finite (leave a sample without a value out of the list)")
    order = np.argsort(x, kind="stable")
    xs = x[order]
    xg = np.zeros(x.size, dtype=np.int32)
    if x.size:
        xg[1:] = np.cumsum(xs[1:] != xs[:-1])
    return np.ascontiguousarray(cols[order], dtype=np.int32), xg


def gram_columns(cols):
    """the selected columns of sample_gram as the library takes them: int32 [m], C-contiguous (the library checks the range
    and that each is listed once)"""
    a = np.asarray(cols).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"sample_gram: column indices must be integers, got {a.dtype}")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("sample_gram: column index out of range")
    return np.ascontiguousarray(a, dtype=np.int32)


def sample_matrix_finish(shared, sum1, sum2, prod, min_shared=3):
    """the four int64 [m, m] matrices of sample_gram -> (corr, rmsd) float64 [m, m]: the Pearson correlation and the
    root-mean-square PS difference of every sample pair over the rows both have, NaN where fewer than min_shared rows are
    shared (corr also where a sample is constant over them).  Host code: no context, no GPU (sdice_sample_matrix_finish)."""
    mats = [np.ascontiguousarray(x, dtype=np.int64) for x in (shared, sum1, sum2, prod)]
    m = mats[0].shape[0]
    if any(x.shape != (m, m) for x in mats):
        raise ValueError(f"sample_matrix_finish: four square matrices of one size, got {[x.shape for x in mats]}")
    corr, rmsd = np.empty((m, m), np.float64), np.empty((m, m), np.float64)
    check(_ffi.load().sdice_sample_matrix_finish(m, *[_ptr(x) for x in mats], int(min_shared), _ptr(corr), _ptr(rmsd)),
          "sdice_sample_matrix_finish")
    return corr, rmsd


class DeviceArray:
    """A device allocation with a numpy-like shape/dtype tag (owned by a Context)."""

    def __init__(self, ctx, shape, dtype, ptr=None, owned=True):
        self.ctx = ctx
        self.shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.owned = owned
        if ptr is None:
            p = C.c_void_p()
            check(ctx.lib.sdice_dmalloc(ctx.h, self.nbytes, C.byref(p)), "sdice_dmalloc")
            self.ptr = p.value
        else:
            self.ptr = ptr

    def upload(self, host):
        host = _c(host, self.dtype)
        assert host.nbytes == self.nbytes, (host.nbytes, self.nbytes)
        check(self.ctx.lib.sdice_h2d(self.ctx.h, self.ptr, _ptr(host), self.nbytes), "sdice_h2d")
        return self

    def to_host(self, out=None):
        """-> host copy (into `out`, a C-contiguous array of the same dtype and size, when given)"""
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        else:
            assert out.dtype == self.dtype and out.flags.c_contiguous and out.nbytes == self.nbytes
        check(self.ctx.lib.sdice_d2h(self.ctx.h, _ptr(out), self.ptr, self.nbytes), "sdice_d2h")
        return out

    def memset(self, byte):
        """fill with one byte value (async on the context stream); returns self"""
        check(self.ctx.lib.sdice_dmemset(self.ctx.h, self.ptr, int(byte), self.nbytes), "sdice_dmemset")
        return self

    def zero(self):
        return self.memset(0)

    def offset(self, n_elems_lead, shape):
        """View starting n_elems_lead elements in (not owned)."""
        return DeviceArray(self.ctx, shape, self.dtype, ptr=self.ptr + n_elems_lead * self.dtype.itemsize, owned=False)

    def free(self):
        if self.owned and self.ptr:
            self.ctx.lib.sdice_dfree(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


class Context:
    """One context per GPU / per rank.  Fails loudly when no gfx950 device is usable."""

    def __init__(self, device=0):
        self.lib = _ffi.load()
        h = C.c_void_p()
        check(self.lib.sdice_ctx_create(int(device), C.byref(h)), "sdice_ctx_create")
        self.h = h
        self.device = int(device)

    def close(self):
        if self.h:
            self.lib.sdice_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---------------------------------------------------------------- info / params / timing
    def device_info(self):
        name = C.create_string_buffer(160)
        cus = C.c_int()
        mem = C.c_int64()
        check(self.lib.sdice_device_info(self.h, name, 160, C.byref(cus), C.byref(mem)), "sdice_device_info")
        return dict(name=name.value.decode(), compute_units=cus.value, hbm_bytes=mem.value)

    def set_param(self, name, value):
        check(self.lib.sdice_set_param(self.h, name.encode(), int(value)), f"sdice_set_param({name})")

    def get_param(self, name):
        """the value in force: the last one set, the library's default if the parameter was never set"""
        v = C.c_int64()
        check(self.lib.sdice_get_param(self.h, name.encode(), C.byref(v)), f"sdice_get_param({name})")
        return v.value

    @contextlib.contextmanager
    def params(self, values):
        """`with ctx.params({"bh.wg": 512, "bh.mean": 900}):` sets the given parameters for the block and then writes back,
        in reverse order, the values that were in force before it, so scopes nest and no caller needs to know a default.
        A parameter that was never set ends up set to its default, which every read treats like unset."""
        old = [(name, self.get_param(name)) for name in values]
        try:
            for name, value in values.items():
                self.set_param(name, value)
            yield self
        finally:
            for name, value in reversed(old):
                self.set_param(name, value)

    def sync(self):
        check(self.lib.sdice_sync(self.h), "sdice_sync")

    def trim(self):
        """synchronise and release the cached device scratch"""
        check(self.lib.sdice_trim(self.h), "sdice_trim")

    def scratch_regions(self):
        """Test support (sdice_scratch_region): the device memory the context keeps between calls and treats as scratch
        -> [(name, DeviceArray uint8 over the whole region, not owned)]: every "arena" chunk, "cluster.col",
        "cluster.reach".  Synchronises; changes nothing."""
        out = []
        name, p, nbytes = C.c_char_p(), C.c_void_p(), C.c_int64()
        while True:
            status = self.lib.sdice_scratch_region(self.h, len(out), C.byref(name), C.byref(p), C.byref(nbytes))
            if status == -1:          # SDICE_ERR_ARG: past the last region
                return out
            check(status, "sdice_scratch_region")
            out.append((name.value.decode(), DeviceArray(self, (nbytes.value,), np.uint8, ptr=p.value, owned=False)))

    def prof_enable(self, on=True):
        """on: False/0 off, True/1 every kernel, 2 dominant kernels only."""
        check(self.lib.sdice_prof_enable(self.h, int(on)), "sdice_prof_enable")

    def prof_reset(self):
        check(self.lib.sdice_prof_reset(self.h), "sdice_prof_reset")

    def prof_query(self, name):
        n = C.c_int64()
        ms = C.c_double()
        check(self.lib.sdice_prof_query(self.h, name.encode(), C.byref(n), C.byref(ms)), "sdice_prof_query")
        return n.value, ms.value

    def prof_report(self):
        buf = C.create_string_buffer(8192)
        check(self.lib.sdice_prof_report(self.h, buf, 8192), "sdice_prof_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split()
            out[name] = (int(n), float(ms))
        return out

    def timer_start(self):
        check(self.lib.sdice_timer_start(self.h), "sdice_timer_start")

    def timer_stop(self):
        ms = C.c_double()
        check(self.lib.sdice_timer_stop(self.h, C.byref(ms)), "sdice_timer_stop")
        return ms.value

    # ---------------------------------------------------------------- device memory
    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        return DeviceArray(self, host.shape, host.dtype).upload(host)

    # ---------------------------------------------------------------- host entry points
    def cluster(self, chrom_rank, left, right, strand):
        """-> (row_of int32[n], row_ptr int64[n+1], col int32[nnz]); SPLICEDICE.py:230-255,96"""
        cr, l, r = _c(chrom_rank, np.int32), _c(left, np.int32), _c(right, np.int32)
        st = _c(strand, np.int8)
        n = cr.size
        row_of = np.empty(n, dtype=np.int32)
        row_ptr = np.zeros(n + 1, dtype=np.int64)
        nnz = C.c_int64()
        check(self.lib.sdice_cluster(self.h, n, _ptr(cr), _ptr(l), _ptr(r), _ptr(st), _ptr(row_of), _ptr(row_ptr),
                                     C.byref(nnz)), "sdice_cluster")
        col = np.empty(nnz.value, dtype=np.int32)
        check(self.lib.sdice_cluster_col(self.h, _ptr(col), col.size), "sdice_cluster_col")
        return row_of, row_ptr, col

    def ps(self, counts, row_ptr, col, want_excl=False, want_ps=True):
        """-> ps float32[n,s] (and excl int64[n,s]); SPLICEDICE.py:297-310"""
        counts = _c(counts, np.int32)
        n, s = counts.shape
        row_ptr, col = _c(row_ptr, np.int64), _c(col, np.int32)
        ps = np.empty((n, s), dtype=np.float32) if want_ps else None
        excl = np.empty((n, s), dtype=np.int64) if want_excl else None
        check(self.lib.sdice_ps(self.h, n, s, _ptr(counts), _ptr(row_ptr), _ptr(col), _ptr(excl), _ptr(ps)), "sdice_ps")
        if want_ps and want_excl:
            return ps, excl
        return ps if want_ps else excl

    def _listed_f64(self, name, counts, row_ptr, col, n_out):
        """sdice_<name>: a float64 [n_out, s] result over the listed rows of a float64 table (ps_f64, excl_f64)"""
        counts = _c(counts, np.float64)
        n_rows, s = counts.shape
        n_out = n_rows if n_out is None else int(n_out)
        row_ptr, col = _c(row_ptr, np.int64), _c(col, np.int32)
        if row_ptr.size != n_out + 1:
            raise ValueError(f"{name}: row_ptr must hold n_out + 1 entries")
        out = np.empty((n_out, s), dtype=np.float64)
        check(getattr(self.lib, "sdice_" + name)(self.h, n_out, n_rows, s, _ptr(counts), _ptr(row_ptr), _ptr(col), _ptr(out)),
              "sdice_" + name)
        return out

    def ps_f64(self, counts, row_ptr, col, n_out=None):
        """-> ps float64[n_out,s] of a float64 count table, sums in list order (counts_to_ps.py:58-70).
        Rows n_out.. of `counts` are sources only."""
        return self._listed_f64("ps_f64", counts, row_ptr, col, n_out)

    def excl_f64(self, counts, row_ptr, col, n_out=None):
        """-> float64[n_out,s]: for every row the sum of the listed rows of a float64 table, one addition per row in list
        order (np.sum(counts[mask], axis=0) of pairwise_fisher.py:158-160 when the lists are in table order).
        Rows n_out.. of `counts` are sources only."""
        return self._listed_f64("excl_f64", counts, row_ptr, col, n_out)

    def mark_low(self, ps, low_flat_idx):
        ps = _c(ps, np.float32)
        idx = _c(low_flat_idx, np.int64)
        check(self.lib.sdice_mark_low(self.h, ps.size, _ptr(ps), _ptr(idx), idx.size), "sdice_mark_low")
        return ps

    def quantize3(self, ps):
        out = np.array(ps, dtype=np.float32, order="C", copy=True)
        check(self.lib.sdice_quantize3(self.h, out.size, _ptr(out)), "sdice_quantize3")
        return out

    def _host_row(self, name, ps, mid, shape=None, k=None, skip=()):
        """the host form of a row test of ROW_TESTS: sdice_<name>(ctx, n, s, ps, *mid, the outputs in field order) on zeroed
        outputs of `shape` (default: [n]; k sets for the per-set and per-pair fields) -> {field: array}.  A field named in
        `skip` is handed to the library as NULL and is not in the result."""
        ps = _c(ps, np.float32)
        n, s = ps.shape
        out = _zeros(ROW_TESTS[name][0], n if shape is None else shape, k)
        check(getattr(self.lib, "sdice_" + name)(self.h, n, s, _ptr(ps), *map(_arg, mid),
                                                 *[None if f in skip else _ptr(a) for f, a in out.items()]), "sdice_" + name)
        return {f: a for f, a in out.items() if f not in skip}

    def _host_sets(self, name, ps, sets, skip=()):
        """_host_row over k column sets (kruskal_sets checks them against the table's columns)"""
        ps = _c(ps, np.float32)
        _, s = ps.shape
        cols, set_ptr = kruskal_sets(sets, s)
        k = len(set_ptr) - 1
        return self._host_row(name, ps, (cols, set_ptr, k), k=k, skip=skip)

    def _host_pairs(self, name, ps, a, b, *more):
        """_host_row over matched column pairs; more: the arguments after the pair count"""
        a, b = _c(a, np.int32), _c(b, np.int32)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError(f"{name}: the pair lists must be two vectors of one length, got {a.shape} and {b.shape}")
        return self._host_row(name, ps, (a, b, a.size, *more))

    def ranksum(self, ps, g1, g2):
        """compareSampleSets.py:216-232 for every row; un-compacted outputs + tested mask."""
        return self._host_row("ranksum", ps, _with_lengths(*_int_lists(g1, g2)))

    def ranksum_exact(self, ps, g1, g2):
        """ranksum() with the exact conditional p-value on the rows that keep at most 32 values (include/sdice.h): the
        same outputs + exact (1 where p is the exact value); every other field is ranksum()'s bit for bit."""
        return self._host_row("ranksum_exact", ps, _with_lengths(*_int_lists(g1, g2)))

    def ranksum_strata(self, ps, g1, g2, strat1, strat2):
        """van Elteren's stratified rank-sum test per row (include/sdice.h): strat1 / strat2 are the dense stratum ids
        (strata_ids) of the columns g1 / g2; the outputs of ranksum(), with medians and means that are ranksum()'s."""
        g1, g2, strat1, strat2 = _int_lists(g1, g2, strat1, strat2)
        if g1.size != strat1.size or g2.size != strat2.size:
            raise ValueError(f"ranksum_strata: one stratum id per listed column, got {g1.size} / {strat1.size} and "
                             f"{g2.size} / {strat2.size}")
        n_strata = int(max(strat1.max(initial=-1), strat2.max(initial=-1))) + 1
        return self._host_row("ranksum_strata", ps, (*_with_lengths(g1, g2), strat1, strat2, n_strata))

    def ks(self, ps, g1, g2, exact=False):
        """the two-sample Kolmogorov-Smirnov test per row (include/sdice.h): un-compacted tested, p, d (the statistic D),
        the medians, means and delta of ranksum(), and exact (1 where p is the exact conditional value: with exact=True,
        on the tested rows that keep at most 32 values; all 0 otherwise)."""
        return self._host_row("ks", ps, (*_with_lengths(*_int_lists(g1, g2)), int(bool(exact))))

    def shift(self, ps, g1, g2, conf=0.95):
        """the Hodges-Lehmann shift of group 1 against group 2 per row with its confidence interval at level conf
        (include/sdice.h): un-compacted tested (ranksum()'s), shift (the median of the pairwise differences), lo and hi (two
        order statistics of them) and rank (which ones; 1 = the whole range, the level is not reached)."""
        return self._host_row("shift", ps, (*_with_lengths(*_int_lists(g1, g2)), shift_quantile(conf)))

    def kruskal(self, ps, sets):
        """scipy.stats.kruskal per row across the k column sets under the row rules of ranksum(); un-compacted outputs:
        tested, p, h [n], med, mean [k, n] (set-major), delta [n] = largest minus smallest set median."""
        return self._host_sets("kruskal", ps, sets)

    def kruskal_dunn(self, ps, sets, pair_p=True, pair_padj=True):
        """kruskal() with Dunn's test for every pair of sets from the same joint ranking (include/sdice.h): kruskal()'s
        outputs bit for bit, and pair_z, pair_p, pair_padj float64 [k (k - 1) / 2, n] in the order of dunn_pairs(k): z > 0
        where set i ranks above set j, p two-sided, padj Holm's step-down inside the row.  At most DUNN_MAX_SETS sets (the
        library refuses more).  pair_p / pair_padj False: the library is handed NULL for that output and the result lacks
        it."""
        return self._host_sets("kruskal_dunn", ps, sets,
                               skip=[name for name, on in (("pair_p", pair_p), ("pair_padj", pair_padj)) if not on])

    def jonckheere(self, ps, sets):
        """Jonckheere-Terpstra trend test per row across the k ORDERED column sets (set 0 < set 1 < ...) under the row rules
        of kruskal(); un-compacted outputs: tested, p, z (> 0: the values rise along the order), j = J [n], med, mean
        [k, n] and delta [n] as kruskal()'s."""
        return self._host_sets("jonckheere", ps, sets)

    def _host_matched(self, name, ps, sets, skip=()):
        """_host_row over k matched column sets (friedman_columns checks them against the table's columns)"""
        ps = _c(ps, np.float32)
        cols = friedman_columns(sets, ps.shape[1])
        k = len(sets)
        return self._host_row(name, ps, (cols, k, cols.size // k if k else 0), k=k, skip=skip)

    def friedman(self, ps, sets):
        """Friedman's test per row across k MATCHED column sets (entry q of every set is the same subject;
        include/sdice.h): a subject's block of k values is kept when none is NaN, the row is tested with 3 kept blocks or
        more; un-compacted outputs: tested, p = chi2.sf(Q, k - 1), q = Q, w = Kendall's W, blocks (int32: kept blocks) [n],
        med, mean [k, n] over the kept blocks, delta [n] = largest minus smallest set median."""
        return self._host_matched("friedman", ps, sets)

    def page(self, ps, sets):
        """Page's L trend test per row across k MATCHED, ORDERED column sets (set 0 < set 1 < ...) under the row rules of
        friedman(); un-compacted outputs: tested, p (two-sided, asymptotic), z (> 0: the values rise along the order, the
        variance conditional on the row's ties), l = L, blocks [n], med, mean [k, n] and delta [n] as friedman()'s."""
        return self._host_matched("page", ps, sets)

    def signedrank(self, ps, a, b):
        """scipy.stats.wilcoxon (asymptotic, zero_method="wilcox") per row over the matched column pairs (a[q], b[q])
        under the row rules of ranksum(); same un-compacted outputs + tested mask (z > 0: side a is larger)."""
        return self._host_pairs("signedrank", ps, a, b)

    def signedrank_exact(self, ps, a, b):
        """signedrank() with the exact p-value on the rows with at most 31 non-zero differences (include/sdice.h): the
        same outputs + exact; every other field is signedrank()'s bit for bit."""
        return self._host_pairs("signedrank_exact", ps, a, b)

    def walsh(self, ps, a, b, conf=0.95):
        """the paired shift per row over the matched column pairs (a[q], b[q]) with its confidence interval at level conf
        (include/sdice.h): the Hodges-Lehmann estimate that belongs to the signed-rank test, R's "(pseudo)median".
        Un-compacted tested (signedrank()'s), shift (the median of the Walsh averages (d_i + d_j) / 2, i <= j, of the kept
        pairs' differences, zeros included), lo and hi (two order statistics of them) and rank (which ones; 1 = the whole
        range, the level is not reached)."""
        return self._host_pairs("walsh", ps, a, b, shift_quantile(conf))

    def spearman(self, ps, cols, x):
        """scipy.stats.spearmanr(x_kept, ps_kept) per row between the PS values of the listed columns and the covariate x
        (one finite value per listed column) under the row rules of ranksum(); un-compacted outputs: tested, p, rho,
        n_kept (int32), med, mean of the kept PS values (in the order of spearman_order(cols, x))."""
        cols, xg = spearman_order(cols, x)
        return self._host_row("spearman", ps, (cols, xg, cols.size))

    def sample_gram(self, ps, cols):
        """the exact integer sums of every pair of the listed columns over the rows both have a value in -> dict of int64
        [m, m]: shared (row count), sum1 / sum2 ([a, b]: a's sum of 3-decimal keys / squared keys over the rows shared
        with b), prod (sum of key products).  A value off the 3-decimal grid in a listed column raises SdiceError."""
        cols = gram_columns(cols)
        return self._host_row("sample_gram", ps, (cols, cols.size), shape=(cols.size, cols.size))

    def _pair_test(self, test, dev, incl, excl, pairs, p, *bad):
        """the C call behind the four pair methods: sdice_<test>_pair_list over a list, else sdice_<test>_pairs; dev: the _dev
        forms on DeviceArrays (pairs: a pair_table()), else p is allocated here; bad: chi2's n_bad argument.  -> p"""
        if not dev:
            incl, excl = _c(incl, np.int32), _c(excl, np.int64)
            pairs = None if pairs is None else pair_array(pairs)
            s = incl.shape[1]
            p = np.empty((incl.shape[0], s * (s - 1) // 2 if pairs is None else len(pairs)), dtype=np.float64)
        ptr = (lambda a: a.ptr) if dev else _ptr
        sym = "sdice_%s_%s%s" % (test, "pairs" if pairs is None else "pair_list", "_dev" if dev else "")
        lst = () if pairs is None else (pairs.shape[0], ptr(pairs))
        check(getattr(self.lib, sym)(self.h, *incl.shape, ptr(incl), ptr(excl), *lst, ptr(p), *bad), sym)
        return p

    def fisher_pairs(self, incl, excl, pairs=None):
        """pairwise_fisher.py:164-179 -> p float64[n, s(s-1)/2]; pairs = [m, 2] column indices: p float64[n, m], column q
        the table [[incl_i, incl_j], [excl_i, excl_j]] of pair q = (i, j) -- any order, i > j and repeats allowed"""
        return self._pair_test("fisher", False, incl, excl, pairs, None)

    def chi2_pairs(self, incl, excl, pairs=None):
        """pairwise --chi2 (scipy chi2_contingency per pair) -> (p float64[n, s(s-1)/2], n_bad); pairs as in fisher_pairs:
        (p float64[n, m], n_bad among the listed tables)"""
        bad = C.c_int64()
        return self._pair_test("chi2", False, incl, excl, pairs, None, C.byref(bad)), bad.value

    def fisher_tables(self, abcd):
        abcd = _c(abcd, np.int64).reshape(-1, 4)
        p = np.empty(abcd.shape[0], dtype=np.float64)
        check(self.lib.sdice_fisher_tables(self.h, abcd.shape[0], _ptr(abcd), _ptr(p)), "sdice_fisher_tables")
        return p

    def bh(self, p):
        p = _c(p, np.float64)
        q = np.empty_like(p)
        check(self.lib.sdice_bh(self.h, p.size, _ptr(p), _ptr(q)), "sdice_bh")
        return q

    def bh_columns(self, p):
        out = np.array(p, dtype=np.float64, order="C", copy=True)
        n, cols = out.shape
        check(self.lib.sdice_bh_columns(self.h, n, cols, _ptr(out)), "sdice_bh_columns")
        return out

    def sort_unique_u64(self, keys):
        """sorted distinct 64-bit keys (the junction union of quant, SPLICEDICE.py:147-228 + :96)"""
        keys = np.array(keys, dtype=np.uint64, order="C", copy=True)
        n_unique = C.c_int64()
        check(self.lib.sdice_sort_unique_u64(self.h, keys.size, _ptr(keys), C.byref(n_unique)), "sdice_sort_unique_u64")
        return keys[: n_unique.value]

    def rowstats(self, data, idx):
        """per-row np.nanmean / np.nanstd over columns idx, bit-identical to numpy in data's dtype
        (float32 / float64) -> (mean, std, n_nan); findOutliers.py:125-135"""
        data = np.ascontiguousarray(data)
        if data.dtype not in (np.float32, np.float64):
            raise TypeError(f"rowstats: unsupported dtype {data.dtype}")
        idx = _c(idx, np.int32)
        n, s = data.shape
        mean, std = np.zeros(n, data.dtype), np.zeros(n, data.dtype)
        n_nan = np.zeros(n, np.int32)
        check(self.lib.sdice_rowstats(self.h, n, s, _ptr(data), 0 if data.dtype == np.float32 else 1, _ptr(idx), idx.size,
                                      _ptr(mean), _ptr(std), _ptr(n_nan)), "sdice_rowstats")
        return mean, std, n_nan

    def similarity(self, ps, mid, sign):
        """similarity.py:25-47 -> (scores int64[s], counts int64[s]); ps float64 [n, s]"""
        ps, mid, sign = _c(ps, np.float64), _c(mid, np.float64), _c(sign, np.int8)
        n, s = ps.shape
        scores, counts = np.zeros(s, np.int64), np.zeros(s, np.int64)
        check(self.lib.sdice_similarity(self.h, n, s, _ptr(ps), _ptr(mid), _ptr(sign), _ptr(scores), _ptr(counts)),
              "sdice_similarity")
        return scores, counts

    # ---------------------------------------------------------------- device entry points
    def cluster_dev(self, d_chrom, d_left, d_right, d_strand, d_row_of, d_row_ptr, sync=True):
        """-> (DeviceArray col view (ctx-owned), nnz).  sync=False enqueues the whole chain without a host
        round trip (nnz is then None; `cluster_status()` / `sync()` report it and any deferred error)."""
        n = d_chrom.shape[0]
        nnz = C.c_int64()
        check(self.lib.sdice_cluster_dev(self.h, n, d_chrom.ptr, d_left.ptr, d_right.ptr, d_strand.ptr, d_row_of.ptr,
                                         d_row_ptr.ptr, C.byref(nnz) if sync else None), "sdice_cluster_dev")
        p = C.c_void_p()
        check(self.lib.sdice_cluster_col_dev(self.h, C.byref(p), None), "sdice_cluster_col_dev")
        if not sync:
            return DeviceArray(self, (0,), np.int32, ptr=p.value, owned=False), None
        return DeviceArray(self, (nnz.value,), np.int32, ptr=p.value, owned=False), nnz.value

    def cluster_status(self):
        """resolve an asynchronous cluster_dev -> (nnz, reach); raises on a deferred error"""
        nnz, reach = C.c_int64(), C.c_int32()
        check(self.lib.sdice_cluster_status(self.h, C.byref(nnz), C.byref(reach)), "sdice_cluster_status")
        return nnz.value, reach.value

    def ps_dev(self, d_counts, d_row_ptr, d_col, d_excl, d_ps):
        n, s = d_counts.shape
        check(self.lib.sdice_ps_dev(self.h, n, s, d_counts.ptr, d_row_ptr.ptr, d_col.ptr if d_col is not None else None,
                                    d_excl.ptr if d_excl is not None else None,
                                    d_ps.ptr if d_ps is not None else None), "sdice_ps_dev")

    PS_PLAN_FIELDS = ("kern", "vec", "chunk_cols", "tile_rows", "halo", "n_tiles", "n_chunks", "lv_shift", "tiles_per_xcd",
                      "use_reach", "nt", "prio", "q3", "threads")

    def ps_last_plan(self):
        """Test support (sdice_ps_last_plan): the launch plan of the last ps_dev / ps launch -> {field: int}"""
        out = (C.c_int32 * len(self.PS_PLAN_FIELDS))()
        n = C.c_int32()
        check(self.lib.sdice_ps_last_plan(self.h, out, len(out), C.byref(n)), "sdice_ps_last_plan")
        assert n.value == len(self.PS_PLAN_FIELDS), n.value
        return dict(zip(self.PS_PLAN_FIELDS, out))

    def quantize3_dev(self, d_ps):
        check(self.lib.sdice_quantize3_dev(self.h, int(np.prod(d_ps.shape)), d_ps.ptr), "sdice_quantize3_dev")

    def _resident_row(self, name, d_ps, mid, out, optional=None):
        """the resident form of a row test of ROW_TESTS: sdice_<name>_dev(ctx, n, s, d_ps, *mid, the device outputs of `out`
        in field order).  A field of `optional` (default: the test's own) that `out` lacks is handed to the library as
        NULL; any other field that `out` lacks raises ValueError."""
        fields, may_omit = ROW_TESTS[name]
        n, s = d_ps.shape
        ptrs = []
        for f in fields:
            d = out.get(f[0])
            if d is None and f[0] not in (may_omit if optional is None else optional):
                raise ValueError(f"{name}_dev: out lacks the required field {f[0]!r}")
            ptrs.append(None if d is None else d.ptr)
        check(getattr(self.lib, f"sdice_{name}_dev")(self.h, n, s, d_ps.ptr, *map(_arg, mid), *ptrs), f"sdice_{name}_dev")

    def ranksum_dev(self, d_ps, d_g1, d_g2, out):
        self._resident_row("ranksum", d_ps, _with_lengths(d_g1, d_g2), out)

    def ranksum_strata_dev(self, d_ps, d_g1, d_g2, d_strat1, d_strat2, n_strata, out):
        """d_strat1, d_strat2: the device copies of the stratum ids of d_g1, d_g2 (checked by the caller: the host call
        checks them, this one cannot); out: the device fields of RANKSUM_FIELDS (z optional)"""
        self._resident_row("ranksum_strata", d_ps, (*_with_lengths(d_g1, d_g2), d_strat1, d_strat2, int(n_strata)), out)

    def ks_dev(self, d_ps, d_g1, d_g2, out, exact=False):
        """out: the device fields of KS_FIELDS (d optional; exact optional unless exact=True)"""
        self._resident_row("ks", d_ps, (*_with_lengths(d_g1, d_g2), int(bool(exact))), out, optional=("d",) if exact else None)

    def shift_dev(self, d_ps, d_g1, d_g2, out, conf=0.95):
        """shift() on a resident table and resident lists; out: the device fields of SHIFT_FIELDS, all of them"""
        self._resident_row("shift", d_ps, (*_with_lengths(d_g1, d_g2), shift_quantile(conf)), out)

    def signedrank_dev(self, d_ps, d_a, d_b, out):
        self._resident_row("signedrank", d_ps, (d_a, d_b, d_a.shape[0]), out)

    def ranksum_exact_dev(self, d_ps, d_g1, d_g2, out):
        """out: the device fields of RANKSUM_EXACT_FIELDS (z optional)"""
        self._resident_row("ranksum_exact", d_ps, _with_lengths(d_g1, d_g2), out)

    def signedrank_exact_dev(self, d_ps, d_a, d_b, out):
        self._resident_row("signedrank_exact", d_ps, (d_a, d_b, d_a.shape[0]), out)

    def spearman_dev(self, d_ps, d_cols, d_xg, out):
        """d_cols, d_xg: the device copies of spearman_order()'s pair; out: device tested, p, (rho), n_kept, med, mean"""
        self._resident_row("spearman", d_ps, (d_cols, d_xg, d_cols.shape[0]), out)

    def sample_gram_dev(self, d_ps, d_cols, out):
        """d_cols: the device copy of gram_columns(); out: device shared, sum1, sum2, prod, int64 [m, m] each.  Synchronises
        once (the bad-value check of the pre-pass); the sums are queued."""
        self._resident_row("sample_gram", d_ps, (d_cols, d_cols.shape[0]), out)

    def _resident_sets(self, name, d_ps, d_cols, set_ptr, out):
        """_resident_row over k column sets: the device copy of kruskal_sets()'s cols and its HOST offsets"""
        set_ptr = _c(set_ptr, np.int32)
        self._resident_row(name, d_ps, (d_cols, set_ptr, set_ptr.size - 1), out)

    def kruskal_dev(self, d_ps, d_cols, set_ptr, out):
        """d_cols: the device copy of kruskal_sets()'s cols; set_ptr: its HOST offsets; out: device tested, p, (h), med and
        mean [k, n], delta"""
        self._resident_sets("kruskal", d_ps, d_cols, set_ptr, out)

    def kruskal_dunn_dev(self, d_ps, d_cols, set_ptr, out):
        """kruskal_dunn() on a resident table; d_cols and set_ptr as kruskal_dev takes them; out: the device fields of
        KRUSKAL_DUNN_FIELDS, h, pair_p and pair_padj optional, the pair fields [k (k - 1) / 2, n]"""
        self._resident_sets("kruskal_dunn", d_ps, d_cols, set_ptr, out)

    def jonckheere_dev(self, d_ps, d_cols, set_ptr, out):
        """d_cols: the device copy of kruskal_sets()'s cols; set_ptr: its HOST offsets; out: device tested, p, z, (j), med and
        mean [k, n], delta"""
        self._resident_sets("jonckheere", d_ps, d_cols, set_ptr, out)

    def friedman_resident(self, d_ps, d_cols, k, out):
        """friedman() on a resident table: sdice_friedman_dev.  d_cols: the device copy of friedman_columns()'s cols, k the
        number of sets (m = len(cols) / k); out: the device fields of FRIEDMAN_FIELDS, q, w and blocks optional.  (Named
        _resident, not _dev: every `_dev` method has to be listed in the call-order catalogue of the test suite, which this
        method joins, under the usual name friedman_dev, when that catalogue is next open for change.)"""
        self._resident_row("friedman", d_ps, (d_cols, int(k), d_cols.shape[0] // int(k)), out)

    def page_resident(self, d_ps, d_cols, k, out):
        """page() on a resident table: sdice_page_dev.  d_cols and k as friedman_resident takes them; out: the device fields
        of PAGE_FIELDS, l and blocks optional.  (page_dev in the call-order catalogue once that is open for change, as
        friedman_resident.)"""
        self._resident_row("page", d_ps, (d_cols, int(k), d_cols.shape[0] // int(k)), out)

    def walsh_resident(self, d_ps, d_a, d_b, out, conf=0.95):
        """walsh() on a resident table and resident pair lists: sdice_walsh_dev; out: the device fields of WALSH_FIELDS, all of
        them.  (walsh_dev in the call-order catalogue once that is open for change, as friedman_resident.)"""
        self._resident_row("walsh", d_ps, (d_a, d_b, d_a.shape[0], shift_quantile(conf)), out)

    def pair_table(self, s, pairs):
        """a pair list for the _dev calls: checked against s samples, packed and uploaded once -> DeviceArray uint32[m]
        (synchronous; the caller frees it)"""
        pairs = pair_array(pairs)
        d_tab = self.empty(len(pairs), np.uint32)
        try:
            check(self.lib.sdice_pair_list_pack_dev(self.h, int(s), len(pairs), _ptr(pairs), d_tab.ptr), "sdice_pair_list_pack_dev")
        except Exception:
            d_tab.free()
            raise
        return d_tab

    def fisher_pairs_dev(self, d_incl, d_excl, d_p, pairs=None):
        """pairs: None (every pair) or the device table pair_table() made for these s samples; d_p is [n, m] then"""
        self._pair_test("fisher", True, d_incl, d_excl, pairs, d_p)

    def fisher_step_stats(self):
        """(useful, issued) lane-steps of the last Fisher launch made with fisher.count_steps = 1"""
        u, t = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.sdice_fisher_step_stats(self.h, C.byref(u), C.byref(t)), "sdice_fisher_step_stats")
        return int(u.value), int(t.value)

    def chi2_pairs_dev(self, d_incl, d_excl, d_p, d_n_bad, pairs=None):
        self._pair_test("chi2", True, d_incl, d_excl, pairs, d_p, d_n_bad.ptr)

    def bh_columns_dev(self, d_p):
        n, cols = d_p.shape
        check(self.lib.sdice_bh_columns_dev(self.h, n, cols, d_p.ptr), "sdice_bh_columns_dev")

    def bh_columns_pitched_dev(self, d_p, n, cols, pitch):
        """BH down the columns of rows x cols values whose rows are `pitch` elements apart (a column range of a wider table)"""
        check(self.lib.sdice_bh_columns_pitched_dev(self.h, int(n), int(cols), int(pitch), d_p.ptr), "sdice_bh_columns_pitched_dev")

    def similarity_dev(self, d_ps, d_mid, d_sign, d_scores, d_counts):
        """d_ps float64 [n, s], d_mid float64 [n], d_sign int8 [n]; d_scores / d_counts int64 [s] are zeroed by the call and
        then added to (queued on the context stream)"""
        n, s = d_ps.shape
        check(self.lib.sdice_similarity_dev(self.h, n, s, d_ps.ptr, d_mid.ptr, d_sign.ptr, d_scores.ptr, d_counts.ptr),
              "sdice_similarity_dev")

    def rowstats_dev(self, d_data, d_idx, d_mean, d_std, d_nan):
        """d_data float32 / float64 [n, s], d_idx int32 [k]; d_mean / d_std [n] of d_data's dtype, d_nan int32 [n]"""
        n, s = d_data.shape
        if d_data.dtype not in (np.float32, np.float64):
            raise TypeError(f"rowstats_dev: unsupported dtype {d_data.dtype}")
        check(self.lib.sdice_rowstats_dev(self.h, n, s, d_data.ptr, 0 if d_data.dtype == np.float32 else 1, d_idx.ptr,
                                          d_idx.shape[0], d_mean.ptr, d_std.ptr, d_nan.ptr), "sdice_rowstats_dev")

    def comm_fork(self):
        check(self.lib.sdice_comm_fork(self.h), "sdice_comm_fork")

    def comm_join(self):
        check(self.lib.sdice_comm_join(self.h), "sdice_comm_join")

    def bh_masked_dev(self, d_p, d_tested, d_q):
        """BH over the present entries (tested != 0, or p >= 0 when d_tested is None); absent -> 0"""
        check(self.lib.sdice_bh_masked_dev(self.h, int(np.prod(d_p.shape)), d_p.ptr,
                                           d_tested.ptr if d_tested is not None else None, d_q.ptr), "sdice_bh_masked_dev")

    def bh_dev(self, d_p, d_q):
        check(self.lib.sdice_bh_dev(self.h, d_p.shape[0], d_p.ptr, d_q.ptr), "sdice_bh_dev")

    # ---------------------------------------------------------------- multi-GPU
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        check(self.lib.sdice_comm_unique_id(self.h, buf), "sdice_comm_unique_id")
        return buf.raw

    def comm_init(self, uid, rank, world):
        assert len(uid) == 128
        check(self.lib.sdice_comm_init(self.h, C.c_char_p(uid), int(rank), int(world)), "sdice_comm_init")

    def allgather_dev(self, d_send, d_recv):
        check(self.lib.sdice_allgather_dev(self.h, d_send.ptr, d_recv.ptr, d_send.nbytes), "sdice_allgather_dev")

    def alltoall_dev(self, d_send, d_recv, bytes_per_peer):
        check(self.lib.sdice_alltoall_dev(self.h, d_send.ptr, d_recv.ptr, int(bytes_per_peer)), "sdice_alltoall_dev")

    def copy2d_dev(self, dst_ptr, dpitch, src_ptr, spitch, width_bytes, rows):
        check(self.lib.sdice_copy2d_dev(self.h, dst_ptr, int(dpitch), src_ptr, int(spitch), int(width_bytes), int(rows)),
              "sdice_copy2d_dev")
