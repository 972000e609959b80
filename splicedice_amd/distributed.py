"""Sharded quant -> compare and pairwise pipelines: one process per GPU, junction axis sharded
(splicedice_amd/shard.py).

What a rank holds: the CSR (replicated: 8 B + 4 B x degree per junction) and ONLY the count rows
[ext_lo, ext_hi) of its own shard (its rows plus the read-only halo the plan gives it) -- never the
whole [n, s] table.  With the HIP Context everything stays in HBM: the shard is uploaded once, PS is
produced, quantised and consumed in place, the per-junction statistics are all-gathered as device
buffers (RCCL, padded to equal length), Benjamini-Hochberg runs on the gathered device vectors
(sdice_bh_masked_dev), and only the final per-junction table comes back to the host.

The PS matrix itself never crosses GPUs by default: it stays resident in the HBM of the rank that
owns the rows (at config 5 it is 20 GB; each rank streams its shard to the host over its own PCIe
link).  What has to be reassembled is the per-junction table (tested, p, medians, means), 29 B per
junction, because Benjamini-Hochberg ranks the p-values of ALL tested junctions
(compareSampleSets.py:235).  `gather_ps_dev` is the all-gather of the PS shards that
BASELINE.json's north_star names; bench.py times it next to the no-gather design.

pairwise: every rank computes the Fisher p-values of its rows; the reference's default correction is
BH down every pair COLUMN over all junctions (pairwise_fisher.py:187-191), so the p-value matrix is
transposed across ranks -- blocks packed on the device (sdice_copy2d_dev), RCCL all-to-all, column
BH on complete columns, all-to-all back.  `--multiple_test_correction all` (one BH over the whole
n x pairs matrix, pairwise_fisher.py:182-186) all-gathers the raw matrix (config 4: 32 GB, 26 ms of
xGMI time) and every rank ranks it redundantly, keeping its own rows.

Communicators implement rank, world, allgather(x), alltoall(x), allsum(v) for host arrays (GlooComm: the CPU
tests of the N>1 logic; SingleComm) or device arrays (RcclComm; SingleComm); _allgather / _alltoall hand
the receive buffer to one that also has allgather_into / alltoall_into.

_RowRange is a rank's rows on the device (plan geometry, counts, CSR or coordinates, every array it
allocated); CompareShard and PairwiseShard add their buffers and step(); both *_sharded entry points start
in _shard_inputs; pad_rows / drop_padding pad to the longest shard and back.
"""
import numpy as np

from . import shard
from .engine import RANKSUM_FIELDS

STAT_NAMES, STAT_DTYPES = zip(*RANKSUM_FIELDS)      # (the packed all-gather carries the rank-sum fields, in their order)


def _is_dev(x):
    return hasattr(x, "ptr") and hasattr(x, "to_host")


def _allgather(comm, send, recv):
    """all-gather into `recv` when there is one and the communicator takes it; otherwise the communicator allocates"""
    if recv is not None and hasattr(comm, "allgather_into"):
        return comm.allgather_into(send, recv)
    return comm.allgather(send)


def _alltoall(comm, send, recv, in_place=False):
    """all-to-all into `recv` when there is one and the communicator takes it; otherwise the communicator allocates
    the result -- except `in_place` (recv is a slice of a buffer that is read as a whole later): a communicator
    without alltoall_into then leaves the blocks where they are, and they are copied across on the device."""
    if recv is not None and hasattr(comm, "alltoall_into"):
        return comm.alltoall_into(send, recv)
    if in_place:
        send.ctx.copy2d_dev(recv.ptr, send.nbytes, send.ptr, send.nbytes, send.nbytes, 1)
        return recv
    return comm.alltoall(send)


def rows_per_rank(plan):
    return [p["own_hi"] - p["own_lo"] for p in plan]


def longest(rows_of):
    """rows of the longest shard: every rank pads to it (at least 1: no collective is empty)"""
    return max(max(rows_of), 1)


def pad_rows(a, m, fill=0):
    """a's rows, then `fill` up to m rows"""
    out = np.full((m,) + a.shape[1:], fill, dtype=a.dtype)
    out[: a.shape[0]] = a
    return out


def drop_padding(a, rows_of, m):
    """rank blocks of m rows each -> the first rows_of[r] rows of every block, in rank order"""
    return np.concatenate([a[r * m: r * m + k] for r, k in enumerate(rows_of)])


class SingleComm:
    rank, world = 0, 1
    device = True          # passes device arrays through untouched

    def allgather(self, x):
        return x

    def alltoall(self, x):
        return x

    def allsum(self, value):
        return int(value)


class GlooComm:
    """Host-side collectives over an initialised torch.distributed (gloo) process group."""
    device = False

    def __init__(self):
        import torch.distributed as dist
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()

    def allgather(self, x):
        """equal-shaped x on every rank -> concatenation along axis 0 in rank order"""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(x))
        outs = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(outs, t)
        return np.concatenate([o.numpy() for o in outs], axis=0)

    def alltoall(self, x):
        """x[q] goes to rank q; returns y with y[r] = the block rank r sent here.
        (gloo has no all_to_all on CPU tensors: one all_gather of the stacked blocks, keep slice `rank`.)"""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(x))
        outs = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(outs, t)
        return np.stack([o.numpy()[self.rank] for o in outs])

    def allsum(self, value):
        """sum of one integer over the ranks (error counts: every rank must take the same decision)"""
        import torch
        t = torch.tensor([int(value)], dtype=torch.int64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return int(t[0])


class RcclComm:
    """Device collectives through the engine context (RCCL over xGMI)."""
    device = True

    def __init__(self, ctx, rank, world, bcast_bytes):
        self.ctx, self.rank, self.world = ctx, rank, world
        # every rank takes part in the broadcast whatever happens on rank 0 (an all-zero id = "rank 0 failed")
        uid, err = None, None
        if rank == 0:
            try:
                uid = ctx.comm_unique_id()
            except Exception as e:       # noqa: BLE001 -- re-raised below, after the broadcast
                uid, err = bytes(128), e
        uid = bcast_bytes(uid, 128)
        if err is not None:
            raise err
        if not any(uid):
            raise RuntimeError("RCCL unique id could not be created on rank 0")
        ctx.comm_init(uid, rank, world)

    def allgather(self, x):
        if not _is_dev(x):
            x = self.ctx.to_device(np.ascontiguousarray(x))
            return self.allgather(x).to_host()
        recv = self.ctx.empty((self.world * x.shape[0],) + tuple(x.shape[1:]), x.dtype)
        self.ctx.allgather_dev(x, recv)
        return recv

    def allgather_into(self, x, recv):
        self.ctx.allgather_dev(x, recv)
        return recv

    def alltoall_into(self, x, recv):
        self.ctx.alltoall_dev(x, recv, x.nbytes // self.world)
        return recv

    def alltoall(self, x):
        """grouped ncclSend/ncclRecv (sdice_alltoall_dev): block q -> rank q over its direct xGMI link"""
        if not _is_dev(x):
            x = self.ctx.to_device(np.ascontiguousarray(x))
            return self.alltoall(x).to_host()
        recv = self.ctx.empty(x.shape, x.dtype)
        self.ctx.alltoall_dev(x, recv, x.nbytes // self.world)
        return recv

    def allsum(self, value):
        return int(self.allgather(np.asarray([int(value)], dtype=np.int64)).sum())


def stat_layout(m):
    """The per-junction table of one rank (m rows, padded) as ONE byte block for ONE all-gather (north_star: "a single
    RCCL all-gather ... to reassemble the output tables"): name -> (byte offset, dtype); every vector starts at a
    multiple of 16 bytes.  -> (offsets, block bytes)"""
    off, at = {}, 0
    for name, dt in zip(STAT_NAMES, STAT_DTYPES):
        off[name] = (at, np.dtype(dt))
        at += (m * np.dtype(dt).itemsize + 15) // 16 * 16
    return off, at


def pack_stats_host(stats, m):
    off, nbytes = stat_layout(m)
    buf = np.zeros(nbytes, dtype=np.uint8)
    for name, (at, dt) in off.items():
        buf[at: at + m * dt.itemsize] = np.ascontiguousarray(stats[name], dtype=dt).view(np.uint8)
    return buf


def unpack_stats_host(gathered, m, world):
    """[world * block bytes] -> name -> array of world * m entries (rank blocks concatenated)"""
    off, nbytes = stat_layout(m)
    blocks = np.asarray(gathered, dtype=np.uint8).reshape(world, nbytes)
    return {name: np.concatenate([blocks[r, at: at + m * dt.itemsize].view(dt) for r in range(world)])
            for name, (at, dt) in off.items()}


def _own_slice(counts_ext, n, part):
    """the caller hands over rows [ext_lo, ext_hi); a full [n, s] table (single-process callers) is cut here"""
    elo, ehi = part["ext_lo"], part["ext_hi"]
    if counts_ext.shape[0] == ehi - elo:
        return counts_ext
    if counts_ext.shape[0] == n:
        return counts_ext[elo:ehi]
    raise ValueError(f"expected the {ehi - elo} count rows [{elo}, {ehi}) of this rank's shard, got {counts_ext.shape[0]}")


def _shard_inputs(engine, comm, counts_ext, row_ptr, col, plan, junctions_ext, dev):
    """what quant_compare_sharded and pairwise_sharded start from -> (n, plan, part, ext, rp, cl): the plan (made here
    from the CSR unless given), this rank's part of it, its count rows and its local CSR -- cut out of (row_ptr, col),
    or clustered here from junctions_ext by a host engine (`dev`: the caller takes the device path, where the shard
    object clusters the range itself and rp = cl = None).  A rank without own rows gets counts_ext[:0] and no CSR."""
    if junctions_ext is not None:
        if plan is None:
            raise ValueError("junctions_ext needs the plan it was cut by (shard.shard_plan_junctions)")
        n = plan[-1]["own_hi"]
    else:
        n = row_ptr.size - 1
        plan = plan or shard.shard_plan(row_ptr, col, comm.world)
    part = plan[comm.rank]
    if part["own_hi"] == part["own_lo"]:
        return n, plan, part, counts_ext[:0], None, None
    ext = np.ascontiguousarray(_own_slice(counts_ext, n, part))
    rp = cl = None
    if junctions_ext is None:
        rp, cl = shard.local_csr(row_ptr, col, part)
    elif not dev:
        row_of, rp, cl = engine.cluster(*junctions_ext)             # the range alone; rows arrive in row order
        if not np.array_equal(row_of, np.arange(len(row_of))):
            raise ValueError("junctions_ext must be in output row order")
    return n, plan, part, ext, rp, cl


def _bh_masked_host(engine, p, tested):
    """host twin of sdice_bh_masked_dev for engines without device entry points (the CPU test double)"""
    keep = np.flatnonzero(tested if tested is not None else p >= 0)
    q = np.zeros(p.shape, dtype=np.float64)
    if keep.size:
        q[keep] = engine.bh(np.ascontiguousarray(p[keep]))
    return q


def shard_stats(engine, counts_ext, rp, cl, first, k, g1, g2, pad_to=None):
    """(host engines: the CPU test double)  PS -> '.3f' quantise -> rank-sum for rows [first, first + k) of one shard
    (with its halo rows) -> dict name -> array of length pad_to (default k), zero beyond k."""
    r = dict.fromkeys(STAT_NAMES, ())
    if k:
        ps = engine.quantize3(engine.ps(counts_ext, rp, cl))   # the _allPS.tsv text round trip
        r = engine.ranksum(ps[first: first + k], g1, g2)
    return {name: pad_rows(np.asarray(r[name], dt), k if pad_to is None else pad_to) for name, dt in zip(STAT_NAMES, STAT_DTYPES)}


class _RowRange:
    """One rank's row range on the device: the plan geometry (own rows [lo, hi), held rows from elo, k own rows, maxk =
    the longest shard), the count rows, and EITHER the local CSR OR the coordinates of the rows [ext_lo, ext_hi), which
    lists() then clusters itself.  Every array is allocated through empty() / to_device(), and free() releases exactly
    those."""

    def __init__(self, engine, comm, n, s, plan):
        self.e, self.comm, self.n, self.s, self.plan = engine, comm, n, s, plan
        part = plan[comm.rank]
        self.lo, self.hi, self.elo = part["own_lo"], part["own_hi"], part["ext_lo"]
        self.k = self.hi - self.lo
        self.rows_of = rows_per_rank(plan)
        self.maxk = longest(self.rows_of)
        self.owned = []
        self.d_counts = self.d_rp = self.d_cl = self.d_row_of = self.d_j = None

    def empty(self, shape, dtype):
        self.owned.append(self.e.empty(shape, dtype))
        return self.owned[-1]

    def to_device(self, host, dtype):
        self.owned.append(self.e.to_device(host, dtype))
        return self.owned[-1]

    def load_rows(self, counts_ext, rp, cl, junctions):
        """counts_ext: rows [ext_lo, ext_hi); either (rp, cl) -- the local CSR -- or junctions = (chrom_rank, left,
        right, strand) of those rows in row order"""
        self.d_counts = self.to_device(np.ascontiguousarray(counts_ext), np.int32)
        rows = self.d_counts.shape[0]
        if junctions is None:
            self.d_rp = self.to_device(rp, np.int64)
            self.d_cl = self.to_device(cl if cl.size else np.zeros(1, np.int32), np.int32)
            return
        assert len(junctions[0]) == rows, (len(junctions[0]), rows)
        self.d_j = [self.to_device(x, dt) for x, dt in zip(junctions, (np.int32, np.int32, np.int32, np.int8))]
        self.d_row_of, self.d_rp = self.empty(rows, np.int32), self.empty(rows + 1, np.int64)
        # cluster the range once synchronously.  lists() clusters it asynchronously, and an asynchronous sdice_cluster_dev
        # only sizes the context's list buffer at 16 entries per junction: a denser range would fail at the next sync.
        # The synchronous call grows the buffer to the range's list total (it never shrinks) and reports invalid or
        # duplicate junctions here.  (A range that the fast path can only cluster synchronously -- a sort bucket
        # overflow, e.g. more than 16 384 junctions sharing one (chrom, left) -- still fails in step(); that is not
        # handled here.)
        self.e.cluster_dev(*self.d_j, self.d_row_of, self.d_rp, sync=True)

    def lists(self):
        """the neighbour lists of this step: the uploaded ones, or the rank's own range clustered now, enqueued without
        a host round trip (a view of the context's list buffer: not owned, never freed here)"""
        if self.d_j is not None:
            self.d_cl, _ = self.e.cluster_dev(*self.d_j, self.d_row_of, self.d_rp, sync=False)
        return self.d_cl

    def csr_host(self):
        """(row_ptr, col, nnz) of the rows [ext_lo, ext_hi) as the device holds them (after a step)"""
        rp = self.d_rp.to_host()
        nnz = int(rp[-1])
        if self.d_j is not None:
            nnz, _ = self.e.cluster_status()            # (resolves the asynchronous clustering: deferred errors surface here)
        cl = self.d_cl.offset(0, (nnz,)).to_host() if nnz else np.zeros(0, np.int32)
        return rp, cl, nnz

    def free(self):
        for a in self.owned:
            a.free()
        self.owned = []


class CompareShard(_RowRange):
    """One rank's part of quant -> compare_sample_sets, resident in HBM (device engines).

    load() uploads the rank's count rows and EITHER its local CSR (cut out of a replicated clustering by the caller)
    OR the coordinates of its rows [ext_lo, ext_hi) -- then step() clusters that range itself (sdice_cluster_dev,
    asynchronous: no rank ever clusters the whole junction set; the lists of the own rows are complete by the plan's
    construction, shard.shard_plan_junctions).  step() is device work only: [clustering of the range,] PS with the
    '.3f' round trip fused into the store, rank-sum into ONE packed block (stat_layout), ONE all-gather of that
    block, p / tested made contiguous with two strided copies, Benjamini-Hochberg over the gathered vector
    (sdice_bh_masked_dev: padding and untested rows are absent); result() downloads and drops the padding.
    bench.py --workload e2e --gpus N times exactly this step."""

    def __init__(self, engine, comm, n, s, plan, g1, g2):
        super().__init__(engine, comm, n, s, plan)
        m, w = self.maxk, comm.world
        self.off, self.block = stat_layout(m)
        from .engine import DeviceArray
        self.packed = self.empty(self.block, np.uint8).zero()
        self.views = {name: DeviceArray(engine, (m,), dt, ptr=self.packed.ptr + at, owned=False)
                      for name, (at, dt) in self.off.items()}
        self.d_g1, self.d_g2 = self.to_device(g1, np.int32), self.to_device(g2, np.int32)
        self.d_p_all, self.d_t_all = self.empty(w * m, np.float64), self.empty(w * m, np.uint8)
        self.d_q = self.empty(w * m, np.float64)
        self.recv_buf = self.empty(w * self.block, np.uint8) if w > 1 else None    # (allocated once: step() is malloc-free)
        self.recv = self.recv_buf                    # what the last step gathered
        self.d_ps = None

    def load(self, counts_ext, rp=None, cl=None, junctions=None):
        if self.k:
            self.load_rows(counts_ext, rp, cl, junctions)
            self.d_ps = self.empty(self.d_counts.shape, np.float32)

    def step(self):
        e, k, m, w = self.e, self.k, self.maxk, self.comm.world
        if k:
            d_cl = self.lists()
            e.set_param("ps.quantize3", 1)          # the '.3f' round trip is fused into the PS store
            try:
                e.ps_dev(self.d_counts, self.d_rp, d_cl, None, self.d_ps)
            finally:
                e.set_param("ps.quantize3", 0)
            first = self.lo - self.elo
            e.ranksum_dev(self.d_ps.offset(first * self.s, (k, self.s)), self.d_g1, self.d_g2,
                          {name: v.offset(0, (k,)) for name, v in self.views.items()})
        self.recv = _allgather(self.comm, self.packed, self.recv_buf)     # ONE collective: world x block bytes
        at_p, at_t = self.off["p"][0], self.off["tested"][0]
        e.copy2d_dev(self.d_p_all.ptr, m * 8, self.recv.ptr + at_p, self.block, m * 8, w)      # rank blocks -> one vector
        e.copy2d_dev(self.d_t_all.ptr, m, self.recv.ptr + at_t, self.block, m, w)
        e.bh_masked_dev(self.d_p_all, self.d_t_all, self.d_q)

    def result(self):
        host = unpack_stats_host(self.recv.to_host(), self.maxk, self.comm.world)
        host["corrected"] = self.d_q.to_host()
        return host

    def free(self):
        if self.recv is not None and not any(self.recv is a for a in self.owned):
            self.recv.free()                         # (a communicator without allgather_into allocated it)
        super().free()


def quant_compare_sharded(engine, comm, counts_ext, row_ptr, col, g1, g2, plan=None, junctions_ext=None):
    """counts_ext: int32 rows [ext_lo, ext_hi) of the count table in output row order -- this rank's
    shard only (shard.shard_plan(row_ptr, col, world)[rank]); CSR over all rows; two column groups.

    junctions_ext = (chrom_rank, left, right, strand) of the rows [ext_lo, ext_hi), in row order: the rank clusters
    ITS range itself and no global CSR exists anywhere (row_ptr = col = None; plan = shard.shard_plan_junctions(...)
    is then required) -- the lists of its own rows are complete by the plan's construction.

    Returns dict(tested, p, z, corrected, med1, med2, mean1, mean2, delta) for ALL n rows, identical
    on every rank, plus plan.  `engine`: the HIP Context (device path) or a host double with
    ps / quantize3 / ranksum / bh (/ cluster).  The per-junction table crosses the ranks as ONE packed block in ONE all-gather.
    """
    dev = hasattr(engine, "ps_dev")
    n, plan, part, ext, rp, cl = _shard_inputs(engine, comm, counts_ext, row_ptr, col, plan, junctions_ext, dev)
    lo, hi, elo = part["own_lo"], part["own_hi"], part["ext_lo"]
    k = hi - lo
    rows_of = rows_per_rank(plan)
    max_rows = longest(rows_of)
    if dev and comm.device:
        sh = CompareShard(engine, comm, n, ext.shape[1] if k else len(g1) + len(g2), plan, g1, g2)
        try:
            sh.load(ext, rp, cl, junctions=junctions_ext if k else None)
            sh.step()
            engine.sync()
            host = sh.result()
        finally:
            sh.free()
    else:
        if dev:
            raise NotImplementedError("a device engine needs a device communicator (RcclComm / SingleComm)")
        stats = shard_stats(engine, ext, rp, cl, lo - elo, k, g1, g2, pad_to=max_rows)
        gathered = comm.allgather(pack_stats_host(stats, max_rows))             # ONE collective
        host = unpack_stats_host(gathered, max_rows, comm.world)
        host["corrected"] = _bh_masked_host(engine, host["p"], host["tested"])
    out = {name: drop_padding(a, rows_of, max_rows) for name, a in host.items()}     # rows in global order
    assert all(a.shape[0] == n for a in out.values())
    out["plan"] = plan
    return out


def gather_ps_dev(engine, comm, d_ps_own, k, s, max_rows):
    """north_star's collective: all-gather of the PS shards (padded to max_rows rows) -> device array
    [world * max_rows, s] float32.  Timed by bench.py beside the design that leaves PS where it is."""
    if k == max_rows:
        send = d_ps_own
    else:
        send = engine.empty((max_rows, s), np.float32).zero()
        engine.copy2d_dev(send.ptr, s * 4, d_ps_own.ptr, s * 4, s * 4, k)
    return comm.allgather(send)


def pair_column_ranges(pairs, world):
    """Pair columns owned by each rank for the column-wise BH: contiguous, near-equal."""
    return [(q * pairs // world, (q + 1) * pairs // world) for q in range(world)]


CHI2_ZERO_MSG = "The internally computed table of expected frequencies has a zero element"


def pair_test_host(engine, test, incl, excl, pair_list=None):
    """the chosen test of a host-array engine -> (p, n_bad); no list: exactly the calls of an all-pairs run"""
    kw = {} if pair_list is None else dict(pairs=pair_list)
    if test == "chi2":
        return engine.chi2_pairs(incl, excl, **kw)
    return engine.fisher_pairs(incl, excl, **kw), 0


def pair_test_dev(engine, test, d_incl, d_excl, d_p, d_bad, d_tab=None):
    """the chosen test of a device engine into d_p -> n_bad (chi2: one host round trip, d_bad its device word)"""
    kw = {} if d_tab is None else dict(pairs=d_tab)
    if test != "chi2":
        engine.fisher_pairs_dev(d_incl, d_excl, d_p, **kw)
        return 0
    engine.chi2_pairs_dev(d_incl, d_excl, d_p, d_bad, **kw)
    return int(d_bad.to_host()[0])


def chi2_abort(comm, n_bad, n_tables):
    """scipy.stats.chi2_contingency raises on the first table with an empty row or column and the reference run dies
    with it (pairwise_fisher.py:167-179): every rank takes the same decision from the global count (comm None: one process)"""
    total = n_bad if comm is None else comm.allsum(n_bad)
    if total:
        raise ValueError(f"{CHI2_ZERO_MSG} ({total} of {n_tables} sample-pair tables have an empty row or column)")


def _pairwise_host(engine, comm, ext, rp, cl, a0, k, plan, n, pairs, correction, test="fisher", pair_list=None):
    if k:
        excl = engine.ps(ext, rp, cl, want_excl=True, want_ps=False)
        p, n_bad = pair_test_host(engine, test, ext[a0: a0 + k], excl[a0: a0 + k], pair_list)
    else:
        p, n_bad = np.zeros((0, pairs), dtype=np.float64), 0
    if test == "chi2":
        chi2_abort(comm, n_bad, n * pairs)
    rows_of = rows_per_rank(plan)
    maxk = longest(rows_of)
    if correction == "pairwise" and pairs > 0:
        ranges = pair_column_ranges(pairs, comm.world)
        maxw = max(max(b - a for a, b in ranges), 1)
        send = np.zeros((comm.world, maxk, maxw), dtype=np.float64)
        for q, (a, b) in enumerate(ranges):                   # my rows of rank q's columns
            send[q, :k, : b - a] = p[:, a:b]
        got = comm.alltoall(send)                             # rank r's rows of MY columns
        a, b = ranges[comm.rank]
        mine = drop_padding(got.reshape(comm.world * maxk, maxw), rows_of, maxk)[:, : b - a]
        assert mine.shape == (n, b - a)
        if mine.size:
            mine = engine.bh_columns(mine)
        back, at = np.zeros((comm.world, maxk, maxw), dtype=np.float64), 0
        for r in range(comm.world):                           # corrected values go home
            back[r, : rows_of[r], : b - a] = mine[at: at + rows_of[r]]
            at += rows_of[r]
        got = comm.alltoall(back)                             # my rows of rank q's columns, corrected
        for q, (a, b) in enumerate(ranges):
            p[:, a:b] = got[q][:k, : b - a]
    elif correction == "all" and pairs > 0:
        everything = comm.allgather(pad_rows(p, maxk, fill=-1.0))      # [world * maxk, pairs], absent rows negative
        q = _bh_masked_host(engine, everything.reshape(-1), None).reshape(everything.shape)
        p = q[comm.rank * maxk: comm.rank * maxk + k]
    return p


def _groups(width, G):
    """the G column groups of a rank that owns `width` pair columns: [(lo, hi)] relative to its first column"""
    return [(g * width // G, (g + 1) * width // G) for g in range(G)]


class PairwiseShard(_RowRange):
    """One rank's part of `pairwise`, resident in HBM (device engines): load() uploads the rank's count rows and EITHER
    its local CSR OR the coordinates of its rows [ext_lo, ext_hi) (step() then clusters that range itself, as
    CompareShard does) and allocates every exchange buffer ONCE (their shapes follow from the plan); step() is device
    work only, no allocation, no synchronisation -- exclusion sums, the per-pair test of the rank's rows, and the
    correction: "pairwise" packs the p-value matrix into per-rank column blocks ON THE DEVICE (sdice_copy2d_dev),
    all-to-all, column BH on complete columns, all-to-all back, unpack; "all" all-gathers the raw matrix and ranks it
    redundantly (sdice_bh_masked_dev); "none" needs no exchange.  bench.py --workload pairwise --gpus N times exactly
    this step.  pair_list ([m, 2] column indices): the m listed pairs instead of all s(s-1)/2; load() packs the list into
    a device table once (engine.pair_table) and step() hands it to the two kernel calls."""

    def __init__(self, engine, comm, n, s, plan, correction="pairwise", test="fisher", overlap_groups=None, pair_list=None):
        super().__init__(engine, comm, n, s, plan)
        self.correction, self.test = correction, test
        self.pair_list, self.d_tab = pair_list, None
        self.pairs = s * (s - 1) // 2 if pair_list is None else len(pair_list)
        # the exchange that takes the corrected values home goes in G column groups: group g's all-to-all runs on the
        # context's second stream (sdice_comm_fork) while group g + 1 is being corrected.  Every rank derives the same G.
        self.ranges = pair_column_ranges(self.pairs, comm.world)
        wmin = min(b - a for a, b in self.ranges) if self.pairs else 0
        if overlap_groups is None:
            overlap_groups = 1 if comm.world == 1 else min(4, max(1, wmin // 1024))
        self.G = max(1, min(int(overlap_groups), max(wmin, 1))) if hasattr(engine, "comm_fork") else 1
        # block width of an exchange laid out in 1 or G column groups: the widest group any rank has
        self.gw = {G: max(max(hi - lo for a, b in self.ranges for lo, hi in _groups(b - a, G)), 1) for G in (1, self.G)}
        self.d_p = self.empty((max(self.k, 1), max(self.pairs, 1)), np.float64)
        self.d_excl = None
        self.d_bad = self.empty(1, np.int64) if test == "chi2" else None
        self.bufs = {}                                        # exchange buffers, allocated by load()
        self.ms = {}                                          # per-collective times of the last timed_collectives()

    def load(self, counts_ext, rp=None, cl=None, junctions=None):
        w, maxk, pairs = self.comm.world, self.maxk, self.pairs
        if self.k and pairs:
            self.load_rows(counts_ext, rp, cl, junctions)
            self.d_excl = self.empty(self.d_counts.shape, np.int64)
            if self.pair_list is not None:
                self.owned.append(self.e.pair_table(self.s, self.pair_list))
                self.d_tab = self.owned[-1]
        if pairs and self.correction == "pairwise":
            a, b = self.ranges[self.comm.rank]
            shape = (w, maxk, self.gw[1])
            # (G > 1: the way back is laid out [group][rank][row][column of the group], so that a group is one contiguous exchange)
            shape2 = (self.G, w, maxk, self.gw[self.G]) if self.G > 1 else shape
            self.bufs = dict(send=self.empty(shape, np.float64).zero(), back=self.empty(shape2, np.float64).zero(),
                             mine=self.empty((max(self.n, 1), max(b - a, 1)), np.float64))
            if w > 1 or self.G > 1:
                self.bufs.update(got=self.empty(shape, np.float64), got2=self.empty(shape2, np.float64))
        elif pairs and self.correction == "all":
            self.bufs = dict(pad=self.empty((maxk, pairs), np.float64), d_q=self.empty((w * maxk, pairs), np.float64))
            if w > 1:
                self.bufs["everything"] = self.empty((w * maxk, pairs), np.float64)

    def step(self):
        self._test_rows()
        if self.pairs and self.correction == "pairwise":
            self._correct_pairwise()
        elif self.pairs and self.correction == "all":
            self._correct_all()

    def _test_rows(self):
        """exclusion sums and the per-pair test of my rows -> d_p; a chi2 table with an empty row or column anywhere aborts
        every rank (the one host round trip of a step: the count of such tables)"""
        e, k, s, pairs, a0 = self.e, self.k, self.s, self.pairs, self.lo - self.elo
        n_bad = 0
        if k and pairs:
            e.ps_dev(self.d_counts, self.d_rp, self.lists(), self.d_excl, None)
            inc, exc = self.d_counts.offset(a0 * s, (k, s)), self.d_excl.offset(a0 * s, (k, s))
            n_bad = pair_test_dev(e, self.test, inc, exc, self.d_p.offset(0, (k, pairs)), self.d_bad, self.d_tab)
        if self.test == "chi2":
            chi2_abort(self.comm, n_bad, self.n * pairs)

    def _copy_my_rows(self, blocks, G, pack):
        """my rows of every rank's columns, d_p -> blocks (pack) or blocks -> d_p; `blocks` is laid out
        [group][rank][maxk rows][gw[G] columns] with every rank's columns in G groups (device, strided)"""
        gw = self.gw[G]
        for q, (a, b) in enumerate(self.ranges):
            for g, (ga, gb) in enumerate(_groups(b - a, G)):
                if self.k and gb > ga:
                    blk = (blocks.ptr + (g * self.comm.world + q) * self.maxk * gw * 8, gw * 8)
                    own = (self.d_p.ptr + (a + ga) * 8, self.pairs * 8)
                    self.e.copy2d_dev(*(blk + own if pack else own + blk), (gb - ga) * 8, self.k)

    def _copy_my_columns(self, blocks, g, G, pack):
        """every rank's rows of group g (of G) of my columns, mine -> blocks (pack) or blocks -> mine, the one [n, w] table
        of complete columns; `blocks` laid out as in _copy_my_rows"""
        a, b = self.ranges[self.comm.rank]
        w, gw, (ga, gb), at = b - a, self.gw[G], _groups(b - a, G)[g], 0
        for r, rows in enumerate(self.rows_of):
            if rows and gb > ga:
                blk = (blocks.ptr + (g * self.comm.world + r) * self.maxk * gw * 8, gw * 8)
                tab = (self.bufs["mine"].ptr + (at * w + ga) * 8, w * 8)
                self.e.copy2d_dev(*(blk + tab if pack else tab + blk), (gb - ga) * 8, rows)
            at += rows

    def _correct_pairwise(self):
        """BH down every pair column over all junctions: rows -> columns all-to-all, column BH, and the way home in G
        column groups -- with G > 1 group g travels on the second stream while group g + 1 is corrected"""
        e, comm, n, G = self.e, self.comm, self.n, self.G
        send, back, mine, got2 = self.bufs["send"], self.bufs["back"], self.bufs["mine"], self.bufs.get("got2")
        self._copy_my_rows(send, 1, pack=True)
        got = _alltoall(comm, send, self.bufs.get("got"))
        self._copy_my_columns(got, 0, 1, pack=False)
        a, b = self.ranges[comm.rank]
        group = (comm.world, self.maxk, self.gw[G])
        for g, (ga, gb) in enumerate(_groups(b - a, G)):
            if n and gb > ga:
                e.bh_columns_pitched_dev(mine.offset(ga, (n, gb - ga)), n, gb - ga, b - a)
            self._copy_my_columns(back, g, G, pack=True)
            if G > 1:
                e.comm_fork()                                 # the second stream waits for the group's packing ...
            at = g * int(np.prod(group))
            home = _alltoall(comm, back.offset(at, group), got2.offset(at, group) if got2 is not None else None,
                             in_place=G > 1)                  # ... and carries it while the main stream goes on
        if G > 1:
            e.comm_join()
            home = got2
        self._copy_my_rows(home, G, pack=False)

    def _correct_all(self):
        """one BH over the whole matrix: all-gather the raw rows, rank them redundantly, keep my rows"""
        e, comm, k, pairs, d_p = self.e, self.comm, self.k, self.pairs, self.d_p
        pad, d_q = self.bufs["pad"].memset(0xBF), self.bufs["d_q"]     # 0xBFBF... is a negative double: "absent"
        if k:
            e.copy2d_dev(pad.ptr, pairs * 8, d_p.ptr, pairs * 8, pairs * 8, k)
        everything = _allgather(comm, pad, self.bufs.get("everything"))
        e.bh_masked_dev(everything, None, d_q)
        if k:
            e.copy2d_dev(d_p.ptr, pairs * 8, d_q.ptr + comm.rank * self.maxk * pairs * 8, pairs * 8, pairs * 8, k)

    def timed_collectives(self, reps=3):
        """ms per all-to-all of the step's block shape, timed alone (after a step)"""
        if "send" not in self.bufs:
            return {}
        e, send = self.e, self.bufs["send"]
        _alltoall(self.comm, send, self.bufs.get("got"))
        e.sync()
        e.timer_start()
        for _ in range(reps):
            _alltoall(self.comm, send, self.bufs.get("got"))
        ms = e.timer_stop() / reps
        return {"alltoall_ms": ms, "alltoall_bytes_per_rank": int(send.nbytes), "alltoalls_per_step": 2}

    def result(self):
        self.e.sync()
        k, pairs = self.k, self.pairs
        return self.d_p.offset(0, (k, pairs)).to_host() if k and pairs else np.zeros((k, pairs), dtype=np.float64)

    def free(self):
        super().free()
        self.bufs = {}


def pairwise_sharded(engine, comm, counts_ext, row_ptr, col, correction="pairwise", plan=None, test="fisher",
                     junctions_ext=None, overlap_groups=None, pairs=None):
    """`pairwise` with junction rows sharded over ranks.

    counts_ext: int32 rows [ext_lo, ext_hi) of this rank's shard in row order; CSR over all rows.
    Every rank computes the exclusion sums and the s(s-1)/2 Fisher p-values of ITS rows; the
    correction modes are the reference's (pairwise_fisher.py:182-193): "pairwise" (BH down every pair
    column over all junctions), "all" (one BH over the whole matrix), "none".  test = "chi2": the Yates-corrected
    chi-square of --chi2 (pairwise_fisher.py:133-136) on the same shards; a table with a zero expected frequency anywhere
    aborts the run on every rank, as the reference's chi2_contingency does.
    junctions_ext (with plan = shard.shard_plan_junctions(...), row_ptr = col = None): the rank clusters its own rows
    [ext_lo, ext_hi) itself, as in quant_compare_sharded.  overlap_groups: column groups of the exchange that takes the
    corrected values home (device engines; default: by the width of a rank's column range, 1 on one rank).
    pairs ([m, 2] column indices, the same list on every rank): test the m listed pairs instead of all s(s-1)/2 --
    column q is pair q, any order, (j, i) the swapped table, repeats allowed; "pairwise" corrects every listed column,
    "all" the n * m listed p-values.
    Returns dict(p=[k, pairs] for this rank's own rows, own=(lo, hi), plan=...).
    """
    if correction not in ("pairwise", "all", "none"):
        raise ValueError("correction must be pairwise | all | none")
    if test not in ("fisher", "chi2"):
        raise ValueError("test must be fisher | chi2")
    dev = hasattr(engine, "fisher_pairs_dev") and comm.device    # (a device engine with a host communicator: host path)
    n, plan, part, ext, rp, cl = _shard_inputs(engine, comm, counts_ext, row_ptr, col, plan, junctions_ext, dev)
    lo, hi, elo = part["own_lo"], part["own_hi"], part["ext_lo"]
    k = hi - lo
    if not k:
        ext = np.ascontiguousarray(_own_slice(counts_ext, n, part))     # (here a rank without rows has its row count checked too)
    s = ext.shape[1]
    pair_list = None
    if pairs is not None:
        from .engine import pair_array
        pair_list = pair_array(pairs)
        if pair_list.min() < 0 or pair_list.max() >= s or (pair_list[:, 0] == pair_list[:, 1]).any():
            raise ValueError(f"pairs must name two different columns of [0, {s}) each")
    pairs = s * (s - 1) // 2 if pair_list is None else len(pair_list)
    if dev:
        sh = PairwiseShard(engine, comm, n, s, plan, correction, test, overlap_groups=overlap_groups, pair_list=pair_list)
        try:
            sh.load(ext, rp, cl, junctions=junctions_ext if k else None)
            sh.step()
            p = sh.result()
        finally:
            sh.free()
    else:
        p = _pairwise_host(engine, comm, ext, rp, cl, lo - elo, k, plan, n, pairs, correction, test, pair_list)
    return dict(p=p, own=(lo, hi), plan=plan)
