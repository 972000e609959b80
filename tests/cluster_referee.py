"""Referee for the clustering sort stage: numpy on the host, no GPU, and none of the kernels' method.

`row_order`, `row_ptr` and `row_list` state WHAT sdice_cluster returns, from the definition alone (row order is
(chrom, left, right, strand); two junctions of one chromosome and strand are neighbours iff their closed
intervals overlap; a list holds the earlier rows most recent first, then the later ones in order):
  row_order   one np.lexsort
  row_ptr     closed-form degrees in O(n log n): one searchsorted and one difference array per (chrom, strand) group
  row_list    the list of ONE row by brute force over all rows, O(n)
They are checked whole against oracle_np.cluster_csr (the reference's loop) in test_cluster_sort_cpu.py and can
then stand in for it at sizes the Python sweep cannot reach.

`sort_plan` restates HOW cluster_fast.hip splits the junctions into buckets (fast_plan's clamps, sample_pos, the
sample ranks, the splitters) and which of its code paths each bucket takes.  It only proves which paths a
fixture drives: nothing it returns is ever the expected value of a device result, except that its `slot_cap`
is pinned against the device by the overflow test.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------- what is computed


def _as64(cr, left, right, strand):
    return (np.asarray(cr).astype(np.int64), np.asarray(left).astype(np.int64), np.asarray(right).astype(np.int64),
            np.asarray(strand).astype(np.int64))


def row_order(cr, left, right, strand):
    """row_of int32[n]: output row of input junction i, the inverse of np.lexsort((strand, right, left, cr))."""
    cr, left, right, strand = _as64(cr, left, right, strand)
    order = np.lexsort((strand, right, left, cr))
    row_of = np.empty(order.size, np.int32)
    row_of[order] = np.arange(order.size, dtype=np.int32)
    return row_of


def rows(cr, left, right, strand):
    """the four arrays in row order (int64)"""
    cr, left, right, strand = _as64(cr, left, right, strand)
    order = np.lexsort((strand, right, left, cr))
    return cr[order], left[order], right[order], strand[order]


def row_ptr(cr, left, right, strand):
    """row_ptr int64[n + 1] from closed-form degrees.  Inside one (chrom, strand) group in (left, right) order, the
    later neighbours of member i are the contiguous run i + 1 .. hi_i - 1 with hi_i = searchsorted(left, right_i,
    'right') (every later left that does not exceed right_i); the earlier neighbours of member j are the members i
    whose run covers j, counted by a difference array (+1 at i + 1, -1 at hi_i) and a cumsum."""
    c, l, r, s = rows(cr, left, right, strand)
    n = c.size
    deg = np.zeros(n, np.int64)
    # group members in (left, right) order: the row order restricted to the group
    g = np.lexsort((r, l, s, c))
    gc, gs = c[g], s[g]
    cut = np.flatnonzero((np.diff(gc) != 0) | (np.diff(gs) != 0)) + 1
    for lo, hi in zip(np.r_[0, cut], np.r_[cut, n]):
        if hi <= lo:
            continue
        idx = g[lo:hi]
        gl, gr = l[idx], r[idx]
        m = hi - lo
        end = np.searchsorted(gl, gr, side="right")            # >= i + 1: left_i <= right_i
        later = end - (np.arange(m) + 1)
        diff = np.zeros(m + 1, np.int64)
        np.add.at(diff, np.arange(m) + 1, 1)
        np.add.at(diff, end, -1)
        earlier = np.cumsum(diff)[:m]
        deg[idx] = later + earlier
    out = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=out[1:])
    return out


class RowLister:
    """row_list for many rows of one table (the sort is done once)."""

    def __init__(self, cr, left, right, strand):
        self.c, self.l, self.r, self.s = rows(cr, left, right, strand)

    def __call__(self, r):
        c, l, rr, s = self.c, self.l, self.r, self.s
        lo, hi = np.searchsorted(c, c[r], side="left"), np.searchsorted(c, c[r], side="right")    # its chromosome's rows
        hit = lo + np.flatnonzero((s[lo:hi] == s[r]) & (l[lo:hi] <= rr[r]) & (rr[lo:hi] >= l[r]))
        return np.concatenate([hit[hit < r][::-1], hit[hit > r]]).astype(np.int32)


def row_list(cr, left, right, strand, r):
    """The neighbour list of row r by brute force over all rows of its chromosome: the overlapping rows of its strand,
    the earlier ones in descending row order, then the later ones ascending."""
    return RowLister(cr, left, right, strand)(r)


# ---------------------------------------------------------------------------------------------- how it is sorted
BUCKET_MEAN, MAX_BUCKETS, SLOT_FACTOR = 2048, 4096, 8
RDX_CAP, RDX_IDX_BITS, SORT_LDS_ELEMS = 8192, 13, 4096
SS_MIN, SS_MAX = 512, 6400
_GOLDEN = 0x9E3779B97F4A7C15


def _bits(v):
    return int(v).bit_length()


def sample_positions(n, S):
    """sample_pos(i, n, S) for i in 0..S-1: one jittered position per stride, jitter from a 64-bit multiplicative hash"""
    stride = n // S
    out = np.empty(S, np.int64)
    for i in range(S):
        h = ((i * _GOLDEN) & 0xFFFFFFFFFFFFFFFF) >> 33
        out[i] = i * stride + h % stride
    return out


class SortPlan:
    """B, S, spb, slot_cap, lds_cap; per bucket: count, total_bits (99 where the kernel does not measure them) and
    cls ('A'..'H'); bucket_of[i] for every input junction; start[b] = first row of bucket b."""

    def classes(self):
        return set(self.cls[self.count > 0])

    def buckets(self, cls):
        return np.flatnonzero((self.cls == cls) & (self.count > 0))


def sort_plan(cr, left, right, *, bucket_mean=0, spb=0, lds_cap=0):
    """Which bucket every junction lands in, and which path of bucket_sort_kernel sorts each bucket.  Knob values as
    they would be handed to the library (0 = default, out of range = default)."""
    cr, left, right, _ = _as64(cr, left, right, np.zeros(len(cr)))
    n = cr.size
    p = SortPlan()
    if bucket_mean < 256 or bucket_mean > BUCKET_MEAN:
        bucket_mean = BUCKET_MEAN
    B = max(1, min(MAX_BUCKETS, -(-n // bucket_mean)))
    if spb < 2 or spb > 64:
        spb = 12 if n <= (2 << 20) else 8
    S = B * spb if B > 1 else 0
    mean = -(-n // B)
    slot_cap = min(mean * SLOT_FACTOR, n) if B > 1 else n
    if lds_cap <= 0 or lds_cap > 8192:
        lds_cap = 8192
    lds_cap = max(lds_cap, 2)
    p.n, p.B, p.S, p.spb, p.slot_cap, p.lds_cap = n, B, S, spb, slot_cap, lds_cap
    key = (cr.astype(np.uint64) << np.uint64(32)) | left.astype(np.uint64)
    if B == 1:
        bucket_of = np.zeros(n, np.int64)
        p.sample_pos = np.zeros(0, np.int64)
    else:
        pos = sample_positions(n, S)
        sk = key[pos]
        ranked = sk[np.argsort(sk, kind="stable")]            # rank = position in (key, sample index) order
        spl = ranked[spb::spb][: B - 1]                        # rank spb, 2 spb, ... -> slots 0 .. B - 2
        assert spl.size == B - 1
        bucket_of = np.searchsorted(spl, key, side="right")    # number of splitters <= key
        p.sample_pos = pos
    p.bucket_of = bucket_of
    p.count = np.bincount(bucket_of, minlength=B).astype(np.int64)
    p.start = np.r_[0, np.cumsum(p.count)[:-1]]
    p.total_bits = np.full(B, 99, np.int64)
    p.cls = np.full(B, "-", dtype="<U1")
    overflow = bool((p.count > slot_cap).any())
    order = np.argsort(bucket_of, kind="stable")
    length = right - left
    for b in range(B):
        cnt = int(p.count[b])
        if cnt == 0:
            continue
        if overflow:                                           # the whole chain is redone: no bucket is sorted here
            p.cls[b] = "H"
            continue
        if cnt > RDX_CAP or cnt > lds_cap:
            p.cls[b] = "E"
            continue
        idx = order[p.start[b]: p.start[b] + cnt]
        c, l = cr[idx], left[idx]
        bits = _bits(c.max() - c.min()) + _bits(l.max() - l.min()) + _bits(length[idx].max()) + 1
        p.total_bits[b] = bits
        if bits + RDX_IDX_BITS <= 64:
            p.cls[b] = "A" if cnt < SS_MIN else "B" if cnt <= 2048 else "C" if cnt <= SS_MAX else "D"
        else:
            p.cls[b] = "F" if cnt <= SORT_LDS_ELEMS else "G"
    p.overflow = overflow
    return p
