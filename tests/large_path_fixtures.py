"""Inputs for test_gpu_large_paths.py: the branches of the shared primitives (scan.hip, radix.hip, unique.hip, the
generic chain of cluster.hip, the radix path of bh.hip, the two element-wise kernels at the end of ps.hip) that only an
input SIZE selects.  Everything here is vectorised numpy: no Python loop over rows or keys, only over the handful of
pieces a table is made of.  test_large_path_fixtures_cpu.py checks the builders at small sizes against the oracle and
the cluster referee, so that the closed forms below are never their own witness.

  star_table       junctions in ROW order with their overlap lists in closed form (row_of, row_ptr, col whole), shuffled
                   by i -> a * i mod n
  junction_keys    packed junction keys whose duplicate flags, once sorted, hold whole scan blocks of zeros
  bh_pvalues       p-values whose reversed sorted order holds tie runs across chosen scan blocks
  digit_mask_keys  keys whose varying bits (OR & ~AND) are a given mask
  quantize_values  every k / 1000 neighbourhood, tiled, with boundary values in the scalar tail
  low_indices      flat indices for mark_low with duplicates, 0 and the last cell
"""
from math import gcd

import numpy as np

# ---------------------------------------------------------------------------------------------- mirrored constants
# scan.hip: SCAN_THREADS (256) * SCAN_ITEMS (8) consecutive elements per workgroup of every scan kernel
SCAN_BLOCK = 2048
# scan.hip: SCAN_SELF_MAX, the largest block count of the two-launch scan (scan_impl: `if (nb <= SCAN_SELF_MAX)`)
SCAN_SELF_MAX = 4096
# the largest input of the two-launch scan; also cluster_fast.hip: FAST_MAX_N = MAX_BUCKETS (4096) * BUCKET_MEAN (2048),
# the largest table sdice_cluster_dev keeps on the fast path (`legacy = n > FAST_MAX_N || ...`)
N0 = SCAN_SELF_MAX * SCAN_BLOCK
MAX_BUCKETS = 4096
# scan_sums_kernel walks the block sums SCAN_BLOCK at a time: its loop iterations meet at these input positions
MID, TOP = 2048 * SCAN_BLOCK, 4096 * SCAN_BLOCK
# radix.hip: a tile is THREADS (256) * ROUNDS keys, ROUNDS = param sort.rounds (12, or 4)
RADIX_TILE = {12: 3072, 4: 1024}
# radix.hip, radix_sort_passes: `if (n_tiles <= 64 && segs >= 64)` takes radix_binscan_small_kernel
BINSCAN_SMALL_MAX_TILES, BINSCAN_SMALL_MIN_SEGS = 64, 64
# bh.hip, transpose(): `chunk = 65535 * 32` rows per launch (the y extent of a grid)
TRANSPOSE_CHUNK = 65535 * 32
# bh_cols.hip: sd_bh_vector_supported (n <= 2 << 20) and sd_bh_cols_supported (m <= 1 << POS_SHIFT = 2^18): beyond them the
# radix paths of bh.hip are the only ones
BH_VECTOR_SAMPLESORT_MAX, BH_COLS_SAMPLESORT_MAX = 2 << 20, 1 << 18
# sd_bh_vector_supported again: the smallest vector the sample-sort path takes (n >= 16384)
BH_VECTOR_SAMPLESORT_MIN = 16384
# ps.hip, sdice_quantize3_dev: at most 2048 workgroups of 256 threads, 4 values per thread and pass
QUANTIZE_GRID = 2048 * 256 * 4
# ps.hip, sdice_mark_low_dev: at most 2048 workgroups of 256 threads, one index per thread and pass
MARK_LOW_GRID = 2048 * 256
LARGE_SIZES = (N0, N0 + 1, N0 + 2 * SCAN_BLOCK + 5)

STEP = 10                                            # distance of two lefts of a ladder


def multiplier(n):
    """a with gcd(a, n) = 1 near n / golden ratio: i -> a * i mod n is a permutation that sends neighbours far apart"""
    a = max(1, int(n * 0.6180339887)) | 1
    while gcd(a, n) != 1:
        a += 2
    return a


def shuffle_index(n):
    """src[i] = a * i mod n (int64): input position i holds element src[i] of the ordered sequence"""
    return (np.arange(n, dtype=np.int64) * multiplier(n)) % n


# ---------------------------------------------------------------------------------------------- clustering
class StarTable:
    """cr, left, right, strand: the shuffled input.  row_of, row_ptr, col: what sdice_cluster must return.  pieces: the
    (kind, first row, rows, starts a chromosome) list the table was made of."""


def star_pieces(n, B=SCAN_BLOCK, bounds=(MID, TOP)):
    """The layout in row order.  Stars (one long junction over k - 1 disjoint short ones, k about 3 B):
      * an early one from row 5.5 B on, followed by more ladder on the same chromosome;
      * one per boundary in `bounds` from B + B / 4 rows in front of it, so that the rows that have the star's right end
        as their prefix maximum run across it; its last short junction ends the chromosome;
      * one that ends two rows before the end of the table (the last, partial scan block when n is no multiple of B)
        and ends its chromosome; the last two rows are a chromosome of their own.
    A boundary star that would run into the last one is left out.  Plain ladders in between, two of them cut into
    two chromosomes."""
    k, k_tail = 3 * B + 7, 3 * B - 7
    tail = n - 2 - k_tail
    stars = [(5 * B + B // 2, k, False)]
    for bnd in bounds:
        s = bnd - B - B // 4
        if s + k + 4 <= tail:
            stars.append((s, k, True))
    stars.append((tail, k_tail, True))
    assert stars[0][0] + k + 4 <= stars[1][0], "table too small for its stars"
    cuts = [c for c in (n // 3 + 11, 2 * n // 3 + 5) if all(c < s - 4 or c > s + kk + 4 for s, kk, _ in stars)]
    pieces, pos, new = [], 0, True
    for s, kk, ends in stars:
        for c in [c for c in cuts if pos < c < s] + [s]:
            pieces.append(("ladder", pos, c - pos, new))
            pos, new = c, True                       # the ladder behind a cut starts a chromosome ...
        pieces.append(("star", s, kk, False))        # ... a star never does: it shares the ladder's in front of it
        pos, new = s + kk, ends
    pieces.append(("ladder", pos, n - pos, new))
    return pieces


def star_table(n, B=SCAN_BLOCK, bounds=(MID, TOP)):
    pieces = star_pieces(n, B, bounds)
    cr = np.empty(n, np.int32)
    left, right = np.empty(n, np.int64), np.empty(n, np.int64)
    e_cnt, e_hi, l_cnt = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    chrom, base = -1, 0
    for kind, s, m, new in pieces:
        assert m >= 1
        if new:
            chrom, base = chrom + 1, 100             # lefts restart below whatever the last chromosome reached
        else:
            base += 100 * STEP                       # a gap between a ladder and a star of one chromosome
        sl = slice(s, s + m)
        j = np.arange(m, dtype=np.int64)
        cr[sl] = chrom
        left[sl] = base + STEP * j
        if kind == "ladder":                         # row r lists r-1, r-2, r-3, then r+1, r+2, r+3, inside the piece
            right[sl] = left[sl] + 3 * STEP + STEP // 2
            e_cnt[sl] = np.minimum(3, j)
            e_hi[sl] = s + j - 1
            l_cnt[sl] = np.minimum(3, m - 1 - j)
        else:                                        # the star lists every short junction, each of them lists the star
            right[sl] = left[sl] + 3
            right[s] = right[s + m - 1] + 1
            e_cnt[sl], e_hi[sl], l_cnt[sl] = 1, s, 0
            e_cnt[s], l_cnt[s] = 0, m - 1
        base = int(left[s + m - 1]) + STEP
    assert left.max() < 2 ** 31 - 2 ** 20
    t = StarTable()
    t.pieces, t.n_chrom = pieces, chrom + 1
    t.row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(e_cnt + l_cnt, out=t.row_ptr[1:])
    # entry `off` of row r: the earlier rows e_hi, e_hi - 1, ... (e_cnt of them), then r + 1, r + 2, ...
    deg = (e_cnt + l_cnt).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int32), deg)
    off = np.arange(rows.size, dtype=np.int32) - np.repeat(t.row_ptr[:-1].astype(np.int32), deg)
    ec = np.repeat(e_cnt, deg)
    t.col = np.where(off < ec, np.repeat(e_hi, deg) - off, rows + 1 + off - ec).astype(np.int32)
    # one strand per chromosome, alternating: row order (chrom, left, right, strand) is the order built above
    src = shuffle_index(n)
    t.cr, t.left, t.right = cr[src], left[src].astype(np.int32), right[src].astype(np.int32)
    t.strand = (t.cr & 1).astype(np.int8)
    t.row_of = src.astype(np.int32)
    for a in (t.cr, t.left, t.right, t.strand, t.row_of, t.row_ptr, t.col):
        a.setflags(write=False)
    return t


def star_input(t):
    return t.cr, t.left, t.right, t.strand


# ---------------------------------------------------------------------------------------------- junction union
def zero_runs(n, B=SCAN_BLOCK, bounds=(MID, TOP)):
    """[lo, hi) per boundary: more than 3 B positions around it (cut at the end of the input)"""
    out = []
    for bnd in bounds:
        lo, hi = bnd - 3 * B - 77, min(n, bnd + 2 * B + 50)
        if lo > 0 and hi - lo > 3 * B:
            out.append((lo, hi))
    return out


def junction_keys(n, seed=1, B=SCAN_BLOCK, bounds=(MID, TOP), pair_at=None):
    """-> (keys, sorted_keys).  Keys are chrom (12 bits) | left (31) | span (20) | strand (1) with chromosome ranks below
    24 and spans below 2^11.  Sorted, they hold: one key repeated over each range of zero_runs (more than 3 B copies
    across a boundary of `bounds`: the scan blocks inside sum to 0); one pair of equal keys at pair_at - 1, pair_at (a
    scan block boundary) between distinct neighbours; a stretch [n / 8, n / 4) where every key is repeated with
    probability 1/2; distinct keys everywhere else."""
    rng = np.random.default_rng([seed, 0x4B])
    pair_at = 1500 * B if pair_at is None else pair_at
    inc = np.ones(n, np.int64)                               # 1: a new key at this sorted position
    inc[n // 8:n // 4] = rng.random(n // 4 - n // 8) < 0.5
    for lo, hi in zero_runs(n, B, bounds):
        inc[lo] = 1
        inc[lo + 1:hi] = 0
        if hi < n:
            inc[hi] = 1
    if 2 <= pair_at < n - 1:
        inc[pair_at - 1:pair_at + 2] = (1, 0, 1)
    inc[0] = 0
    u = np.cumsum(inc)                                       # dense id of the key at every sorted position
    per_chrom = -(-(int(u[-1]) + 1) // 24)
    chrom, w = u // per_chrom, u % per_chrom
    left = 1000 + 37 * (w >> 2)
    span = 50 + 1013 * ((w >> 1) & 1) + 3 * ((w >> 2) % 7)   # (left, span, strand) ascends with w
    assert chrom.max() < 32 and left.max() < 2 ** 31 and span.max() < 2 ** 20
    s = ((chrom << 52) | (left << 21) | (span << 1) | (w & 1)).astype(np.uint64)
    return s[shuffle_index(n)], s


# ---------------------------------------------------------------------------------------------- BH
def bh_tie_runs(m, B=SCAN_BLOCK, bounds=(MID, TOP)):
    """[lo, hi) in the REVERSED sorted order (what the min scan runs over): one run of a mid-range value across
    bounds[0]; one run of 1e-300 from 3 B in front of bounds[1] up to the two smallest values (0 and 5e-324 end the
    order), across bounds[1] when m reaches that far"""
    b0, b1 = bounds
    return (b0 - 3 * B - 77, b0 + 2 * B + 50), (b1 - 3 * B - 77, m - 2)


def bh_pvalues(m, seed=1, B=SCAN_BLOCK, bounds=(MID, TOP)):
    """-> (p, sorted_p): 30 % exact ones; 0, 5e-324 and a run of 1e-300; a run of one mid-range value; 5000 values a
    few ulps apart; distinct values otherwise.  Runs as in bh_tie_runs; shuffled by i -> a * i mod m."""
    rng = np.random.default_rng([seed, 0x42])
    (mid_lo, mid_hi), (low_lo, low_hi) = bh_tie_runs(m, B, bounds)
    n_one = int(0.3 * m)
    n_low = low_hi - low_lo
    assert n_one < mid_lo and mid_hi < low_lo and n_low > 3 * B and mid_hi - mid_lo > 3 * B
    ps = np.empty(m, np.float64)
    ps[0], ps[1] = 0.0, 5e-324
    ps[2:2 + n_low] = 1e-300
    ps[m - n_one:] = 1.0
    body = ps[2 + n_low:m - n_one]
    body[:] = np.maximum(np.sort(rng.random(body.size)) ** 3, 1e-290) * 0.999
    t, c = body.size // 3, min(5000, body.size // 8)
    body[t:t + c] = body[t] * (1.0 + np.sort(rng.integers(0, 7, size=c)) * 2.0 ** -52)
    ps[m - mid_hi:m - mid_lo] = ps[m - mid_hi]
    assert np.all(np.diff(ps) >= 0) and ps[m - n_one - 1] < 1.0
    return ps[shuffle_index(m)], ps


# ---------------------------------------------------------------------------------------------- radix digit masks
def _digits(*ds):
    return sum(0xFF << (8 * d) for d in ds)


#              name              varying bits          constant bits that must be set
MASK_SHAPES = [(f"digit_{d}", _digits(d), 0) for d in range(8)] + [
    ("digits_0_7", _digits(0, 7), 0),
    ("digits_0_2_5", _digits(0, 2, 5), 0),                   # an odd number of passes, with gaps
    ("digits_1_3_4_6", _digits(1, 3, 4, 6), 0),              # an even number, with gaps
    ("all_digits", _digits(*range(8)), 0),
    ("one_bit", 1 << 37, 0),
    ("ff_between", _digits(2, 4), 0xFF << 24),               # a constant byte of 0xFF between two varying ones
]
MASK_SIZES = [1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 3071, 3072, 3073, 6145, 786_432, 786_433]


def digit_mask_keys(n, mask, const, seed=1):
    """n keys (uint64) that agree outside `mask` and, from two keys on, differ in every bit of it"""
    rng = np.random.default_rng([seed, 0x4D])
    fixed = (0x5AC396E13C78B4D2 | const) & ~mask & 0xFFFFFFFFFFFFFFFF
    keys = (rng.integers(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1)) | rng.integers(0, 2, size=n, dtype=np.uint64)
    keys = (keys & np.uint64(mask)) | np.uint64(fixed)
    keys[0] = fixed
    if n > 1:
        keys[1] = fixed | mask
    return keys


def varying_bits(keys):
    return int(np.bitwise_or.reduce(keys) & ~np.bitwise_and.reduce(keys))


# ---------------------------------------------------------------------------------------------- element-wise kernels
def quantize_values(n, seed=1):
    """float32: the k / 1000 neighbourhoods (each k / 1000, its two neighbours, k / 1000 + 0.0005), random values, NaN, 0
    and 1, repeated up to n; the last three values, the scalar tail of the vector kernel, are rounding boundaries"""
    rng = np.random.default_rng([seed, 0x51])
    k = np.arange(0, 1001, dtype=np.float64) / 1000.0
    base = k.astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1)),
                           (k + 0.0005).astype(np.float32), rng.random(20000).astype(np.float32),
                           np.float32([np.nan, 0.0, 1.0, 0.0005, 0.9995, 0.99951, 1e-8])])
    out = np.resize(vals, n)
    out[-3:] = np.float32([0.9985, 0.9995, 0.0005])
    return out


def low_indices(n_low, n_elems, seed=1):
    """int64 flat indices: random with repeats, 0 first, the last cell second, one repeat next to the other, and as the
    LAST entry (the one the last pass of the grid-stride loop takes) a cell no other entry names"""
    rng = np.random.default_rng([seed, 0x4C])
    idx = rng.integers(0, n_elems, size=n_low, dtype=np.int64)
    lone = n_elems - 3
    idx[idx == lone] = 7
    idx[:4] = (0, n_elems - 1, 12345, 12345)
    idx[-1] = lone
    return idx
