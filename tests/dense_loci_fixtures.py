"""Dense loci as junction fixtures: the layout helper, the named loci with their counts, and the PS reference that
test_gpu_dense_loci.py and ps_count_fixtures.py share.  What each locus holds is asserted by the CPU tests of
test_gpu_dense_loci.py."""
import functools

import numpy as np
import scipy.sparse

from oracle import oracle_np as O

STEP = 10                  # ladder pitch (bp)
NB_T = 512                 # neighbours_kernel tile rows
KMAX = 16
HB, HF = 256, 128
STAGE = 11 * NB_T
F24 = 1 << 24
T_PS = 1024                # ps.threads default: the gen-2 kernel stages at most 3 T list entries
S = 16                     # count columns of the PS fixtures
STAR_CAP = 65000           # largest count on the stars of degree 252 .. 256: 257 x 65 000 < 2^24


# ------------------------------------------------------------------------------ fixture construction
class _Layout:
    """Junctions appended in output row order (chrom, left, right, strand): every element starts right of everything
    before it on the chromosome, so rows come out in construction order and elements never overlap each other."""

    def __init__(self):
        self.c, self.l, self.r, self.s = [], [], [], []
        self.chrom, self.pos = 0, 100

    def _add(self, left, right, strand):
        left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
        self.c.append(np.full(left.size, self.chrom, np.int32))
        self.l.append(left)
        self.r.append(right)
        self.s.append(np.broadcast_to(np.asarray(strand, np.int8), left.shape).copy())
        self.pos = max(self.pos, int(right.max()) + STEP)

    def pad_to(self, R):
        """singletons up to the next multiple of R rows"""
        return self.singletons(-sum(len(x) for x in self.c) % R)

    def new_chrom(self, rank=None):
        self.chrom = self.chrom + 1 if rank is None else rank
        self.pos = 100

    def ladder(self, n, m, both=False):
        """junction i = (i STEP, i STEP + m STEP + STEP / 2): interior rows list m rows on either side.  both: the same
        ladder on '-' as well, 1 bp to the right, so that the strands interleave row by row"""
        left = self.pos + STEP * np.arange(n, dtype=np.int64)
        right = left + m * STEP + STEP // 2
        if not both:
            self._add(left, right, 0)
        else:
            self._add(np.stack([left, left + 1], 1).ravel(), np.stack([right, right + 1], 1).ravel(), np.tile([0, 1], n))
        return self

    def fan(self, k):
        """k junctions sharing their left end: every row lists the k - 1 others"""
        self._add(np.full(k, self.pos), self.pos + 1 + np.arange(k), 0)
        return self

    def singletons(self, k):
        if k:
            left = self.pos + STEP * np.arange(k, dtype=np.int64)
            self._add(left, left + 2, 0)
        return self

    def star(self, k, giant=False):
        """one long junction over k disjoint short ones (degree k; every short row has degree 1)"""
        left = self.pos + 5 + STEP * np.arange(k, dtype=np.int64)
        self._add(np.concatenate([[self.pos], left]), np.concatenate([[left[-1] + 4 + (10 ** 7 if giant else 0)], left + 3]), 0)
        return self

    def arrays(self):
        cr, left, right, st = (np.concatenate(x) for x in (self.c, self.l, self.r, self.s))
        assert right.max() < 2 ** 31 - 1
        return cr.astype(np.int32), left.astype(np.int32), right.astype(np.int32), st.astype(np.int8)


def _nk_tiles(lay, R, targets):
    """tiles of R rows whose lists hold targets[t] entries in all: fans (k (k - 1) entries each), singletons, and for an
    odd total a pair across the tile's end (one entry on either side)"""
    carry = 0
    for want in targets:
        budget, odd = want - carry, (want - carry) % 2
        budget -= odd
        used = carry
        while budget:
            k = int((1 + np.sqrt(1 + 4 * budget)) / 2) + 1
            while k * (k - 1) > budget:
                k -= 1
            lay.fan(k)
            budget -= k * (k - 1)
            used += k
        assert used + odd <= R
        lay.singletons(R - used - odd)
        if odd:
            lay.fan(2)
        carry = odd
    lay.singletons(R - carry)


def _build(name):
    lay = _Layout()
    if name == "kmax":                       # degrees 16 / 17 / 18 (interior 2 m, odd at the ends of a ladder)
        lay.ladder(700, 8).ladder(700, 9).singletons(3).ladder(40, 8).ladder(700, 9)
    elif name == "stage":                    # tile totals 6072 - 2 N1 around STAGE = 5632
        for n1 in (246, 221, 220, 219, 194, 220):
            lay.ladder(n1, 5).ladder(NB_T - n1, 6)
    elif name == "hf":                       # reach 127 / 128 / 129 around HF
        for m in (127, 128, 129):
            lay.ladder(900, m)
    elif name == "hb":                       # reach 255 / 256 / 257 around HB and the 255 saturation of the reach words
        for m in (255, 256, 257):
            lay.ladder(1100, m)
    elif name == "star":                     # degree 252 .. 256 around the fast-item cutoff at 254, 300 past the halo
        for k in (252, 253, 254, 255, 256):  # (long rows at the start of a 256-row tile, its short rows inside it)
            lay.pad_to(256).star(k)
        lay.pad_to(256).singletons(64).star(300).singletons(40)
    elif name == "giant":                    # one junction over 40 000: distances > 32 767, `exact` off everywhere
        lay.singletons(7).star(40000, giant=True)
        lay.new_chrom()                      # (`exact` is off on every chromosome: rows of 17 earlier neighbours)
        lay.ladder(1500, 20).ladder(300, 17).singletons(3)
        for _ in range(5):
            lay.fan(18)
        lay.fan(17).ladder(300, 9).pad_to(NB_T)
        for _ in range(2):                   # staged tiles (lists built from the 16-bit list in LDS) of such rows
            for _ in range(12):
                lay.fan(18)
            lay.fan(17).pad_to(NB_T)
    elif name == "strands":                  # both strands interleaved; chromosome changes inside tiles and windows
        for rank, rows in ((0, 150), (1, 350), (3, 19), (4, 500), (7, 260)):
            lay.new_chrom(rank)
            lay.ladder(rows, 9, both=True)
    elif name == "fans":                     # several fans per tile (totals far above STAGE), fans up to 1000
        lay.fan(2).singletons(5)
        for _ in range(20):
            lay.fan(17)
        lay.singletons(NB_T - 347)
        for _ in range(31):
            lay.fan(17)
        for _ in range(6):
            lay.fan(100)
        lay.fan(300).fan(1000).singletons(11).fan(999)
    elif name == "nk64":                     # ps.tile_rows 64: tile list totals at 16 R = 1024
        _nk_tiles(lay, 64, (500, 1024, 1025, 1023, 1024, 1026, 1025, 1024, 700))
    elif name == "nk256":                    # ps.tile_rows 256: totals at 3 T = 3072 (gen-2) and 16 R = 4096 (gen-1)
        _nk_tiles(lay, 256, (1000, 3072, 3073, 3071, 4096, 4097, 4095, 3072, 2000))
    elif name == "cmax":                     # (degree + 1) x tile max count at 2^24 - 1, 2^24, 2^24 + 33 (tiles of 64)
        for fans in _CMAX_FANS:
            for _ in range(4):
                for k in fans:
                    lay.fan(k)
    else:
        raise KeyError(name)
    return lay.arrays()


# (fans per 64-row tile, tile max count, largest fan column sum) of the three regimes of the "cmax" fixture, 4 tiles each
_CMAX_FANS = ((17, 17, 17, 13), (16, 16, 16, 16), (17, 17, 17, 13))
_CMAX = ((F24 - 1) // 17, F24 // 16, 986897)           # 17 x 986 895 = 2^24 - 1; 16 x 2^20 = 2^24; 17 x 986 897 = 2^24 + 33

CLUSTER_FIXTURES = ("kmax", "stage", "hf", "hb", "star", "giant", "strands", "fans")
ASYNC_FITS = ("stage", "star", "giant", "nk64", "nk256", "cmax")       # lists within the 16 n + 1024 of an asynchronous call
ASYNC_DENSE = ("strands", "kmax", "hf", "hb", "fans")                 # ... beyond it
PS_FIXTURES = CLUSTER_FIXTURES + ("nk64", "nk256", "cmax")


@functools.lru_cache(maxsize=None)
def junctions(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def oracle_csr(name):
    return O.cluster_csr(*junctions(name))


def _row_reach(row_ptr, col):
    n = row_ptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    reach = np.zeros(n, np.int64)
    np.maximum.at(reach, rows, np.abs(col.astype(np.int64) - rows))
    return reach


def _tile_totals(row_ptr, R):
    return np.diff(row_ptr[np.minimum(np.arange(0, row_ptr.size - 1 + R, R), row_ptr.size - 1)])


@functools.lru_cache(maxsize=None)
def counts(name):
    """int32 [n, S] below 2^24, zeros included (0 / 0 -> NaN)"""
    n = junctions(name)[0].size
    rng = np.random.default_rng(sum(map(ord, name)))
    c = rng.integers(0, 40, (n, S)).astype(np.int32)
    c[rng.random(n) < 0.05] = 0
    c[:, 5] = np.where(rng.random(n) < 0.3, 0, c[:, 5])
    c[n // 3: n // 3 + 700, 6] = 0                # (a zero run longer than the reach: 0 / 0 inside it)
    if name in ("hb", "fans"):             # degree >= 300 with counts near 2^24: exclusion sums beyond 2^32
        c[:, :4] = rng.integers(F24 - 1000, F24, (n, 4))
    if name == "star":
        row_ptr, col = oracle_csr(name)[1:]
        deg = np.diff(row_ptr)
        for r in np.flatnonzero(deg > 1):
            rows = np.concatenate([[r], col[row_ptr[r]:row_ptr[r + 1]]])
            if deg[r] < 300:                 # (degree + 1) x tile max count < 2^24 up to degree 256: fast unless deg >= 254
                c[rows, 0] = STAR_CAP
                c[rows, 1:4] = rng.integers(STAR_CAP - 2000, STAR_CAP + 1, (rows.size, 3))
            else:                            # counts near 2^24 at degree 300: exclusion sums beyond 2^32
                c[rows, :4] = rng.integers(F24 - 1000, F24, (rows.size, 4))
    if name == "cmax":
        row_ptr = oracle_csr(name)[1]
        at = 0
        for fans, cap in zip(_CMAX_FANS, _CMAX):
            for _ in range(4):
                for k in fans:
                    c[at:at + k] = _fan_counts(rng, k, cap, row_ptr[at + 1] - row_ptr[at] + 1)
                    at += k
        assert at == n
    return c


def _fan_counts(rng, k, cap, rows_in_sum):
    """counts of one fan (every row's incl + excl is the fan's column sum).  Column 0: every row at `cap`, so the sum
    reaches (degree + 1) x cap; the others start there and lose a few units, an even number when the full sum is odd, so
    every sum keeps the parity of k x cap (the 2^24 + 33 regime: odd sums above 2^24, which float32 cannot hold)"""
    assert rows_in_sum == k
    out = np.full((k, S), cap, np.int64)
    if k * cap < (F24 * 15) // 16:          # (the short fans of a tile: any counts up to the cap)
        out[:, 1:] = rng.integers(cap - 5000, cap + 1, (k, S - 1))
        return out
    for col in range(1, S):
        d = int(rng.integers(0, 17)) * 2
        take = rng.multinomial(d, np.full(k, 1.0 / k))
        out[:, col] -= take
    return out


def ps_reference(cnt, row_ptr, col):
    """calculate_psi_vectorised's arithmetic with the exclusion sums as an int64 sparse product (no [nnz, s] gather)"""
    n = cnt.shape[0]
    adj = scipy.sparse.csr_matrix((np.ones(col.size, np.int64), col.astype(np.int64), row_ptr), shape=(n, n))
    excl = np.asarray(adj @ cnt.astype(np.int64), dtype=np.int64)
    incl = cnt.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ps = (incl / (incl + excl.astype(np.float64))).astype(np.float32)
    return ps, excl
