"""Fixtures at the edges of neighbours_kernel (cluster_fast.hip): junctions given in OUTPUT ROW ORDER from explicit
coordinates, so that a row's place in its 512-row tile and in the tile's window is known by construction.

The kernel's constants: tile T = 512 rows, window = HB = 256 rows before the tile and HF = 128 after it, KMAX = 16
earlier neighbours kept per row in LDS, STAGE = 11 T list entries staged per tile.  A row's later neighbours are the
run of its strand up to the last row with left <= its right (found by search, clamped at the window's end); its
earlier neighbours are counted from the runs of the rows before it.

`FIXTURES[name]()` returns (chrom, left, right, strand); `facts(name)` what the CPU test pins about it (which row is
the fan row, its forward run, its earlier count); `reference(name)` the expected (row_ptr, col) from
tests/cluster_referee.py.  Used by test_neighbour_edges_cpu.py and test_gpu_neighbour_edges.py.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_referee as R  # noqa: E402
from splicedice_amd import synth  # noqa: E402

T, HB, HF, KMAX = 512, 256, 128, 16
STAGE = 11 * T
STEP = 10


class Rows:
    """junctions appended in row order on one chromosome at a time; `pos` is the next free coordinate"""

    def __init__(self):
        self.rows = []
        self.chrom, self.pos = 0, 100

    def __len__(self):
        return len(self.rows)

    def add(self, left, right, strand=0):
        self.rows.append((self.chrom, int(left), int(right), int(strand)))
        return len(self.rows) - 1

    def skip_past(self, coord):
        self.pos = max(self.pos, int(coord) + STEP)

    def singles(self, k, strand=0, alternate_from=None):
        """k disjoint junctions (left, left + 2); alternate_from = j: row j + i gets strand i % 2 (... the row at j is '+')"""
        for i in range(k):
            s = strand if alternate_from is None else (len(self.rows) - alternate_from) % 2
            self.add(self.pos, self.pos + 2, s)
            self.pos += STEP

    def singles_to(self, n_rows, **kw):
        self.singles(n_rows - len(self.rows), **kw)

    def new_chrom(self, pos):
        self.chrom += 1
        self.pos = pos

    def arrays(self):
        a = np.array(self.rows, np.int64)
        out = a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.int8)
        assert np.array_equal(R.row_order(*out), np.arange(a.shape[0])), "fixture is not in row order"
        assert np.unique(a, axis=0).shape[0] == a.shape[0]
        return out


# ------------------------------------------------------------------------------------------------ forward fan
def forward_fan(m, at, interleaved):
    """one long junction at row `at` (511: a tile's last row, 512: a tile's first) whose right covers exactly the next m
    junctions of its strand; interleaved: the rows around it alternate strands, so the m-th is 2 m rows ahead"""
    lay = Rows()
    alt = at if interleaved else None
    lay.singles_to(at, alternate_from=alt)
    pitch = 2 * STEP if interleaved else STEP              # distance between two junctions of the fan's strand
    fan = lay.add(lay.pos, lay.pos + m * pitch + STEP // 2, 0)
    lay.pos += STEP
    lay.singles_to(at + 1 + 700, alternate_from=alt)
    return lay, {"fan_row": fan, "later": m, "last_later_row": at + (2 * m if interleaved else m)}


# ------------------------------------------------------------------------------------------------ backward fan
def backward_fan(m, chrom_change):
    """m earlier junctions that all reach row 1024 (first row of tile 2, window start 768).  They contain one point, so
    they overlap each other too.  Without a chromosome change the longest of them makes `exact` false for the target;
    chrom_change: the fan's chromosome starts at the fan, so with m = 255 the window starts on the chromosome before
    and the target counts its 255 earlier neighbours inside the window"""
    lay = Rows()
    target = 2 * T
    lay.singles_to(target - m)
    if chrom_change:
        lay.new_chrom(lay.pos - 300)                       # (coordinates go on numerically across the change)
    p = lay.pos + STEP * m
    for i in range(m):
        lay.add(lay.pos + STEP * i, p + 3 * STEP + i)
    row = lay.add(p, p + 2)
    lay.skip_past(p + 3 * STEP + m)
    lay.singles(300)
    return lay, {"target_row": row, "earlier": m}


# ------------------------------------------------------------------------------------------------ KMAX edge
KMAX_CASES = [(b, f) for b in (15, 16, 17) for f in (0, 1, 40)]


def kmax_edge():
    """nine rows with b earlier and f later neighbours, b in {15, 16, 17}, f in {0, 1, 40}, behind 800 singletons (the
    window of every one starts more than the longest junction before it: `exact`; the nine lie on both sides of
    row 1024).  The earlier ones end AT the row's left, the later ones lie inside it"""
    lay = Rows()
    lay.singles(800)
    targets = {}
    for b, f in KMAX_CASES:
        p = lay.pos + STEP * b
        for i in range(b):
            lay.add(lay.pos + STEP * i, p)
        targets[(b, f)] = lay.add(p, p + STEP * f + STEP // 2)
        for k in range(1, f + 1):
            lay.add(p + STEP * k, p + STEP * k + 2)
        lay.skip_past(p + STEP * f + STEP // 2)
        lay.singles(3)
    lay.singles(40)
    return lay, {"targets": targets}


# ------------------------------------------------------------------------------------------------ chromosome change
CHROM_CHANGES = (300, 560, 1100)       # inside tile 0 (and tile 1's back halo), in tile 0's front halo, in tile 1's front halo


def chrom_change():
    """ladders of reach 9 on both strands; a new chromosome begins at rows 300, 560 and 1100 with coordinates that go on
    50 below where the previous one ended, so rows on either side of a change overlap numerically"""
    lay = Rows()
    cuts = CHROM_CHANGES + (1400,)
    at = 0
    for cut in cuts:
        while len(lay) < cut:
            s = len(lay) % 2
            lay.add(lay.pos + s, lay.pos + s + 9 * STEP + STEP // 2, s)
            if s:
                lay.pos += STEP
        at = cut
        lay.new_chrom(lay.pos - 50)
    return lay, {"changes": CHROM_CHANGES, "rows": at}


# ------------------------------------------------------------------------------------------------ ties
def ties():
    """behind 506 singletons (the group straddles the end of tile 0), on both strands: three junctions with one left;
    D starts AT the right of A (neighbours), E one past it (not neighbours of A); F starts one past the right of C
    (not neighbours), G AT the right of F (neighbours)"""
    lay = Rows()
    lay.singles(506)
    b = lay.pos
    named = {}
    for name, (lo, hi) in (("A", (0, 100)), ("B", (0, 200)), ("C", (0, 300)), ("D", (100, 150)), ("E", (101, 160)),
                           ("F", (301, 400)), ("G", (400, 500))):
        for s in (0, 1):
            named[name, s] = lay.add(b + lo, b + hi, s)
    lay.skip_past(b + 500)
    lay.singles(30)
    return lay, {"named": named}


# ------------------------------------------------------------------------------------------------ dense tile
def dense_tile():
    """600 junctions of one strand that all contain one point: every row lists the 599 others, a tile's total is far
    above STAGE"""
    lay = Rows()
    for i in range(600):
        lay.add(100 + i, 10000 + i)
    return lay, {}


# ------------------------------------------------------------------------------------------------ row counts
def gene_layout(n):
    cr, left, right, strand = synth.make_junctions(n, 40 + n % 7, n_chrom=2, gene_spacing=6000)
    o = np.lexsort((strand, right, left, cr))
    lay = Rows()
    lay.rows = [(int(cr[i]), int(left[i]), int(right[i]), int(strand[i])) for i in o]
    return lay, {"n": n}


def _builders():
    out = {}
    for at in (511, 512):
        for m in (127, 128, 129):
            out[f"ffan-one-{at}-{m}"] = functools.partial(forward_fan, m, at, False)
        for m in (63, 64, 65):
            out[f"ffan-two-{at}-{m}"] = functools.partial(forward_fan, m, at, True)
    for m in (255, 256, 257):
        out[f"bfan-{m}"] = functools.partial(backward_fan, m, False)
        out[f"bfan-chrom-{m}"] = functools.partial(backward_fan, m, True)
    out["kmax"] = kmax_edge
    out["chrom"] = chrom_change
    out["ties"] = ties
    out["dense"] = dense_tile
    for n in (1, 2, 511, 512, 513, 1537):
        out[f"genes-{n}"] = functools.partial(gene_layout, n)
    return out


BUILDERS = _builders()
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def _built(name):
    lay, facts = BUILDERS[name]()
    return lay.arrays(), facts


def junctions(name):
    return _built(name)[0]


def facts(name):
    return _built(name)[1]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(row_ptr, col) by the referee: row_ptr in closed form, col as the brute-force list of every row; the two must
    agree on every degree"""
    junc = junctions(name)
    row_ptr = R.row_ptr(*junc)
    lister = R.RowLister(*junc)
    lists = [lister(r) for r in range(junc[0].size)]
    assert [x.size for x in lists] == np.diff(row_ptr).tolist()
    col = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    for x in (row_ptr, col):
        x.setflags(write=False)
    return row_ptr, col


def split(name):
    """per row: (earlier, later) neighbour counts"""
    row_ptr, col = reference(name)
    rows = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    n = row_ptr.size - 1
    return np.bincount(rows[col < rows], minlength=n), np.bincount(rows[col > rows], minlength=n)
