"""Count tables for the 16-bit-window PS kernel (ps.hip, ps_tile_w16_kernel), built with the builder and checked against
the integer oracle of ps_count_fixtures.py.  Used by test_gpu_ps_w16.py; every claim made here about a fixture is
asserted without a GPU by test_ps_w16_fixtures_cpu.py.

The kernel keeps a tile's window in LDS as min(count, 0xFFFF) and decides per item, from bound = the largest count the
tile loaded (own rows and the halo rows it staged):

  tier 1   (degree + 1) x bound <= 0xFFFF: sums in the 16-bit halves
  tier 2   bound < 0xFFFF: 32-bit sums of the halves; bound >= 0xFFFF: the same unless a half the item read is 0xFFFF
  tier 3   everything else: every count from global memory, 64-bit sums

The tiles are TILE rows (the kernel's one geometry), every second one a tile of rows without neighbours and counts
below 4, so no named tile sees another one through its halo.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402

TILE, HALO = 96, 16
U16 = 0xFFFF
SMALL = 100                                   # the count of the rows that list a special row
# (rows k, count cap) of a fan in which every row lists all the others: (degree + 1) x bound = k x cap
FANS_AT_LIMIT = ((3, 21845), (5, 13107), (15, 4369), (17, 3855))          # k x cap = 65535: the last tier-1 item
FANS_PAST_LIMIT = ((2, 32768), (4, 16384), (16, 4096))                   # k x cap = 65536: the first tier-2 item
MAXIMA = (65534, 65535, 65536, PC.I31)
WHERE = ("own", "below", "above", "beyond")
LISTERS = (3, 4, 40)                          # rows of the tile that list the special row


def _tile(b, name):
    b.pad_to(TILE)
    b.marks[name] = b.n
    return b.n


def _close(b):
    b.pad_to(TILE)
    b.singles(TILE)


@functools.lru_cache(maxsize=None)
def limits(s):
    """one tile per fan of FANS_AT_LIMIT and FANS_PAST_LIMIT, all rows of the fan at cap in column 0 (total k x cap) and a
    little below it in the others (fan_counts)"""
    b = PC._Builder(s, 16)
    b.singles(TILE)
    for k, cap in FANS_AT_LIMIT + FANS_PAST_LIMIT:
        _tile(b, f"fan{k}x{cap}")
        cnt = PC.fan_counts(k, cap, s)
        cnt[:, 0] = cap
        b.fan(cnt)
        _close(b)
    return b.done()


@functools.lru_cache(maxsize=None)
def maxima(s):
    """one tile per (value, place): a fan of 6 rows at SMALL, three rows of which (LISTERS, one of them outside the fan)
    also list the special row, which holds `value` in column 0, value - 1 in column 1 and value - (c mod 3) further on.
    The special row is a row of the tile (own), the row in front of the tile (below), the row behind it (above), or a row
    no window of the tile holds (beyond: then the tile's bound stays SMALL)."""
    b = PC._Builder(s, 17)
    b.singles(TILE)
    cols = np.arange(s)
    far = TILE // 2                                        # a row of the first tile: beyond every named window
    b.rows[far][:] = PC.I31 - (cols % 3)
    for value in MAXIMA:
        for where in WHERE:
            r0 = _tile(b, f"{where}{value}")
            b.fan(np.full((6, s), SMALL, np.int64))
            b.singles(TILE - 6)
            b.singles(TILE)
            special = {"own": r0 + 50, "below": r0 - 1, "above": r0 + TILE, "beyond": far}[where]
            if where != "beyond":
                b.rows[special][:] = value - (cols % 3)
                b.rows[special][1] = value - 1
            for i in LISTERS:
                b.lists[r0 + i].append(special)
    return b.done()


@functools.lru_cache(maxsize=None)
def dense(s):
    """degrees beyond one batch of neighbours: a fan of 40 at counts below 1600 (40 x 1599 <= 0xFFFF: tier 1), a fan of 40
    around 30000 (tier 2), a star of 300 leaves (degree 300: beyond the cutoff of 254, its leaves reach beyond the halo),
    and a fan of 45 (45 x 44 list entries: beyond the 16 x TILE staged offsets, every item of that tile is tier 3)"""
    b = PC._Builder(s, 18)
    b.singles(TILE)
    rng = np.random.default_rng(19)
    _tile(b, "fan40_small")
    b.fan(rng.integers(0, 1600, (40, s)))
    _close(b)
    _tile(b, "fan40_large")
    b.fan(rng.integers(29000, 31000, (40, s)))
    _close(b)
    _tile(b, "star300")
    b.star(rng.integers(0, 50, (301, s)))
    _close(b)
    _tile(b, "fan45")
    b.fan(rng.integers(0, 50, (45, s)))
    _close(b)
    return b.done()


def window_max(fx, r0, halo=HALO, rows=TILE):
    """the largest count in rows [r0 - halo, r0 + rows + halo): the bound of the tile at r0 when both halo runs are staged"""
    return int(fx.counts[max(r0 - halo, 0):r0 + rows + halo].max())


def saturated_sums(fx, r):
    """exclusion sums of row r taken from the saturated window, min(count, 0xFFFF): what tier 2 would store if it trusted
    a saturated half"""
    nb = fx.col[fx.row_ptr[r]:fx.row_ptr[r + 1]]
    return np.minimum(fx.counts[nb].astype(np.int64), U16).sum(0)


def wrapped_total(fx, r):
    """incl + excl of row r modulo 2^16: what a 16-bit half holds after tier 1"""
    nb = fx.col[fx.row_ptr[r]:fx.row_ptr[r + 1]]
    return (fx.counts[nb].astype(np.int64).sum(0) + fx.counts[r]) % (1 << 16)
