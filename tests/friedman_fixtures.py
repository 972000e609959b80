"""Inputs and bars the Friedman / Page suites share (helper module, no tests in here): matched column sets, the row kinds of
the issue mixed in one table on the 3-decimal grid, off it and mixed, the shapes, the comparison of a result with the
referee's (tests/friedman_referee.py) and the resident call."""
import numpy as np

import friedman_referee as FR
from rank_support import P_FLOOR, P_RTOL, assert_same_bits, bits

KS = (2, 3, 4, 5, 8, 63, 64)
MS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
WAVE_MAX = 1024                     # default of friedman.wave_max: staged values (k x m rounded up to a power of two) of a wave's row
KNOB_VALUES = (0, 1, 64, 1024, 4096, 16384, 32768)
FLAVOURS = ("grid", "off", "mixed")
TEST_OUTS = {"friedman": ("tested", "p", "q", "w", "blocks", "med", "mean", "delta"),
             "page": ("tested", "p", "z", "l", "blocks", "med", "mean", "delta")}
FLT_MAX = np.finfo(np.float32).max


def staged(k, m):
    """the planner's measure of a row: k x (m rounded up to a power of two, 2 at least)"""
    pm = 2
    while pm < m:
        pm *= 2
    return k * pm


def boundary_ms(k):
    """the m on both sides of every step of staged(k, m) across WAVE_MAX (the wave form / the workgroup form)"""
    return sorted({m for pm in (2, 4, 8, 16, 32, 64, 128, 256, 512) if k * pm <= WAVE_MAX < 2 * k * pm
                   for m in (pm - 1, pm, pm + 1) if k * m <= FR.MAX_N})


def shapes(k):
    """every m of the issue's list for k sets, the dispatch boundary, and the limits"""
    ms = {m for m in MS if k * m <= FR.MAX_N} | set(boundary_ms(k))
    if k in (2, 3, 4):
        ms.add(4096)
    return sorted(ms)


def draw_sets(rng, k, m, spare=3):
    """k matched sets of m columns of a shuffled table of k m + spare columns -> (int32 [k, m], s)"""
    s = k * m + spare
    return rng.permutation(s).astype(np.int32)[: k * m].reshape(k, m).copy(), s


def _values(rng, shape, flavour):
    g = (rng.integers(0, 1001, size=shape) / 1000.0).astype(np.float32)
    if flavour == "grid":
        return g
    o = (rng.random(shape) ** 2).astype(np.float32)
    o.reshape(-1)[rng.integers(0, o.size, o.size // 4)] = o.reshape(-1)[rng.integers(0, o.size, o.size // 4)]    # exact duplicates
    return o if flavour == "off" else np.where(rng.random(shape) < 0.5, g, o)


def _leave(rng, X, left):
    """a NaN in one set of every block but `left` of them"""
    k, m = X.shape
    for q in rng.permutation(m)[: max(m - left, 0)]:
        X[rng.integers(0, k), q] = np.nan
    return X


def _few(rng, k, m, flavour, count):
    return rng.choice(_values(rng, (64,), flavour)[:count], size=(k, m))


def _same_order(rng, k, m, flavour):
    """every block orders the sets the same way, without ties: W = 1, Q = m'(k - 1)"""
    pool = np.unique(_values(rng, (4 * k + 64,), flavour))
    while pool.size < k:
        pool = np.unique(np.concatenate([pool, _values(rng, (4 * k + 64,), flavour)]))
    order = rng.permutation(k)
    X = np.empty((k, m), np.float32)
    for q in range(m):
        X[order, q] = np.sort(rng.choice(pool, k, replace=False))
    return X


def _specials(rng, k, m, flavour):
    """signed zeros and subnormals anywhere; FLT_MAX once in set 0 and -FLT_MAX once in set 1 (a set's sum stays finite)"""
    tiny = np.array([1e-45, 3e-39], np.float32)
    pool = np.concatenate([[-0.0, 0.0, 1.0, 0.5], tiny, -tiny]).astype(np.float32)
    X = rng.choice(pool, size=(k, m))
    X[0, rng.integers(0, m)] = FLT_MAX
    X[1, rng.integers(0, m)] = -FLT_MAX
    return X


def _sprinkle(rng, X, share):
    X[rng.random(X.shape) < share] = np.nan
    return X


KINDS = (
    ("plain", lambda rng, k, m, f: _values(rng, (k, m), f)),
    ("two blocks left", lambda rng, k, m, f: _leave(rng, _values(rng, (k, m), f), 2)),
    ("three blocks left", lambda rng, k, m, f: _leave(rng, _values(rng, (k, m), f), 3)),
    ("no block left", lambda rng, k, m, f: _leave(rng, _values(rng, (k, m), f), 0)),
    ("a set of NaNs", lambda rng, k, m, f: np.where(np.arange(k)[:, None] == rng.integers(0, k), np.float32(np.nan),
                                                    _values(rng, (k, m), f))),
    ("blocks fully tied", lambda rng, k, m, f: np.repeat(_values(rng, (1, m), f), k, axis=0)),
    ("two values", lambda rng, k, m, f: _few(rng, k, m, f, 2)),
    ("three values", lambda rng, k, m, f: _few(rng, k, m, f, 3)),
    ("same order", _same_order),
    ("specials", _specials),
    ("NaNs sprinkled", lambda rng, k, m, f: _sprinkle(rng, _values(rng, (k, m), f), 0.5 / k)),
    ("heavy ties", lambda rng, k, m, f: _sprinkle(rng, np.round(_values(rng, (k, m), f) * 4) / np.float32(4), 0.1 / k)),
)
SAME_ORDER = [name for name, _ in KINDS].index("same order")


def table(rng, sets, s, turn=0):
    """one row of every kind, the flavours taking turns (turn: where they start) -> (ps float32 [len(KINDS), s], the kinds'
    names); the columns outside the sets hold values, too"""
    k, m = sets.shape
    ps = _values(rng, (len(KINDS), s), "mixed")
    for r, (_, make) in enumerate(KINDS):
        ps[r, sets.reshape(-1)] = np.asarray(make(rng, k, m, FLAVOURS[(r + turn) % 3]), np.float32).reshape(-1)
    return ps, [name for name, _ in KINDS]


# ------------------------------------------------------------------------------ bars
class Worst:
    """the worst figures seen, per band, over the checks of a test"""

    def __init__(self):
        self.rel, self.below, self.z_ulp, self.cells, self.under = 0.0, 0.0, 0.0, 0, 0

    def line(self, label):
        return (f"{label}: {self.cells} tested rows; p >= {P_FLOOR:g}: worst rel {self.rel:.3g}; p < {P_FLOOR:g}: {self.under} cells, "
                f"largest {self.below:.3g}; z: worst {self.z_ulp:.3g} ulp")


def check_p(p, p_ref, label, worst):
    """p of the tested rows against the referee's 50-digit values (rounded to float64): within P_RTOL where the referee's p
    is at or above P_FLOOR, below 2 * P_FLOOR under it, 0 past the float64 range"""
    ref = np.asarray(p_ref, np.float64)
    cell = ref >= P_FLOOR
    err = np.abs(p[cell] - ref[cell]) / ref[cell]
    worst.cells += p.size
    worst.under += int((~cell).sum())
    if err.size:
        worst.rel = max(worst.rel, float(err.max()))
    if (~cell).any():
        worst.below = max(worst.below, float(p[~cell].max()))
    assert not err.size or err.max() <= P_RTOL, (label, "p", float(err.max()))
    assert np.all(p[~cell] < 2 * P_FLOOR) and np.all(p[~cell] >= 0), (label, "p under the floor")
    assert np.all(p[ref == 0.0] == 0.0), (label, "p past the float64 range")


def check(test, got, ref, label, worst, skip=()):
    """every bar of the issue: tested, blocks, means, medians, delta, Q, W and L as bits; z within 2 ulp of the correctly
    rounded value; p by check_p; 0 in every slot of a row that is not tested -> the tested mask"""
    assert_same_bits(got["tested"], ref["tested"], (label, "tested"))
    t = ref["tested"].astype(bool)
    exact = {"friedman": ("blocks", "med", "mean", "delta", "q", "w"), "page": ("blocks", "med", "mean", "delta", "l")}[test]
    for name in exact:
        if name not in skip:
            assert_same_bits(got[name], ref[name], (label, name))
    for name in TEST_OUTS[test]:
        if name not in skip:
            assert not bits(np.asarray(got[name])[..., ~t]).any(), (label, name, "a slot of a row that is not tested")
    if test == "page":
        z, zr = got["z"][t], ref["z"][t]
        ulp = np.abs(z - zr) / np.spacing(np.abs(zr))
        if ulp.size:
            worst.z_ulp = max(worst.z_ulp, float(ulp.max()))
        assert np.all(ulp <= 2), (label, "z", float(ulp.max()))
        assert not np.signbit(z[zr == 0]).any() and np.all(np.sign(z) == np.sign(zr)), (label, "sign of z")
    check_p(got["p"][t], ref["p_" + test][t], label, worst)
    return t


# ------------------------------------------------------------------------------ the resident call
def resident(ctx, test, ps, sets, skip=(), fill=0xA5, d_ps=None):
    """<test>_resident on device copies of the table (or the given resident table) and the set-major columns; every output
    pre-filled with `fill` bytes; the fields of `skip` are absent (NULL) -> {field: host array}"""
    from splicedice_amd import engine
    k = len(sets)
    held = [] if d_ps is not None else [ctx.to_device(ps, np.float32)]
    d_ps = d_ps if d_ps is not None else held[0]
    d_cols = ctx.to_device(engine.friedman_columns(sets, d_ps.shape[1]), np.int32)
    out = {name: ctx.empty(sh, dt).memset(fill)
           for name, (sh, dt) in engine.field_shapes(engine.ROW_TESTS[test][0], d_ps.shape[0], k).items() if name not in skip}
    try:
        getattr(ctx, test + "_resident")(d_ps, d_cols, k, out)
        ctx.sync()
        return {name: a.to_host() for name, a in out.items()}
    finally:
        for a in (*held, d_cols, *out.values()):
            a.free()
