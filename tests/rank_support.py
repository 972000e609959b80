"""What the per-row rank suites (rank-sum, Kruskal-Wallis, Jonckheere-Terpstra, signed-rank, Spearman, strata, --exact)
share (helper module, no tests in here): the bit view, the bars every suite holds p and the float32 fields to, the launch
rule of the rows-per-wave kernels restated, the NaN placements and value flavours of the count sweeps, column pairs, the
direct call of a C entry point and the writer of a command-line input table.

The bars of one statistic (H, z, rho) stay in that statistic's own test file.  Import rule: a support module or referee
imports no test module; a test module imports support modules and referees, and a `*_sweeps` file its own base file."""
import ctypes as C

import numpy as np

P_RTOL = 1e-9
P_FLOOR = 1e-280
N_LIMIT = 16384                     # selected columns per row the library supports (include/sdice.h)
NOMINAL_CUS = 256


# ------------------------------------------------------------------------------ bits and bars
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_f32(got, want):
    """bit-identical"""
    return np.asarray(got, np.float32).view(np.uint32) == np.asarray(want, np.float32).view(np.uint32)


def assert_same_bits(got, want, label, where=None):
    """every cell bit-identical; the message names the first rows (the last axis) that differ and where(rows) of them"""
    bad = np.argwhere(bits(got) != bits(want))
    rows = bad[:8, -1] if bad.size else bad
    assert bad.size == 0, (label, f"{len(bad)} cells differ", "rows", rows.tolist(), None if where is None else where(rows))


def check_common(got, ref, f32_fields, zero_fields, label, where=None):
    """tested mask equal, float32 fields bit-identical, zero fields all-zero bits on untested rows -> the tested mask"""
    bad = np.flatnonzero(got["tested"] != ref["tested"])
    assert bad.size == 0, (label, "tested", bad.size, bad[:5].tolist())
    t = ref["tested"].astype(bool)
    for name in f32_fields:
        assert got[name].dtype == np.float32, (label, name)
        assert_same_bits(got[name], ref[name], (label, name), where)
    for name in zero_fields:
        assert not bits(np.asarray(got[name])[..., ~t]).any(), (label, name, "a slot of a row that is not tested")
    return t


def check_p(p, p_ref, label, quiet=False):
    """p of the tested rows: within P_RTOL where the referee's p is at or above P_FLOOR, below 2 * P_FLOOR under it
    -> (cells below the floor, worst relative error at or above it); prints the figures before it asserts"""
    cell = p_ref >= P_FLOOR
    err = np.abs(p[cell] - p_ref[cell]) / p_ref[cell]
    below, worst = int((~cell).sum()), float(err.max()) if err.size else 0.0
    if not quiet:
        print(f"worst p rel {worst:.3g} smallest p {p_ref.min() if p_ref.size else 1:.3g} below floor {below}")
    assert worst <= P_RTOL, (label, "p", worst)
    assert np.all(p[~cell] < 2 * P_FLOOR), label
    return below, worst


def check_floor_share(tested, below, label):
    """cells under the p floor are at most 1 % of the tested rows, and there are tested rows"""
    assert tested > 0 and below <= 0.01 * tested, (label, tested, below)


# ------------------------------------------------------------------------------ the launch rule, restated
def rows_per_wave(n, compute_units):
    """rows_per_chunk of csrc/rowsum.h: the largest ch of 64, 32, .. 1 with ceil(n / ch) >= 2 * 32 * compute_units"""
    ch = 64
    while ch > 1 and -(-n // ch) < 2 * 32 * compute_units:
        ch >>= 1
    return ch


def chunk_table_rows(ch, compute_units):
    """the smallest n that selects ch, plus 37 rows (38 where 37 would fill the last chunk)"""
    n = 64 * compute_units * ch - (ch - 1)
    assert rows_per_wave(n, compute_units) == ch and (ch == 1 or rows_per_wave(n - 1, compute_units) == ch // 2)
    n += 37
    n += ch > 1 and n % ch == 0
    assert rows_per_wave(n, compute_units) == ch and (ch == 1 or n % ch)
    return n


def palette_index(n, rows):
    """row r takes palette row (r + 3 (r // 64)) mod rows: neighbours are of different kinds (the palettes interleave
    them) and what sits at a chunk's first and last position moves on from chunk to chunk"""
    r = np.arange(n, dtype=np.int64)
    return (r + 3 * (r // 64)) % rows


def scatter(ref, idx):
    return {name: np.ascontiguousarray(v[..., idx]) for name, v in ref.items()}


# ------------------------------------------------------------------------------ the grid and its off-grid twin
def on_grid(v):
    """the grid kernel's own question restated: is the value float32(key / 1000) of its clamped key (NaN: yes)"""
    kf = np.clip(np.rint(v * np.float32(1000.0)), 0.0, 1000.0)
    return np.isnan(v) | ((kf.astype(np.float64) / 1000.0).astype(np.float32) == v)


def twin(ps, cols):
    """the off-grid twin of a 3-decimal table: x -> x * float32(0.9) + float32(0.0123) in float32.  The map is strictly
    increasing over the 1001 grid values, so it keeps the order and the ties of every row; every row with a kept value
    among `cols` gets a value off the grid there, so the grid kernel hands the whole table to the sorting kernel."""
    grid = (np.arange(1001) / 1000.0).astype(np.float32)
    image = grid * np.float32(0.9) + np.float32(0.0123)
    assert image.dtype == np.float32 and np.all(np.diff(image) > 0)
    assert np.all(on_grid(ps[:, cols]))
    tw = ps * np.float32(0.9) + np.float32(0.0123)
    kept = ~np.isnan(ps[:, cols]).all(axis=1)
    assert np.all((~on_grid(tw[:, cols])).any(axis=1) == kept)
    return np.ascontiguousarray(tw)


# ------------------------------------------------------------------------------ fixtures of the count sweeps
PLACEMENTS = ("front", "back", "spread", "random")     # where a group's NaNs sit, in group (table) order


def _kept_positions(g, nv, how, rng):
    """positions (0..g-1, ascending) inside a group of g columns that keep a value; the others hold NaN"""
    if how == "front":
        return np.arange(g - nv, g)
    if how == "back":
        return np.arange(nv)
    if how == "spread":
        return np.round(np.linspace(0, g - 1, nv)).astype(np.int64)     # step >= 1: distinct
    return np.sort(rng.choice(g, nv, replace=False))


def _values(rng, k, flavour):
    if flavour == "q3":          # 3-decimal PS values: the counting kernel's input for groups of 65..1024
        return (rng.integers(0, 1001, size=k) / 1000.0).astype(np.float32)
    return (rng.random(k) ** 4).astype(np.float32)


def tree_sum(a, split8=True):
    """numpy's float32 pairwise_sum: a leaf of <= 128 values is numpy's own leaf (8 accumulators), above that
    n2 = n/2 - (n/2) % 8; split8=False drops the adjustment (a plausible wrong tree)"""
    n = a.size
    if n <= 128:
        return np.add.reduce(a)
    n2 = n // 2
    if split8:
        n2 -= n2 % 8
    return np.float32(tree_sum(a[:n2], split8) + tree_sum(a[n2:], split8))


def draw_pairs(rng, m, spare=3):
    """m disjoint column pairs of a shuffled table of 2 m + spare columns: a[q] lies before or after b[q] and the pairs
    are not in table order"""
    s = 2 * m + spare
    perm = rng.permutation(s).astype(np.int32)
    return perm[:m].copy(), perm[m: 2 * m].copy(), s


# ------------------------------------------------------------------------------ the C entry points, called directly
def raw_call(ctx, symbol, ps, args, outs, order):
    """ctx.lib.<symbol>(handle, n, s, ps, *args, *outputs in `order`): the table goes as float32, every list or array of
    `args` as int32, a scalar as it is; the outputs are the caller's host arrays, None goes as a NULL pointer"""
    ps = np.ascontiguousarray(ps, dtype=np.float32)
    held = [int(a) if np.isscalar(a) else np.ascontiguousarray(a, np.int32) for a in args]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    return getattr(ctx.lib, symbol)(ctx.h, *ps.shape, ptr(ps), *[a if isinstance(a, int) else ptr(a) for a in held],
                                    *[ptr(outs[x]) for x in order])


# ------------------------------------------------------------------------------ command-line inputs
def ps_names(n, s):
    """-> (the sample names of s columns, the event names of n rows)"""
    return [f"samp{j}" for j in range(s)], [f"chr1:{1000 + 10 * i}-{2000 + 10 * i}:+" for i in range(n)]


def write_ps_inputs(tmp_path, text, groups=()):
    """the PS table of the str cells text[n, s] as in_allPS.tsv and one manifest m<i>.tsv per (sample names, label) of
    `groups` -> (table path, manifest paths, event names)"""
    n, s = text.shape
    samples, names = ps_names(n, s)
    table = tmp_path / "in_allPS.tsv"
    with open(table, "w") as f:
        f.write("cluster\t" + "\t".join(samples) + "\n")
        for i in range(n):
            f.write(names[i] + "\t" + "\t".join(text[i]) + "\n")
    manifests = []
    for i, (group, label) in enumerate(groups):
        p = tmp_path / f"m{i + 1}.tsv"
        p.write_text("".join(f"{x}\tpath\tmeta\t{label}\n" for x in group))
        manifests.append(str(p))
    return str(table), manifests, names


def write_paired_cli_inputs(tmp_path):
    """40 rows x 6 pairs + 2 samples outside the manifests; the manifests' order is not the table's (the inputs of the
    --paired and of the --exact command-line tests)"""
    rng = np.random.default_rng(606)
    n, s = 40, 14
    samples, _ = ps_names(n, s)
    v = rng.integers(0, 1001, size=(n, s)) / 1000.0
    v[:, :6] = np.clip(v[:, 6:12] + 0.08 * rng.standard_normal((n, 6)) + 0.05, 0, 1)      # pairs (j, j + 6) move together
    v[:8] = np.round(v[:8] * 4) / 4                                                      # heavy ties, equal pairs
    text = np.where(rng.random((n, s)) < 0.08, "nan", np.char.mod("%.3f", v))
    text[8:11] = "0.500"                                                                  # all-equal rows stay in the table
    text[11:14, 0:4] = "nan"                                                              # two kept pairs: rows dropped
    order = [3, 0, 5, 1, 4, 2]
    path, (m1, m2), names = write_ps_inputs(tmp_path, text, [([samples[j] for j in order], "A"),
                                                             ([samples[j + 6] for j in order], "B")])
    matrix = text.astype(np.float64).astype(np.float32)
    return path, m1, m2, names, matrix, np.array(order, np.int32), np.array(order, np.int32) + 6
