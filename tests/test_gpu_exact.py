"""sdice_ranksum_exact / sdice_signedrank_exact and compare_sample_sets --exact against the referee
(tests/exact_referee.py: scipy's rankdata, the subset-count recurrence in dicts of Python ints, one division).

Bars: `exact` equal to the referee's eligibility; p EQUAL AS FLOAT64 to the referee's on the eligible
rows; on every other row p, and on all rows tested, z, med1/2, mean1/2 and delta, bit for bit what sdice_ranksum /
sdice_signedrank return for the same call.

The rank-sum table has 20 + 20 selected columns and NaN patterns that give every kept pair (n1', n2') with 3 <= n1', n2'
and N <= 34, each as every kind of RS_KINDS; N = 33, 34 are the rows above the limit.  The signed-rank table has 34 pairs
and every n' = 0..34 as every kind of SR_KINDS.  The builders and their references are cached and shared with
tests/test_gpu_exact_sweeps.py.  Tests without the gpu mark check on the CPU that the tables are what they claim."""
import argparse
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_referee as ER  # noqa: E402
import rank_support as RS  # noqa: E402
import signedrank_referee as SR  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from rank_support import bits  # noqa: E402

gpu = pytest.mark.gpu

F32 = ("med1", "med2", "mean1", "mean2", "delta")
OUTS = ("tested", "p", "z") + F32 + ("exact",)
DTYPES = dict(tested=np.uint8, p=np.float64, z=np.float64, exact=np.uint8, **{k: np.float32 for k in F32})
RS_COLS = 20                          # selected columns per set of the rank-sum table
RS_KINDS = ("untied", "2 distinct values", "3 distinct values", "all equal", "separated, set 1 low", "separated, set 1 high",
            "grid", "off-grid", "signed zeros", "an infinity", "subnormals")
SR_PAIRS = 34
SR_KINDS = ("grid", "off-grid", "2 distinct |d|", "equal printed differences", "all positive", "all negative",
            "signed zeros", "an infinity", "subnormal differences")
TINY = np.float32(1e-45)              # the smallest subnormal, 2^-149


# ---------------------------------------------------------------- the rank-sum table
def rs_values(rng, kind, n1, n2):
    """the kept values of the two sets, float32"""
    n = n1 + n2
    name = RS_KINDS[kind]
    if name == "untied":
        v = rng.permutation(1001)[:n] / 1000.0
    elif name.endswith("distinct values"):
        v = rng.integers(0, int(name[0]), size=n) / 4.0
    elif name == "all equal":
        v = np.full(n, rng.integers(0, 1001) / 1000.0)
    elif name.startswith("separated"):
        v = np.sort(rng.permutation(1001)[:n]) / 1000.0
        if name.endswith("high"):
            v = np.concatenate([v[n2:], v[:n2]])
    elif name == "grid":
        v = rng.integers(0, 41, size=n) / 1000.0
    elif name == "off-grid":
        v = rng.random(n) * 3.0 - 1.0
        v[rng.integers(0, n, size=2)] = v[rng.integers(0, n, size=2)]
    elif name == "signed zeros":
        v = rng.choice(np.array([-0.0, 0.0, 0.001, -0.001, 0.25]), size=n)
        v[rng.permutation(n)[:2]] = [-0.0, 0.0]
    elif name == "an infinity":
        v = rng.permutation(1001)[:n] / 1000.0
        where, sign = rng.permutation(n)[:2], rng.choice([-1.0, 1.0])
        v[where[0]] = sign * np.inf
        if n > 8:
            v[where[1]] = -sign * np.inf
    else:
        return (rng.integers(-4, 5, size=n).astype(np.float32) * TINY)[:n1], \
               (rng.integers(-4, 5, size=n).astype(np.float32) * TINY)[:n2]
    v = v.astype(np.float32)
    return v[:n1], v[n1:]


def rs_pairs():
    return [(a, b) for a in range(3, RS_COLS + 1) for b in range(3, RS_COLS + 1) if a + b <= 34]


@functools.lru_cache(maxsize=None)
def rs_table():
    """-> (ps float32 [rows, 43], g1, g2, kept pair [rows, 2], kind [rows]); shuffled columns, 3 spare ones"""
    rng = np.random.default_rng(3216)
    s = 2 * RS_COLS + 3
    perm = rng.permutation(s).astype(np.int32)
    g1, g2 = np.sort(perm[:RS_COLS]), np.sort(perm[RS_COLS: 2 * RS_COLS])
    rows, pairs, kinds = [], [], []
    for n1, n2 in rs_pairs():
        for kind in range(len(RS_KINDS)):
            x, y = rs_values(rng, kind, n1, n2)
            row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)     # would show if a spare column were read
            row[g1], row[g2] = np.nan, np.nan
            row[rng.permutation(g1)[:n1]] = x
            row[rng.permutation(g2)[:n2]] = y
            rows.append(row)
            pairs.append((n1, n2))
            kinds.append(kind)
    order = rng.permutation(len(rows))               # neighbouring rows differ in size and kind
    ps = np.ascontiguousarray(np.stack(rows)[order])
    ps.setflags(write=False)
    return ps, g1, g2, np.array(pairs)[order], np.array(kinds)[order]


@functools.lru_cache(maxsize=None)
def rs_reference():
    ps, g1, g2, _, _ = rs_table()
    return ER.table_reference(ps, g1, g2, paired=False)


# ---------------------------------------------------------------- the signed-rank table
def sr_values(rng, kind, n_prime, zeros):
    """the two sides of the kept pairs: n_prime non-zero differences and `zeros` equal pairs, float32"""
    m = n_prime + zeros
    name = SR_KINDS[kind]
    f = np.float32
    if name == "grid":
        ky = rng.integers(100, 901, size=m)
        kx = ky + rng.choice([-1, 1], size=m) * rng.integers(1, 31, size=m)
        x, y = (kx / 1000.0).astype(f), (ky / 1000.0).astype(f)
    elif name == "off-grid":
        y = (rng.random(m) * 2.0 - 0.5).astype(f)
        x = y + ((rng.random(m) + 0.01) * rng.choice([-1, 1], size=m)).astype(f)
    elif name == "2 distinct |d|":
        y = rng.integers(2, 40, size=m).astype(f)
        x = y + (rng.choice([0.5, 1.5], size=m) * rng.choice([-1, 1], size=m)).astype(f)
    elif name == "equal printed differences":
        ky = rng.integers(1, 10, size=m) * 100
        kx = ky + rng.choice([-100, 100], size=m)        # 0.3 - 0.2 against 0.2 - 0.1: one tie group on a grid row
        x, y = (kx / 1000.0).astype(f), (ky / 1000.0).astype(f)
    elif name in ("all positive", "all negative"):
        lo = np.sort(rng.permutation(1001)[: 2 * m]) / 1000.0
        a, b = lo[m:].astype(f), lo[:m].astype(f)
        a = a[rng.permutation(m)]
        x, y = (a, b) if name == "all positive" else (b, a)
    elif name == "signed zeros":
        x = rng.choice(np.array([-0.0, 0.0, 0.5, 0.25], f), size=m)
        y = rng.choice(np.array([-0.0, 0.0, 0.125], f), size=m)
        same = x == y
        y[same] = f(0.75)
        x[same] = rng.choice(np.array([-0.0, 0.0], f), size=int(same.sum()))
    elif name == "an infinity":
        y = (rng.random(m) * 2.0 - 0.5).astype(f)
        x = y + ((rng.random(m) + 0.01) * rng.choice([-1, 1], size=m)).astype(f)
        if m:
            x[rng.integers(0, m)] = rng.choice(np.array([-np.inf, np.inf], f))
    else:
        y = rng.integers(-3000, 3001, size=m).astype(f) * TINY
        x = y + (rng.integers(1, 6, size=m) * rng.choice([-1, 1], size=m)).astype(f) * TINY
    if zeros:
        z = rng.permutation(m)[:zeros]
        x[z] = y[z]
        if name == "signed zeros":
            x[z], y[z] = f(-0.0), f(0.0)                 # -0.0 - +0.0 is a zero difference
    return x, y


@functools.lru_cache(maxsize=None)
def sr_table():
    """-> (ps float32 [rows, 71], a, b, n' [rows], kind [rows]): every n' = 0..34 as every kind, the other pairs equal or
    dropped by a NaN on either side"""
    rng = np.random.default_rng(3431)
    a, b, s = RS.draw_pairs(rng, SR_PAIRS)
    rows, nps, kinds = [], [], []
    for n_prime in range(SR_PAIRS + 1):
        for kind in range(len(SR_KINDS)):
            kept = int(rng.integers(max(n_prime, 3), SR_PAIRS + 1))
            x, y = sr_values(rng, kind, n_prime, kept - n_prime)
            row = rng.choice(np.array([np.nan, 1e30, -7.0, 0.12345], np.float32), size=s)
            slots = rng.permutation(SR_PAIRS)
            live, gone = slots[:kept], slots[kept:]
            row[a[live]], row[b[live]] = x, y
            side = rng.integers(0, 3, size=gone.size)
            row[a[gone]] = np.where(side != 1, np.nan, 0.5).astype(np.float32)
            row[b[gone]] = np.where(side != 0, np.nan, 0.5).astype(np.float32)
            rows.append(row)
            nps.append(n_prime)
            kinds.append(kind)
    order = rng.permutation(len(rows))
    ps = np.ascontiguousarray(np.stack(rows)[order])
    ps.setflags(write=False)
    return ps, a, b, np.array(nps)[order], np.array(kinds)[order]


@functools.lru_cache(maxsize=None)
def sr_reference():
    ps, a, b, _, _ = sr_table()
    return ER.table_reference(ps, a, b, paired=True)


# ---------------------------------------------------------------- the bars
def check(got, base, ref, label):
    """got: the _exact call; base: the plain call on the same arguments; ref: (exact, p) of the referee"""
    exact, p = ref
    assert np.array_equal(got["exact"], exact), (label, np.flatnonzero(got["exact"] != exact)[:5])
    for name in ("tested", "z") + F32:
        bad = np.flatnonzero(bits(got[name]) != bits(base[name]))
        assert bad.size == 0, (label, name, bad[:5], got[name][bad[:5]], base[name][bad[:5]])
    assert not exact[base["tested"] == 0].any(), label
    on = exact == 1
    bad = np.flatnonzero(bits(got["p"][~on]) != bits(base["p"][~on]))
    assert bad.size == 0, (label, "asymptotic p", bad[:5])
    bad = np.flatnonzero(got["p"][on] != p[on])
    worst = float(np.max(np.abs(got["p"][on] - p[on]) / p[on])) if on.any() else 0.0
    print(f"{label}: rows {exact.size} tested {int(base['tested'].sum())} exact {int(on.sum())} "
          f"p unequal {bad.size} worst rel {worst:.3g} smallest exact p {p[on].min() if on.any() else 1:.3g}")
    assert bad.size == 0, (label, "exact p", np.flatnonzero(on)[bad[:5]], got["p"][on][bad[:5]], p[on][bad[:5]])


# ---------------------------------------------------------------- the tables, on the CPU
def test_rank_sum_table_is_what_it_claims():
    ps, g1, g2, pair, kind = rs_table()
    exact, p = rs_reference()
    assert ps.shape == (len(rs_pairs()) * len(RS_KINDS), 43) and len(rs_pairs()) == 303
    assert not np.intersect1d(g1, g2).size and (np.diff(g1) > 1).any()
    x, y = ps[:, g1], ps[:, g2]
    assert np.array_equal((~np.isnan(x)).sum(1), pair[:, 0]) and np.array_equal((~np.isnan(y)).sum(1), pair[:, 1])
    n_kept = pair.sum(1)
    assert np.array_equal(exact == 1, n_kept <= 32) and (n_kept >= 33).sum() == 15 * len(RS_KINDS)
    assert {(int(a), int(b)) for a, b in pair[kind == 0]} == set(rs_pairs())
    with np.errstate(invalid="ignore"):
        for r in range(ps.shape[0]):
            name = RS_KINDS[kind[r]]
            v = np.concatenate([x[r][~np.isnan(x[r])], y[r][~np.isnan(y[r])]])
            distinct = np.unique(v).size
            if name in ("untied", "an infinity") or name.startswith("separated"):
                assert distinct == v.size
            if name.endswith("distinct values"):
                assert distinct <= int(name[0])
            if name == "all equal":
                assert distinct == 1 and (exact[r] == 0 or p[r] == 1.0)
            if name.startswith("separated") and exact[r]:
                assert p[r] == 2 / math.comb(int(pair[r].sum()), int(pair[r].min()))       # the two edges of the sum range
            if name == "grid":
                assert SR.grid_keys(v) is not None
            if name == "off-grid":
                assert SR.grid_keys(v) is None
            if name == "signed zeros":
                assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
            if name == "an infinity":
                assert np.isinf(v).any()
            if name == "subnormals":
                assert (np.abs(v) < np.finfo(np.float32).tiny).all() and distinct >= 3
    assert p[exact == 1].min() == 2 / 601_080_390          # 16 v 16 separated


def test_signed_rank_table_is_what_it_claims():
    ps, a, b, n_prime, kind = sr_table()
    exact, p = sr_reference()
    ref = SR.table_reference(ps, a, b)
    assert ps.shape == (35 * len(SR_KINDS), 2 * SR_PAIRS + 3) and ref["tested"].all()
    assert np.array_equal(ref["npairs"], n_prime)
    assert np.array_equal(exact == 1, n_prime <= 31) and (p[n_prime == 0] == 1.0).all()
    for name in ("grid", "equal printed differences"):
        assert ref["grid"][kind == SR_KINDS.index(name)].all()
    for name in ("off-grid", "subnormal differences", "an infinity"):
        assert not ref["grid"][(kind == SR_KINDS.index(name)) & (n_prime > 0)].any()
    one_sided = (kind == SR_KINDS.index("all positive")) | (kind == SR_KINDS.index("all negative"))
    sel = one_sided & (n_prime >= 1) & (n_prime <= 31)
    assert np.array_equal(p[sel], 2.0 / 2.0 ** n_prime[sel])
    # 0.3 - 0.2 against 0.2 - 0.1: float32 differences would not tie, the rule's do -- p is that of n' equal ranks
    tie = np.flatnonzero((kind == SR_KINDS.index("equal printed differences")) & (n_prime >= 3) & (n_prime <= 31))
    x, y = ps[:, a], ps[:, b]
    with np.errstate(invalid="ignore"):
        assert any(np.unique(np.abs((x[r] - y[r])[(x[r] - y[r]) != 0])).size > 1 for r in tie)
    for r in tie:
        d = (x[r] - y[r])[~np.isnan(x[r] - y[r])]
        pos, n = int((d > 0).sum()), int(n_prime[r])
        assert p[r] == sum(math.comb(n, j) for j in range(n + 1) if abs(2 * j - n) >= abs(2 * pos - n)) / 2 ** n
    assert p[exact == 1].min() == 2.0 / 2.0 ** 31


# ---------------------------------------------------------------- the library
@gpu
def test_rank_sum_every_kept_pair_and_kind(ctx):
    """test 1 of the issue: every (n1', n2') with N <= 34 as every kind; N = 33, 34 keep the asymptotic p"""
    ps, g1, g2, _, _ = rs_table()
    check(ctx.ranksum_exact(ps, g1, g2), ctx.ranksum(ps, g1, g2), rs_reference(), "rank-sum 20 v 20")


@gpu
def test_signed_rank_every_count_and_kind(ctx):
    """test 2 of the issue: every n' = 0..34 as every kind; n' = 32..34 keep the asymptotic p, n' = 0 is exact with p = 1"""
    ps, a, b, _, _ = sr_table()
    check(ctx.signedrank_exact(ps, a, b), ctx.signedrank(ps, a, b), sr_reference(), "signed-rank 34 pairs")


@gpu
def test_three_against_three_separated_is_a_tenth(ctx):
    ps = np.array([[0.1, 0.2, 0.3, 0.7, 0.8, 0.9], [0.9, 0.8, 0.7, 0.1, 0.2, 0.3], [0.5] * 6], np.float32)
    got, base = ctx.ranksum_exact(ps, [0, 1, 2], [3, 4, 5]), ctx.ranksum(ps, [0, 1, 2], [3, 4, 5])
    assert got["p"].tolist() == [0.1, 0.1, 1.0] and got["exact"].tolist() == [1, 1, 1]
    assert abs(base["p"][0] - 0.0495) < 1e-4
    got = ctx.signedrank_exact(ps, [0, 1, 2], [3, 4, 5])
    assert got["p"].tolist() == [0.25, 0.25, 1.0] and got["exact"].tolist() == [1, 1, 1]
    for m in (1, 2):                                    # nothing can be tested: every output 0
        for out in (ctx.ranksum_exact(ps, np.arange(m), [3, 4, 5]), ctx.signedrank_exact(ps, np.arange(m), np.arange(3, 3 + m))):
            assert not any(out[name].any() for name in OUTS)
    assert all(v.shape == (0,) for v in ctx.ranksum_exact(np.zeros((0, 6), np.float32), [0, 1, 2], [3, 4, 5]).values())


def _device_call(ctx, paired, ps, c1, c2):
    from splicedice_amd import _cli
    from splicedice_amd.engine import RANKSUM_EXACT_FIELDS, field_shapes
    call = ctx.signedrank_exact_dev if paired else ctx.ranksum_exact_dev
    return _cli.device_call(ctx, dict(ps=(ps, np.float32), c1=(c1, np.int32), c2=(c2, np.int32)),
                            field_shapes(RANKSUM_EXACT_FIELDS, ps.shape[0]), lambda d, out: call(d["ps"], d["c1"], d["c2"], out))


@gpu
@pytest.mark.parametrize("paired", [False, True])
def test_host_and_dev_entry_points_agree(ctx, paired):
    """test 5 of the issue, first half"""
    ps, c1, c2, _, _ = sr_table() if paired else rs_table()
    host = (ctx.signedrank_exact if paired else ctx.ranksum_exact)(ps, c1, c2)
    dev = _device_call(ctx, paired, ps, c1, c2)
    assert set(host) == set(dev) == set(OUTS)
    for name in OUTS:
        assert np.array_equal(bits(host[name]), bits(dev[name])), name


def _raw_call(ctx, paired, exact, ps, c1, c2, n1, n2, outs):
    symbol = ("sdice_signedrank" if paired else "sdice_ranksum") + ("_exact" if exact else "")
    return RS.raw_call(ctx, symbol, ps, (c1, c2, n1) if paired else (c1, n1, c2, n2), outs, OUTS if exact else OUTS[:-1])


REFUSALS = [(False, "g1 index out of range"), (False, "g2 negative index"), (False, "negative group size"),
            (False, "group over the limit"), (True, "m=0"), (True, "m over the limit"), (True, "index out of range"),
            (True, "negative index"), (True, "twice in one list"), (True, "in both lists")]


@gpu
@pytest.mark.parametrize("paired,case", REFUSALS)
def test_refusals_leave_every_output_untouched(ctx, paired, case):
    """test 5 of the issue, second half: every refusal of sdice_ranksum / sdice_signedrank, `exact` included"""
    n, s = 3, 12
    c1, c2 = np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7])
    n1 = n2 = 4
    if case in ("g1 index out of range", "index out of range"):
        (c1 if not paired else c2)[3] = s
    elif case in ("g2 negative index", "negative index"):
        (c2 if not paired else c1)[0] = -1
    elif case == "negative group size":
        n2 = -1
    elif case == "group over the limit":
        n1, s = 4097, 4200
        c1, c2 = np.arange(n1), np.arange(4100, 4104)
    elif case == "m=0":
        n1 = 0
    elif case == "m over the limit":
        n1, s = 4097, 2 * 4097 + 2
        c1, c2 = np.arange(n1), np.arange(n1, 2 * n1)
    elif case == "twice in one list":
        c1[3] = c1[1]
    else:
        c2[2] = c1[0]
    ps = np.full((n, s), 0.5, dtype=np.float32)
    outs = {name: np.full(n, 7 + i, DTYPES[name]) for i, name in enumerate(OUTS)}
    before = {x: v.copy() for x, v in outs.items()}
    rc = _raw_call(ctx, paired, True, ps, c1, c2, n1, n2, outs)
    assert rc == -1, case                                   # SDICE_ERR_ARG
    assert ctx.lib.sdice_last_error()
    for x in outs:
        assert np.array_equal(outs[x], before[x]), (case, x)
    # the plain call refuses the same arguments
    plain = {x: v.copy() for x, v in before.items() if x != "exact"}
    assert _raw_call(ctx, paired, False, ps, c1, c2, n1, n2, plain) == -1
    ok = ctx.ranksum_exact(np.tile(np.array([0.1, 0.2, 0.3, 0.3, 0.1, 0.2], np.float32), (2, 1)), [0, 1, 2], [3, 4, 5])
    assert ok["tested"].tolist() == [1, 1] and ok["exact"].tolist() == [1, 1]       # the context still works


@gpu
def test_engine_refuses_pair_lists_of_two_lengths(ctx):
    with pytest.raises(ValueError, match="one length"):
        ctx.signedrank_exact(np.zeros((2, 9), np.float32), [0, 1, 2], [3, 4])


# ---------------------------------------------------------------- command line
def _referee_table(names, matrix, c1, c2, paired, anno):
    """the table the command must write, from the referees: float32 cells by numpy, p from the exact referee (every row of
    6 v 6 or 6 pairs is eligible), BH from the oracle over the tested rows, cells as numpy str()"""
    from splicedice_amd import compare_sample_sets as css
    if paired:
        ref = SR.table_reference(matrix, c1, c2)
    else:
        ref = {k: np.zeros(matrix.shape[0], dt) for k, dt in SR.FIELDS}
        for r in range(matrix.shape[0]):
            x, y = matrix[r, c1], matrix[r, c2]
            x, y = x[~np.isnan(x)], y[~np.isnan(y)]
            if x.size >= 3 and y.size >= 3:
                ref["tested"][r] = 1
                ref["mean1"][r], ref["mean2"][r], ref["med1"][r], ref["med2"][r] = np.mean(x), np.mean(y), np.median(x), np.median(y)
                ref["delta"][r] = np.float32(np.median(x) - np.median(y))
    exact, p = ER.table_reference(matrix, c1, c2, paired)
    keep = np.flatnonzero(ref["tested"])
    assert exact[keep].all() and not exact[ref["tested"] == 0].any()
    q = O.bh_fdr(p[keep])
    sfx = css.annotation_suffixes([names[r] for r in keep], anno) if anno else [""] * keep.size
    lines = ["event\tmean1\tmean2\tmedian1\tmedian2\tdelta\tp-value\tcorrected" + ("\tgene\toverlapping\ttranscript_id" if anno else "")]
    for i, r in enumerate(keep):
        cells = [ref["mean1"][r], ref["mean2"][r], ref["med1"][r], ref["med2"][r], ref["delta"][r], np.float64(p[r]), np.float64(q[i])]
        lines.append("\t".join([names[r]] + [str(c) for c in cells]) + sfx[i])
    return "\n".join(lines) + "\n", keep


@gpu
@pytest.mark.parametrize("gtf", [False, True])
@pytest.mark.parametrize("paired", [False, True])
def test_cli_exact_byte_for_byte(ctx, golden_dir, tmp_path, paired, gtf):
    """test 6 of the issue: --exact and --paired --exact, with and without -a, on the 40-row table of the --paired test;
    the file equals the referee's table byte for byte"""
    from splicedice_amd import compare_sample_sets as css
    table_path, m1, m2, names, matrix, a, b = RS.write_paired_cli_inputs(tmp_path)
    out = str(tmp_path / "out.tsv")
    anno = os.path.join(golden_dir, "compare", "anno.gtf") if gtf else ""
    css.run_with(argparse.Namespace(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=paired,
                                    exact=True, annotation=anno, outputFile=out), ctx=ctx)
    c1, c2 = (a, b) if paired else (np.sort(a), np.sort(b))      # the unpaired test takes the columns in table order
    want, keep = _referee_table(names, matrix, c1, c2, paired, anno)
    assert 30 <= keep.size <= 40
    got = open(out).read()
    diff = [(g, w) for g, w in zip(got.split("\n"), want.split("\n")) if g != w]
    print(f"paired={paired} gtf={gtf}: lines that differ {len(diff)} of {want.count(chr(10))}")
    for g, w in diff[:5]:
        print("got ", g, "\nwant", w)
    assert got == want
    # and the flag changed the p-values: the same run without it
    plain = str(tmp_path / "plain.tsv")
    css.run_with(argparse.Namespace(psiSPLICEDICE=table_path, manifest1=m1, manifest2=m2, moreManifests=None, paired=paired,
                                    exact=False, annotation=anno, outputFile=plain), ctx=ctx)
    rows = [(g.split("\t"), w.split("\t")) for g, w in zip(got.split("\n")[1:-1], open(plain).read().split("\n")[1:-1])]
    assert all(g[:6] == w[:6] and g[8:] == w[8:] for g, w in rows) and any(g[6] != w[6] for g, w in rows)


def _run_golden_without_the_flag(ctx, golden_dir, tmp_path):
    """-> (the bytes of the golden two-set run with `exact` absent and with exact=False, the golden file's bytes)"""
    from splicedice_amd import compare_sample_sets as css
    d = os.path.join(golden_dir, "compare")
    outs = []
    for extra in ({}, dict(paired=False, exact=False, moreManifests=None)):
        outs.append(str(tmp_path / f"cmp{len(outs)}.tsv"))
        css.run_with(argparse.Namespace(psiSPLICEDICE=os.path.join(d, "in_allPS.tsv"), manifest1=os.path.join(d, "m1.tsv"),
                                        manifest2=os.path.join(d, "m2.tsv"), annotation="", outputFile=outs[-1], **extra), ctx=ctx)
    return [open(o, "rb").read() for o in outs], open(os.path.join(d, "expected_out.tsv"), "rb").read()


@gpu
def test_cli_without_the_flag_is_unchanged(ctx, golden_dir, tmp_path):
    """the golden two-set run with `exact` absent and with exact=False: the same bytes, and the golden's cells by the rule
    of tests/test_gpu_cli.py (float32 cells as strings, p-value and corrected to 1e-6 relative)"""
    (absent, false), want = _run_golden_without_the_flag(ctx, golden_dir, tmp_path)
    assert absent == false
    got = [ln.split("\t") for ln in false.decode().rstrip("\n").split("\n")]
    want = [ln.split("\t") for ln in want.decode().rstrip("\n").split("\n")]
    assert len(got) == len(want) and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert g[:6] == w[:6]
        np.testing.assert_allclose([float(x) for x in g[6:]], [float(x) for x in w[6:]], rtol=1e-6)


@gpu
def test_cli_without_the_flag_is_the_golden_file_byte_for_byte(ctx, golden_dir, tmp_path):
    """the same run, every byte, against tests/golden/compare/expected_out_device.tsv: what the command wrote for these
    inputs on an MI355X on the commit before --exact existed (its own compare_sample_sets.py, the same kernels).

    The older golden file of this run, expected_out.tsv, cannot serve for a comparison of bytes: it holds scipy's p-values
    and statsmodels' BH of them, and the asymptotic path, which computes erfc and BH on the device, is an ulp or two
    beside them in 242 of its 297 lines (p-value or corrected only, worst relative difference 1.3e-15, every other cell
    equal) -- before --exact as well as after, which is why tests/test_gpu_cli.py holds that file to 1e-6 relative."""
    (absent, false), _ = _run_golden_without_the_flag(ctx, golden_dir, tmp_path)
    want = open(os.path.join(golden_dir, "compare", "expected_out_device.tsv"), "rb").read()
    lines = [(g, w) for g, w in zip(absent.split(b"\n"), want.split(b"\n")) if g != w]
    print(f"lines that differ from the recorded output: {len(lines)} of {want.count(10) - 1}", *lines[:3])
    assert absent == want and false == want
