"""One GPU case for every path that the PS planner (psplan.cpp) can name: column chunks at every lv_shift of the
register-staged kernel and on the first-generation kernel, tables reached through pointers that are not 16-byte aligned,
rows too wide for 32-bit tile offsets, the XCD remap with and without idle workgroups, ps.prio and ps.nt_loads, reach
words, and the planner's refusal raised with a live context.

Every case reads back the plan that the launch used (sdice_ps_last_plan) and asserts the fields that define its path --
the expected values are written out by hand from psplan.cpp -- and which of the two kernels the context profile counted.
Results are compared bit for bit (NaN = NaN) with the integer oracle of ps_count_fixtures, with both outputs, excl
alone and ps alone, ps.quantize3 0 and 1, on outputs filled with 0xA5 (PC.Resident.check).  The tables are a few hundred
gene-shaped rows (synth.make_junctions) plus one pair of rows that list each other across the whole table, so the
global-memory path runs in every plan.  The last test asserts what the plans seen cover.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd.engine import Context, SdiceError  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = []                  # every plan that a launch of this module ran
N = 300                    # rows of the gene-shaped table; ps.tile_rows 32: ten tiles, the last one of 12 rows
ROWS = 32
LDS_REFUSAL = "row chunk does not fit LDS; lower ps.chunk_cols"


def _resident(ctx, n, s):
    fx = PC.gene_table(n, s)
    return PC.Resident(ctx, fx.counts, fx.row_ptr, fx.col, fx.want)


def test_no_plan_before_the_first_launch():
    own = Context(0)
    try:
        assert own.lib.sdice_ps_last_plan(own.h, None, 0, None) == -4          # SDICE_ERR_STATE
        with pytest.raises(SdiceError, match="no sdice_ps_dev launch yet"):
            own.ps_last_plan()
        assert own.lib.sdice_ps_last_plan(None, None, 0, None) == -1           # SDICE_ERR_ARG
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ column chunks
# (s, ps.chunk_cols) -> (chunk_cols, n_chunks, lv_shift): chunk_cols / 4 vectors per chunk row = 64 >> lv_shift
V3_CHUNKS = {
    (520, 4): (4, 130, 6), (520, 8): (8, 65, 5), (520, 16): (16, 33, 4), (520, 32): (32, 17, 3), (520, 64): (64, 9, 2),
    (520, 128): (128, 5, 1), (520, 256): (256, 3, 0),
    (260, 128): (128, 3, 1),              # a last chunk of 4 columns
    (516, 256): (256, 3, 0),              # a last chunk of one vector
}


@pytest.mark.parametrize("s,chunk", list(V3_CHUNKS))
def test_column_chunks_register_staged_kernel(ctx, s, chunk):
    cw, n_chunks, lv_shift = V3_CHUNKS[(s, chunk)]
    expect = {"kern": 0, "vec": 4, "chunk_cols": cw, "n_chunks": n_chunks, "lv_shift": lv_shift, "tile_rows": ROWS,
              "halo": 16, "n_tiles": 10, "nt": 0, "use_reach": 0, "tiles_per_xcd": 0, "threads": 1024}
    _resident(ctx, N, s).check({"ps.chunk_cols": chunk, "ps.tile_rows": ROWS}, expect, SEEN)


# (s, ps.chunk_cols or 0 for the default) -> the plan fields that define the path
GEN1_CHUNKS = {
    (520, 12): {"kern": 2, "vec": 4, "chunk_cols": 12, "n_chunks": 44},       # 3 vectors per chunk row: no divisor of 64
    (520, 100): {"kern": 2, "vec": 4, "chunk_cols": 100, "n_chunks": 6},      # 25 vectors
    (258, 0): {"kern": 2, "vec": 1, "chunk_cols": 128, "n_chunks": 3},        # rows that are no vectors: a tail of 2 columns
    (515, 0): {"kern": 2, "vec": 1, "chunk_cols": 128, "n_chunks": 5},        # ... of 3 columns
}


@pytest.mark.parametrize("s,chunk", list(GEN1_CHUNKS))
def test_column_chunks_first_generation_kernel(ctx, s, chunk):
    expect = {**GEN1_CHUNKS[(s, chunk)], "tile_rows": ROWS, "halo": 16, "n_tiles": 10, "nt": 0, "use_reach": 0}
    _resident(ctx, N, s).check({"ps.chunk_cols": chunk, "ps.tile_rows": ROWS}, expect, SEEN)


def test_chunk_wider_than_the_table_is_clamped(ctx):
    """ps.chunk_cols 1000 at s = 520: one chunk of 520 columns, which the register-staged kernel takes with 31 rows (4 T /
    130 vectors) and a halo of 3 (80 KiB of LDS)"""
    expect = {"kern": 0, "vec": 4, "chunk_cols": 520, "n_chunks": 1, "tile_rows": 31, "halo": 3, "n_tiles": 10, "nt": 1}
    _resident(ctx, N, 520).check({"ps.chunk_cols": 1000, "ps.tile_rows": ROWS}, expect, SEEN)


# ------------------------------------------------------------------------------------------------ misaligned views
PAD = 8                    # elements in front of and behind every view


def _views(ctx, res, off_counts, off_ps, off_excl):
    """the table and the outputs as views `off` elements into buffers with PAD spare elements on either side of a
    16-byte boundary; -> (d_counts, d_excl, d_ps views, the two output buffers, the buffer under d_counts)"""
    n, s = res.n, res.s
    fx_counts = res.d_counts.to_host()
    buf_c = ctx.empty(n * s + 2 * PAD, np.int32)
    buf_c.upload(np.concatenate([np.zeros(PAD + off_counts, np.int32), fx_counts.ravel(), np.zeros(PAD - off_counts, np.int32)]))
    buf_e, buf_p = ctx.empty(n * s + 2 * PAD, np.int64), ctx.empty(n * s + 2 * PAD, np.float32)
    for b in (buf_c, buf_e, buf_p):
        assert b.ptr % 16 == 0
    return (buf_c.offset(PAD + off_counts, (n, s)), buf_e.offset(PAD + off_excl, (n, s)), buf_p.offset(PAD + off_ps, (n, s)),
            buf_e, buf_p, buf_c)


MISALIGNED = [(k, 0, 0) for k in (1, 2, 3)] + [(0, k, 0) for k in (1, 2, 3)] + [(0, 0, k) for k in (1, 2, 3)] + \
             [(k, k, k) for k in (1, 2, 3)]


@pytest.mark.parametrize("s", [100, 256])
def test_views_that_are_not_16_byte_aligned(ctx, s):
    """d_counts, d_ps and d_excl in turn 1, 2 and 3 elements past a 16-byte boundary, then all three: the scalar
    first-generation kernel (vec 1, kern 2), results bit-identical to the aligned call, the elements on either side of
    each output view untouched.  What counts is the 16-byte boundary (ps.hip, f.aligned): an int64 view two elements in
    is aligned again, and an output that is not asked for does not count -- those launches keep vec 4."""
    res = _resident(ctx, N, s)
    aligned = {}
    for name, want_excl, want_ps in PC.OUTPUTS:
        for q3 in (0, 1):
            ps, excl, plan, ran = res.launch({"ps.tile_rows": ROWS, "ps.quantize3": q3}, want_excl, want_ps)
            assert (plan["kern"], plan["vec"]) == (0, 4) and ran == {"ps_tile_v3_kernel": 1, "ps_tile_kernel": 0}, plan
            aligned[(name, q3)] = (ps, excl)
    ps_want, excl_want, q_want = res.want
    assert PC.same_ps(aligned[("both", 0)][0], ps_want) and np.array_equal(aligned[("both", 0)][1], excl_want)
    assert PC.same_ps(aligned[("ps", 1)][0], q_want)
    for off_counts, off_ps, off_excl in MISALIGNED:
        d_counts, d_excl, d_ps, buf_e, buf_p, buf_c = _views(ctx, res, off_counts, off_ps, off_excl)
        for name, want_excl, want_ps in PC.OUTPUTS:
            for q3 in (0, 1):
                buf_e.memset(PC.FILL)
                buf_p.memset(PC.FILL)
                ps, excl, plan, ran = res.launch({"ps.tile_rows": ROWS, "ps.quantize3": q3}, want_excl, want_ps,
                                                 args=(d_counts, d_excl, d_ps))
                SEEN.append(plan)
                tag = f"offsets counts {off_counts} ps {off_ps} excl {off_excl} outputs={name} q3={q3} plan={plan} {ran}"
                off_16 = bool(off_counts % 4 or (want_ps and off_ps % 4) or (want_excl and off_excl % 2))
                assert (plan["kern"], plan["vec"]) == ((2, 1) if off_16 else (0, 4)), tag
                assert ran[PC.PS_KERNELS[plan["kern"]]] == 1 and sum(ran.values()) == 1, tag
                all_p, all_e = buf_p.to_host().view(np.uint32), buf_e.to_host().view(np.uint64)
                lo_p, lo_e = PAD + off_ps, PAD + off_excl
                assert (all_p[:lo_p] == 0xA5A5A5A5).all() and (all_p[lo_p + res.n * s:] == 0xA5A5A5A5).all(), tag
                assert (all_e[:lo_e] == 0xA5A5A5A5A5A5A5A5).all() and (all_e[lo_e + res.n * s:] == 0xA5A5A5A5A5A5A5A5).all(), tag
                if want_ps:
                    assert PC.same_ps(ps, aligned[(name, q3)][0]), tag
                else:
                    assert (all_p == 0xA5A5A5A5).all(), tag
                if want_excl:
                    assert np.array_equal(excl, aligned[(name, q3)][1]), tag
                else:
                    assert (all_e == 0xA5A5A5A5A5A5A5A5).all(), tag


# ------------------------------------------------------------------------------------------------ wide rows
@pytest.mark.parametrize("s,kern,n_chunks", [(524284, 0, 4096), (524288, 2, 4096), (524292, 2, 4097)])
def test_rows_too_wide_for_32_bit_tile_offsets(ctx, s, kern, n_chunks):
    """the register-staged kernel addresses a tile by 32-bit offsets and gives way at s x 2048 >= 2^30: s = 524 284 is
    its last width, 524 288 and 524 292 go to the first-generation kernel.  Six rows that all list each other; counts
    in the first, a middle and the last chunk, 0 / 0 everywhere else."""
    counts, row_ptr, col, ps, excl, _ = PC.wide(s)
    res = PC.Resident(ctx, counts, row_ptr, col, (ps, excl, O.quantize3_fast(ps)))
    expect = {"kern": kern, "vec": 4, "chunk_cols": 128, "n_chunks": n_chunks, "tile_rows": 6, "n_tiles": 1, "lv_shift": 1,
              "nt": 0, "tiles_per_xcd": 0}
    res.check({}, expect, SEEN, f"s={s}")


# ------------------------------------------------------------------------------------------------ XCD remap
@pytest.mark.parametrize("s,n_chunks", [(100, 1), (300, 3)])
@pytest.mark.parametrize("tiles", [63, 64, 65, 71, 72])
def test_xcd_remap(ctx, tiles, s, n_chunks):
    """ps.tile_rows 8: below 64 tiles no remap; from 64 on every XCD takes ceil(n_tiles / 8) consecutive tiles, and
    unless n_tiles is a multiple of 8 the last workgroups find no tile (65 tiles: 7 idle, 71: 1).  Same bits with
    ps.xcd_remap 0."""
    n = 8 * tiles - 3
    res = _resident(ctx, n, s)
    expect = {"kern": 0, "vec": 4, "tile_rows": 8, "n_tiles": tiles, "n_chunks": n_chunks, "halo": 16}
    per_xcd = 0 if tiles < 64 else -(-tiles // 8)
    assert per_xcd == {63: 0, 64: 8, 65: 9, 71: 9, 72: 9}[tiles]
    res.check({"ps.tile_rows": 8, "ps.xcd_remap": 1}, {**expect, "tiles_per_xcd": per_xcd}, SEEN, f"{tiles} tiles")
    res.check({"ps.tile_rows": 8, "ps.xcd_remap": 0}, {**expect, "tiles_per_xcd": 0}, SEEN, f"{tiles} tiles")
    res.check({"ps.tile_rows": 8, "ps.xcd_remap": 1, "ps.gen1": 1}, {**expect, "kern": 2, "tiles_per_xcd": per_xcd}, SEEN)


# ------------------------------------------------------------------------------------------------ prio, nt_loads
@pytest.mark.parametrize("gen1", [0, 1])
@pytest.mark.parametrize("s,n_chunks", [(100, 1), (300, 3)])
def test_prio_and_nt_loads(ctx, s, n_chunks, gen1):
    """wave priority and non-temporal window loads change no bit; nt is dropped whenever the table is chunked"""
    res = _resident(ctx, N, s)
    for prio in (0, 1):
        for nt in (0, 1):
            expect = {"kern": 2 if gen1 else 0, "n_chunks": n_chunks, "prio": prio, "nt": nt if n_chunks == 1 else 0}
            res.check({"ps.tile_rows": ROWS, "ps.prio": prio, "ps.nt_loads": nt, "ps.gen1": gen1}, expect, SEEN)


# ------------------------------------------------------------------------------------------------ reach words
@pytest.mark.parametrize("s,n_chunks", [(100, 1), (300, 3)])
def test_reach_words_of_the_context_lists(ctx, s, n_chunks):
    """gene-shaped junctions clustered on the device: the lists are the context's own and the planner sizes the halo runs
    from their reach words (capacity 32); ps.use_reach 0 and a copy of the lists go back to 16 rows on either side"""
    from splicedice_amd import synth
    n = 500
    junc = synth.make_junctions(n, 3)
    d = [ctx.to_device(x) for x in junc]
    d_row_of, d_rp = ctx.empty(n, np.int32), ctx.empty(n + 1, np.int64)
    d_col, nnz = ctx.cluster_dev(*d, d_row_of, d_rp, sync=True)
    row_ptr, col = d_rp.to_host(), d_col.to_host()
    want_csr = O.cluster_csr(*junc)
    assert np.array_equal(row_ptr, want_csr[1]) and np.array_equal(col, want_csr[2])
    counts = PC.gene_table(n, s).counts
    ps, excl = PC.oracle(counts, row_ptr, col)
    want = (ps, excl, O.quantize3_fast(ps))
    res = PC.Resident(ctx, counts, row_ptr, col, want, d_rp=d_rp, d_col=d_col)
    base = {"kern": 0, "vec": 4, "tile_rows": 64, "n_tiles": 8, "n_chunks": n_chunks}
    res.check({"ps.tile_rows": 64}, {**base, "use_reach": 1, "halo": 32}, SEEN)
    res.check({"ps.tile_rows": 64, "ps.use_reach": 0}, {**base, "use_reach": 0}, SEEN)
    copy = PC.Resident(ctx, counts, row_ptr, col, want)
    copy.check({"ps.tile_rows": 64}, {**base, "use_reach": 0, "halo": 16}, SEEN)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("lds", [0, 160 * 1024])
def test_chunk_that_fits_no_tile_is_refused(ctx, lds):
    """one chunk of 50 000 columns: a window of two rows is 400 KB, beyond the 160 KiB that ps.lds_bytes can ask for.
    SDICE_ERR_ARG with the planner's message, outputs untouched, and the context goes on working."""
    n, s = 20, 50000
    counts = np.full((n, s), 3, np.int32)
    row_ptr = np.arange(n + 1, dtype=np.int64)
    col = np.roll(np.arange(n, dtype=np.int32), 1)                # every row lists the one before it
    ps = np.full((n, s), 0.5, np.float32)
    res = PC.Resident(ctx, counts, row_ptr, col, (ps, np.full((n, s), 3, np.int64), ps))
    small = _resident(ctx, N, 100)
    small.check({"ps.tile_rows": ROWS}, {"kern": 0}, SEEN)
    before = ctx.ps_last_plan()
    knobs = {"ps.chunk_cols": 50000, **({"ps.lds_bytes": lds} if lds else {})}
    for gen1 in (0, 1):
        with ctx.params({**knobs, "ps.gen1": gen1}):
            res.d_ps.memset(PC.FILL)
            res.d_excl.memset(PC.FILL)
            status = ctx.lib.sdice_ps_dev(ctx.h, n, s, res.d_counts.ptr, res.d_rp.ptr, res.d_col.ptr, res.d_excl.ptr, res.d_ps.ptr)
            assert status == -1 and ctx.lib.sdice_last_error().decode() == "sdice_ps_dev: " + LDS_REFUSAL
            with pytest.raises(SdiceError, match=LDS_REFUSAL):
                ctx.ps_dev(res.d_counts, res.d_rp, res.d_col, res.d_excl, res.d_ps)
        assert (res.d_ps.to_host().view(np.uint32) == 0xA5A5A5A5).all()
        assert (res.d_excl.to_host().view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all()
        assert ctx.ps_last_plan() == before                      # a refused call leaves the plan of the launch before it
    small.check({"ps.tile_rows": ROWS}, {"kern": 0, "vec": 4}, SEEN)
    res.check({}, {"kern": 0, "chunk_cols": 128, "n_chunks": 391, "tile_rows": 20}, SEEN)       # the same table, default chunks


# ------------------------------------------------------------------------------------------------ coverage
def test_plans_seen_cover_the_plan_space():
    """over the launches of this module (and of test_gpu_ps_counts.py when it ran in the same session): both kernels, vec 4
    and 1, nt and use_reach on and off, remapped and plain grids, every lv_shift, chunked and unchunked tables"""
    seen = list(SEEN)
    counts_module = sys.modules.get("test_gpu_ps_counts")
    if counts_module is not None:
        seen += counts_module.SEEN
    assert len(seen) >= 100
    values = {key: {p[key] for p in seen} for key in Context.PS_PLAN_FIELDS}
    assert values["kern"] == {0, 2} and values["vec"] == {1, 4} and values["nt"] == {0, 1}, values
    assert values["use_reach"] == {0, 1} and values["prio"] == {0, 1} and values["q3"] == {0, 1}, values
    assert 0 in values["tiles_per_xcd"] and {8, 9} <= values["tiles_per_xcd"], values
    assert 1 in values["n_chunks"] and max(values["n_chunks"]) > 1, values
    v3_chunked = {p["lv_shift"] for p in seen if p["kern"] == 0 and p["n_chunks"] > 1}
    assert v3_chunked == set(range(7)), v3_chunked
    # both kernels ran chunked and unchunked, and the scalar kernel both ways too
    for kern in (0, 2):
        assert {p["n_chunks"] > 1 for p in seen if p["kern"] == kern} == {False, True}, kern
    assert {p["n_chunks"] > 1 for p in seen if p["vec"] == 1} == {False, True}
