"""PS kernels over the whole int32 count range (counts[n,s] int32, sdice.h): the fixtures of ps_count_fixtures.py --
every magnitude up to 2^31 - 1 alone and in sums, tiles on either side of the 2^24 bound between the 32-bit item and the
64-bit item with the deciding count in an own row, in either halo run and beyond the window, exclusion sums past 2^40,
the dense loci with a large count in every row -- through both kernels, vec 4 and vec 1, chunked tables, the device path
with and without reach words, the host entry point and `quant`.

Every comparison is bit for bit (NaN = NaN) against the integer oracle PC.oracle; what each fixture holds, and that a
32-bit path taken by mistake changes the bits of its show cells, is asserted without a GPU in
test_ps_count_fixtures_cpu.py.  Every launch runs with both outputs, excl alone and ps alone, ps.quantize3 0 and 1, on
outputs filled with 0xA5 (PC.Resident.check), and names the plan it ran (sdice_ps_last_plan) when it fails.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ps_count_fixtures as PC  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from oracle import oracle_quant_io as QIO  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = []                  # every plan that ran in this module (test_gpu_ps_plans.py adds them to its own record)


def _resident(ctx, fx):
    return PC.Resident(ctx, fx.counts, fx.row_ptr, fx.col, fx.want)


def _on_device_lists(ctx, junctions, fx):
    """cluster on the device: the lists are the context's own, reach words exist"""
    d = [ctx.to_device(x) for x in junctions]
    n = d[0].shape[0]
    d_row_of, d_rp = ctx.empty(n, np.int32), ctx.empty(n + 1, np.int64)
    d_col, nnz = ctx.cluster_dev(*d, d_row_of, d_rp, sync=True)
    assert np.array_equal(d_row_of.to_host(), np.arange(n)) and np.array_equal(d_rp.to_host(), fx.row_ptr)
    assert np.array_equal(d_col.to_host(), fx.col)
    return PC.Resident(ctx, fx.counts, fx.row_ptr, fx.col, fx.want, d_rp=d_rp, d_col=d_col)


# ------------------------------------------------------------------------------------------------ palette
@pytest.mark.parametrize("gen1", [0, 1])
@pytest.mark.parametrize("s,vec,chunks", [(8, 4, 1), (9, 1, 1), (260, 4, 3)])
def test_palette(ctx, s, vec, chunks, gen1):
    """every magnitude from 2^16 - 1 to 2^31 - 1 on a star of degree 40, lists given by the caller: vec 4, vec 1 (always
    the first-generation kernel) and a chunked table, both kernels"""
    res = _resident(ctx, PC.palette(s))
    kern = 2 if gen1 or vec == 1 else 0
    res.check({"ps.gen1": gen1}, {"kern": kern, "vec": vec, "n_chunks": chunks, "use_reach": 0}, SEEN, f"palette s={s}")
    res.check({"ps.gen1": gen1, "ps.tile_rows": 16}, {"kern": kern, "vec": vec, "tile_rows": 16, "n_tiles": 4}, SEEN,
              f"palette s={s}")


@pytest.mark.parametrize("s,vec", [(8, 4), (9, 1), (260, 4)])
def test_palette_on_the_context_lists(ctx, s, vec):
    """the same star clustered on the device: with reach words (register-staged kernel at vec 4), with ps.use_reach = 0,
    and through the first-generation kernel"""
    fx = PC.palette_on_device_lists(s)
    res = _on_device_lists(ctx, PC.palette_junctions(), fx)
    for rows in (0, 16):
        res.check({"ps.tile_rows": rows}, {"kern": 0 if vec == 4 else 2, "vec": vec, "use_reach": int(vec == 4)}, SEEN, f"s={s}")
        res.check({"ps.tile_rows": rows, "ps.use_reach": 0}, {"use_reach": 0}, SEEN, f"s={s}")
        res.check({"ps.tile_rows": rows, "ps.gen1": 1}, {"kern": 2, "use_reach": 0}, SEEN, f"s={s}")


def test_palette_through_the_host_entry_point(ctx):
    for s in (8, 9, 260):
        fx = PC.palette(s)
        ps, excl = ctx.ps(fx.counts, fx.row_ptr, fx.col, want_excl=True)
        assert PC.same_ps(ps, fx.want[0]) and excl.dtype == np.int64 and np.array_equal(excl, fx.want[1]), ctx.ps_last_plan()
        SEEN.append(ctx.ps_last_plan())
        assert np.array_equal(ctx.ps(fx.counts, fx.row_ptr, fx.col, want_excl=True, want_ps=False), fx.want[1])


# ------------------------------------------------------------------------------------------------ the 2^24 bound
@pytest.mark.parametrize("gen1", [0, 1])
@pytest.mark.parametrize("s,vec,chunks", [(8, 4, 1), (9, 1, 1), (260, 4, 3)])
def test_fast_slow_decision_from_both_sides(ctx, s, vec, chunks, gen1):
    """tiles of 128 rows whose (degree + 1) x largest count is 2^24 - 16 and 2^24 - 1 (32-bit item), 2^24, 2^24 + 1,
    2^24 + 2 and 2^24 + 33 (64-bit item), the deciding count in an own row, in a halo row on either side that rows of
    the tile list (the own rows alone would leave every item fast), or beyond the window (where it must not decide);
    one tile whose short rows are fast and whose long rows are not.  The show cells (odd totals above 2^24) get other
    bits from a float32 quotient: a bound one step too loose, or taken over the own rows alone, fails here."""
    fx = PC.bound(s)
    res = _resident(ctx, fx)
    kern = 2 if gen1 or vec == 1 else 0
    expect = {"kern": kern, "vec": vec, "tile_rows": PC.BOUND_R, "halo": PC.BOUND_HALO, "n_chunks": chunks,
              "n_tiles": fx.n // PC.BOUND_R, "use_reach": 0}
    # (160 KiB of LDS: at s = 260 a window of 128 + 2 x 16 rows of a 128-column chunk does not fit the default 80 KiB,
    # and the planner would cut the halo to 4 rows; the fixture's tiles are laid out for a halo of 16)
    res.check({"ps.gen1": gen1, "ps.tile_rows": PC.BOUND_R, "ps.lds_bytes": 160 * 1024}, expect, SEEN, f"bound s={s}")


# ------------------------------------------------------------------------------------------------ large sums
@pytest.mark.parametrize("gen1", [0, 1])
def test_large_sums(ctx, gen1):
    """lists of 600 and 3000 rows at 2^31 - 1 (sums past 2^40, list totals beyond the offset stage), 0 / 0, PS of exactly
    0 and 1, and the '.3f' ties k / 2000 from totals of 2000 x 2^20: one tile, and tiles of 64 rows"""
    res = _resident(ctx, PC.large_sums())
    for rows in (0, 64):
        res.check({"ps.gen1": gen1, "ps.tile_rows": rows}, {"kern": 2 if gen1 else 0, "vec": 4}, SEEN, "large sums")


# ------------------------------------------------------------------------------------------------ dense loci
@pytest.mark.parametrize("gen1", [0, 1])
@pytest.mark.parametrize("name", ["star", "hb"])
def test_dense_loci_with_64_bit_sums(ctx, name, gen1):
    """the "star" and "hb" loci of dense_loci_fixtures with a count of 2^24 or more in every row, on the context's own
    lists: the degree cutoff of the fast item (252 .. 256), list totals beyond the offset stage (col_in_lds false) and
    neighbours beyond the halo (reach 255 .. 257), each with 64-bit sums; reach words on and off"""
    fx = PC.dense(name)
    res = _on_device_lists(ctx, PC.DL.junctions(name), fx)
    for rows in (0, 256):
        for use_reach in (1, 0):
            res.check({"ps.gen1": gen1, "ps.tile_rows": rows, "ps.use_reach": use_reach},
                      {"kern": 2 if gen1 else 0, "vec": 4, "use_reach": int(use_reach and not gen1)}, SEEN, name)


# ------------------------------------------------------------------------------------------------ quant
CLI_SCORES = {            # junction -> scores in the three samples
    ("chr1", 1000, 9000, "+"): (PC.I31, PC.F24 + 1, 7),
    ("chr1", 1100, 1400, "+"): (PC.I31, PC.F24, 0),
    ("chr1", 2000, 2300, "+"): (PC.I31 - 1, 2 ** 30, 65536),
    ("chr1", 3000, 3300, "+"): (5, PC.F24 - 1, 65537),
    ("chr1", 4000, 4300, "+"): (PC.I31, 1, PC.I31),
    ("chr1", 9500, 9900, "+"): (12, 0, 9),
    ("chr2", 500, 900, "-"): (PC.I31, PC.I31, PC.I31),
    ("chr2", 600, 1000, "-"): (PC.I31, 0, PC.I31 - 1),
}


def test_quant_on_junction_files_with_scores_up_to_2_31(ctx, tmp_path):
    """`quant` on three bed files whose scores include 2^31 - 1: _inclusionCounts.tsv and _allPS.tsv equal the text that
    the oracle formats (reference parser restated in oracle_quant_io, clusters from oracle_np, the integer oracle)"""
    from splicedice_amd import quant
    rows = []
    for i in range(3):
        path = tmp_path / f"s{i}.bed"
        with open(path, "w") as fh:
            for (chrom, left, right, strand), scores in CLI_SCORES.items():
                fh.write(f"{chrom}\t{left}\t{right}\tj\t{scores[i]}\t{strand}\n")
        rows.append(f"s{i}\t{path}\tmeta\tA\n")
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("".join(rows))
    args = argparse.Namespace(manifest=str(manifest), output_prefix=str(tmp_path / "out"), maxLength=50000, minLength=50,
                              minOverhang=5, drim=False, noMultimap=False, filter="gtag_only", minUnique=5,
                              lowCoverageNan=False, minEntropy=1)
    with contextlib.redirect_stdout(io.StringIO()):
        quant.Quant(args.manifest, args.output_prefix, args, ctx=ctx)
    SEEN.append(ctx.ps_last_plan())

    samples = quant.parse_manifest(str(manifest))
    assert [x.type for x in samples] == ["bed"] * 3
    juncs = QIO.get_all_junctions(samples, args)
    assert juncs == set(CLI_SCORES)
    clusters = O.get_clusters(list(juncs))
    order = sorted(clusters)
    index = {j: i for i, j in enumerate(order)}
    counts, _ = QIO.get_junction_counts(samples, index, args)
    assert counts.max() == PC.I31
    row_ptr = np.concatenate([[0], np.cumsum([len(clusters[j]) for j in order])]).astype(np.int64)
    col = np.asarray([index[o] for j in order for o in clusters[j]], np.int32)
    ps, excl = PC.oracle(counts, row_ptr, col)
    assert excl.max() > 2 ** 32
    names = [f"{j[0]}:{j[1]}-{j[2]}:{j[3]}" for j in order]
    header = "cluster\ts0\ts1\ts2\n"
    want_counts = header + "".join(f"{nm}\t" + "\t".join(str(int(x)) for x in row) + "\n" for nm, row in zip(names, counts))
    want_ps = header + "".join(f"{nm}\t" + "\t".join(f"{x:.3f}" for x in row) + "\n" for nm, row in zip(names, ps))
    assert (tmp_path / "out_inclusionCounts.tsv").read_text() == want_counts
    assert (tmp_path / "out_allPS.tsv").read_text() == want_ps
