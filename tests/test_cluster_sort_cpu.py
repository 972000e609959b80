"""Host-side proofs behind test_gpu_cluster_sort_sweeps.py (no GPU).

1. cluster_referee.row_order / row_ptr / row_list equal oracle_np.cluster_csr (the reference's loop) whole, on
   tables small enough for it: they can then stand in for it at 600 000 junctions.
2. Every fixture of cluster_sort_fixtures reaches the bucket classes it claims, by cluster_referee.sort_plan under
   the knobs the GPU test sets, and the fixtures together reach ALL of A..H:

     class  condition                                       path of bucket_sort_kernel
     A      packed (total_bits + 13 <= 64), count < 512     bitonic_sort_u64
     B      packed, 512 .. 2048                             lds_sample_sort, 128 samples
     C      packed, 2049 .. 6400                            lds_sample_sort, 256 samples
     D      packed, 6401 .. 8192                            bitonic_sort_u64 on the full key buffer
     E      8192 < count <= slot_cap                        bitonic_sort<false, uint4> in place in HBM
     F      wide keys (total_bits > 51), count <= 4096      unpacked uint4 network in LDS
     G      wide keys, 4096 < count <= slot_cap             HBM in place
     H      count > slot_cap                                ST_SLOT_OVERFLOW: generic chain / error at the next sync

   The classes each fixture names are in CLASSES below (test_fixture_classes_cover_a_to_h prints the plan's with -s).
3. The bucket sizes at the thresholds are hit EXACTLY: 511 / 512 / 513 and 2047 / 2048 by single-bucket tables,
   2081 (in 2049..2200) by a two-bucket table, and 6400 / 6401, 8192 / 8193, slot_cap / slot_cap + 1 (and 4096 / 4097
   wide keys) by the seeded searches of cluster_sort_fixtures: every search found its edge, none needed the
   64-key allowance.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_referee as CR  # noqa: E402
import cluster_sort_fixtures as FX  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd import synth  # noqa: E402


def _touching_and_nested():
    cr = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    left = np.array([100, 200, 201, 100, 100, 150, 100, 100, 100, 301], np.int32)
    right = np.array([200, 300, 250, 200, 1000, 160, 300, 300, 100, 301], np.int32)
    strand = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0], np.int8)
    return cr, left, right, strand


SMALL = {
    "touching_nested": _touching_and_nested,
    "one": lambda: synth.make_junctions(1, 1),
    "genes_300": lambda: synth.make_junctions(300, 2, n_chrom=2),
    "genes_5000": lambda: synth.make_junctions(5000, 3),
    "dense_1500": lambda: synth.make_junctions(1500, 4, n_chrom=2, gene_spacing=50, len_span=100000),
    "shared_left_group": lambda: FX.group(400, 60, 5, n_chrom=2),
    "wide": lambda: FX.wide(600, 6, k=40),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_referee_equals_oracle(name):
    a = SMALL[name]()
    want_row_of, want_row_ptr, want_col = O.cluster_csr(*a)
    assert np.array_equal(CR.row_order(*a), want_row_of)
    assert np.array_equal(CR.row_ptr(*a), want_row_ptr)
    lister = CR.RowLister(*a)
    n = a[0].size
    got_col = np.concatenate([lister(r) for r in range(n)]) if n else np.zeros(0, np.int32)
    assert np.array_equal(got_col, want_col)
    assert np.array_equal(CR.row_list(*a, n - 1), want_col[want_row_ptr[n - 1]:])
    if name in ("dense_1500", "shared_left_group"):
        assert want_col.size > 4 * n                          # (the lists are long here)


def test_sample_positions_are_distinct_and_in_range():
    for n, S in [(257, 4), (257, 128), (4097, 36), (300_000, 294), (600_000, 3516)]:
        pos = CR.sample_positions(n, S)
        assert pos.min() >= 0 and pos.max() < n and (np.diff(pos) > 0).all()


def test_plan_clamps():
    """fast_plan's clamps, restated: bucket_mean outside 256..2048 -> 2048, spb outside 2..64 -> 12, B <= 4096,
    slot_cap = min(8 * ceil(n / B), n), one bucket -> no sample."""
    cr, left, right, _ = synth.make_junctions(5000, 7)
    base = CR.sort_plan(cr, left, right)
    assert (base.B, base.spb, base.S, base.slot_cap) == (3, 12, 36, 5000)
    for bm in (0, 255, 2048, 2049, -1):
        p = CR.sort_plan(cr, left, right, bucket_mean=bm)
        assert (p.B, p.slot_cap) == (3, 5000) and np.array_equal(p.bucket_of, base.bucket_of)
    for spb in (0, 1, 12, 65):
        p = CR.sort_plan(cr, left, right, spb=spb)
        assert p.spb == 12 and np.array_equal(p.bucket_of, base.bucket_of)
    p = CR.sort_plan(cr, left, right, bucket_mean=256, spb=64)
    assert (p.B, p.spb, p.S, p.slot_cap) == (20, 64, 1280, 2000) and p.count.sum() == 5000
    p = CR.sort_plan(cr[:256], left[:256], right[:256], bucket_mean=256)
    assert (p.B, p.S, p.slot_cap) == (1, 0, 256)
    p = CR.sort_plan(cr[:257], left[:257], right[:257], bucket_mean=256, spb=2)
    assert (p.B, p.S, p.slot_cap) == (2, 4, 257)
    p = CR.sort_plan(cr, left, right, lds_cap=64)
    assert set(p.classes()) == {"E"}


@pytest.mark.parametrize("n,cls", [(1, "A"), (511, "A"), (512, "B"), (513, "B"), (2047, "B"), (2048, "B")])
def test_single_bucket_thresholds(n, cls):
    """n <= bucket_mean: one bucket of exactly n keys (no sample), on either side of SS_MIN = 512 and at the last
    size before a second bucket appears"""
    cr, left, right, _ = synth.make_junctions(n, 100 + n)
    p = CR.sort_plan(cr, left, right)
    assert p.B == 1 and p.count.tolist() == [n] and p.cls.tolist() == [cls]
    assert CR.sort_plan(*synth.make_junctions(2049, 9)[:3]).B == 2


# the classes every fixture must reach under the knobs of the GPU test (the `classes` column of the fixture table)
CLASSES = {
    "gene300k_spb2": "ABCDE",         # cluster.spb = 2: poor splitters, buckets of 248 .. 9800 keys
    "gene600k_spb2": "ABCDE",         # cluster.spb = 2, beyond the scatter kernel's tile switch
    "two_buckets_2081": "BC",
    "group_6400": "BC",
    "group_6401": "BD",
    "group_8192": "BD",
    "group_8193": "BE",
    "group_slot_cap": "AB",           # cluster.bucket_mean = 256
    "group_slot_cap_plus_1": "H",     # cluster.bucket_mean = 256
    "wide_single_bucket": "F",
    "wide_4096": "BCF",
    "wide_4097": "ABCG",
}


def test_fixture_classes_cover_a_to_h():
    assert CLASSES == {name: f["classes"] for name, f in FX.FIXTURES.items()}
    assert set("".join(CLASSES.values())) == set("ABCDEFGH")
    seen = set()
    for name, f in FX.FIXTURES.items():
        a = FX.build(name)
        p = FX.plan(name)
        got = p.classes()
        print(f"{name:24s} n={a[0].size:7d} B={p.B:4d} slot_cap={p.slot_cap:6d} largest={p.count.max():6d} "
              f"claims {f['classes']:6s} plan {''.join(sorted(got))}")
        assert set(f["classes"]) <= got, (name, f["classes"], sorted(got))
        assert p.count.sum() == a[0].size
        seen |= set(f["classes"])
        # the four arrays hold distinct, valid junctions
        key = np.stack([x.astype(np.int64) for x in a], axis=1)
        assert np.unique(key, axis=0).shape[0] == key.shape[0], name
        assert (a[1] >= 0).all() and (a[2] >= a[1]).all()
    assert seen == set("ABCDEFGH"), sorted(seen)


@pytest.mark.parametrize("name", [n for n, f in FX.FIXTURES.items() if f["largest"] is not None])
def test_fixture_hits_its_threshold_exactly(name):
    f, p = FX.FIXTURES[name], FX.plan(name)
    want = {"slot_cap": p.slot_cap, "slot_cap+1": p.slot_cap + 1}.get(f["largest"], f["largest"])
    assert p.count.max() == want, (name, p.count.max(), want)
    b = int(np.argmax(p.count))
    if name.startswith("wide"):
        assert p.total_bits[b] > 51 or p.cls[b] == "G"
    elif f["largest"] != "slot_cap+1":
        assert p.total_bits[b] + 13 <= 64 or p.count[b] > 8192


def test_overflow_pair_differs_by_one_key():
    """the class-H fixture and its neighbour below the capacity are one table and the same table without its last
    junction: same buckets, same slot_cap, the largest bucket one key apart"""
    over, below = FX.build(FX.OVERFLOW), FX.build(FX.BELOW_OVERFLOW)
    for x, y in zip(over, below):
        assert np.array_equal(x[:-1], y)
    p, q = FX.plan(FX.OVERFLOW), FX.plan(FX.BELOW_OVERFLOW)
    assert p.overflow and not q.overflow
    assert (p.B, p.slot_cap) == (q.B, q.slot_cap) == (20, 1952)
    assert p.count.max() == p.slot_cap + 1 and q.count.max() == q.slot_cap
    assert (p.count > p.slot_cap).sum() == 1


def test_fixture_lists_stay_below_the_cap():
    for name in FX.FIXTURES:
        assert FX.list_entries(*FX.build(name)) <= FX.MAX_LIST_ENTRIES, name
