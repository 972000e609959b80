"""Seeded junction tables that drive every code path of the clustering sort stage (cluster_fast.hip), shared by
test_cluster_sort_cpu.py (which proves on the host, with cluster_referee.sort_plan, that each table reaches the
bucket classes it claims) and test_gpu_cluster_sort_sweeps.py (which runs them).

Three builders:
  gene         synth.make_junctions: gene-shaped tables with sparse lists.  Under cluster.spb = 2 the splitters are
               poor and the buckets range from a few hundred keys to beyond the LDS capacity.
  group        a sparse background plus `k` junctions that share one (chrom, left): the splitters are prefixes
               (chrom << 32 | left), so the group lands in one bucket whatever the sample.  Its lists are quadratic
               (k * k / 2 entries over two strands), capped here at 4e7 entries.
  wide         chromosome ranks {0, 2^20}, lefts near 0 and near 2e9, lengths up to 30 000: a bucket that spans them
               needs more than 51 key bits and takes the unpacked paths.
`python tests/cluster_sort_fixtures.py` redoes the seeded searches that chose the group sizes and seeds below.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_referee as CR  # noqa: E402
from splicedice_amd import synth  # noqa: E402

MAX_LIST_ENTRIES = 40_000_000


def gene(n, seed, **kw):
    return synth.make_junctions(n, seed, **kw)


_bg_cache = {}


def _background(n_bg, seed, n_chrom):
    if (n_bg, seed, n_chrom) not in _bg_cache:
        _bg_cache.clear()
        _bg_cache[(n_bg, seed, n_chrom)] = synth.make_junctions(n_bg, seed, n_chrom=2 * n_chrom)
    return _bg_cache[(n_bg, seed, n_chrom)]


def group(n_bg, k, seed, n_chrom=12, drop_last=False):
    """n_bg gene-shaped junctions on 2 * n_chrom chromosomes with a free chromosome rank in the middle, which holds k
    junctions of one left end (rights ascending, strands alternating).  Seeded shuffle; the LAST input junction is a
    group member, so that dropping it (drop_last) takes exactly one key out of the group."""
    rng = np.random.default_rng([seed, 0x67])
    cr, left, right, strand = _background(n_bg, seed, n_chrom)
    cr = np.where(cr >= n_chrom, cr + 1, cr).astype(np.int32)
    j = np.arange(k)
    g = (np.full(k, n_chrom, np.int32), np.full(k, 50_000, np.int32), (50_010 + (j >> 1)).astype(np.int32),
         (j & 1).astype(np.int8))
    cols = [np.concatenate([a, b]) for a, b in zip((cr, left, right, strand), g)]
    perm = rng.permutation(n_bg + k)
    last = int(np.flatnonzero(perm >= n_bg)[-1])              # a group member goes to the end
    perm[[last, -1]] = perm[[-1, last]]
    if drop_last:
        perm = perm[:-1]
    return tuple(np.ascontiguousarray(c[perm]) for c in cols)


def wide(n, seed, k=0):
    """n sparse junctions on chromosome ranks {0, 2^20} with lefts in [0, 5e7) and [2e9, 2e9 + 5e7) and lengths below
    30 000, plus k junctions that share the largest left of chromosome 0 (the bucket they land in goes on into
    chromosome 2^20)."""
    rng = np.random.default_rng([seed, 0x77])
    m = n + 64
    key = np.stack([rng.choice(np.array([0, 1 << 20], np.int64), size=m),
                    rng.integers(0, 50_000_000, size=m) + rng.choice(np.array([0, 2_000_000_000], np.int64), size=m),
                    rng.integers(0, 30_000, size=m), rng.integers(0, 2, size=m)], axis=1)
    key[:, 2] += key[:, 1]
    key = np.unique(key, axis=0)
    rng.shuffle(key)
    key = key[:n]
    assert key.shape[0] == n
    if k:
        j = np.arange(k)
        top = 2_050_000_001                                   # beyond every background left
        g = np.stack([np.zeros(k, np.int64), np.full(k, top), top + 1 + (j >> 1), j & 1], axis=1)
        key = np.concatenate([key, g])
        rng.shuffle(key)
    return (key[:, 0].astype(np.int32), key[:, 1].astype(np.int32), key[:, 2].astype(np.int32), key[:, 3].astype(np.int8))


BUILDERS = {"gene": gene, "group": group, "wide": wide}

# name -> builder, its arguments, the knobs the GPU test sets, the classes sort_plan must report (A..H, see the path
# table in DESIGN.md) and, for the threshold fixtures, the exact size of the largest bucket ("slot_cap" = the plan's).
# `whole`: small and sparse enough for oracle_np.cluster_csr.
FIXTURES = {}


def _fx(name, builder, args, knobs, classes, largest=None, whole=False):
    FIXTURES[name] = dict(builder=builder, args=args, knobs=knobs, classes=classes, largest=largest, whole=whole)


def plan_knobs(knobs):
    return dict(bucket_mean=knobs.get("cluster.bucket_mean", 0), spb=knobs.get("cluster.spb", 0),
                lds_cap=knobs.get("cluster.lds_cap", 0))


_cache = {}


def build(name):
    """-> (cr, left, right, strand) of a fixture; built once per process, never written to"""
    if name not in _cache:
        f = FIXTURES[name]
        arrs = BUILDERS[f["builder"]](**f["args"])
        for a in arrs:
            a.setflags(write=False)
        _cache[name] = arrs
    return _cache[name]


def plan(name, arrays=None):
    cr, left, right, _ = arrays if arrays is not None else build(name)
    return CR.sort_plan(cr, left, right, **plan_knobs(FIXTURES[name]["knobs"]))


def list_entries(cr, left, right, strand):
    return int(CR.row_ptr(cr, left, right, strand)[-1])


SPB2 = {"cluster.spb": 2}
MEAN256 = {"cluster.bucket_mean": 256}
#    name                    builder  arguments                                      knobs    classes  largest bucket
_fx("gene300k_spb2",         "gene",  dict(n=300_000, seed=4),                       SPB2,    "ABCDE")
_fx("gene600k_spb2",         "gene",  dict(n=600_000, seed=3),                       SPB2,    "ABCDE")
_fx("two_buckets_2081",      "gene",  dict(n=4096, seed=1, n_chrom=3),               {},      "BC",    2081, whole=True)
_fx("group_6400",            "group", dict(n_bg=20_000, k=6179, seed=1),             {},      "BC",    6400)
_fx("group_6401",            "group", dict(n_bg=20_000, k=5471, seed=1),             {},      "BD",    6401)
_fx("group_8192",            "group", dict(n_bg=20_000, k=7951, seed=1),             {},      "BD",    8192)
_fx("group_8193",            "group", dict(n_bg=20_000, k=6968, seed=2),             {},      "BE",    8193)
_fx("group_slot_cap",        "group", dict(n_bg=3000, k=1874, seed=1, drop_last=True), MEAN256, "AB",  "slot_cap")
_fx("group_slot_cap_plus_1", "group", dict(n_bg=3000, k=1874, seed=1),               MEAN256, "H",     "slot_cap+1")
_fx("wide_single_bucket",    "wide",  dict(n=2000, seed=1),                          {},      "F",     2000, whole=True)
_fx("wide_4096",             "wide",  dict(n=6000, seed=2, k=3868),                  {},      "BCF",   4096)
_fx("wide_4097",             "wide",  dict(n=6000, seed=1, k=3514),                  {},      "ABCG",  4097)
OVERFLOW, BELOW_OVERFLOW = "group_slot_cap_plus_1", "group_slot_cap"


# ---------------------------------------------------------------------------------------------- the searches
def search_group(edge, knobs, n_bg, seeds=range(1, 9), budget_s=55.0):
    """(seed, k) whose group bucket holds exactly `edge` keys (edge = 'slot_cap' or 'slot_cap+1': relative to the plan),
    k descending from the edge: the bucket is the group plus the background keys up to the next splitter."""
    import time
    t0 = time.time()
    for seed in seeds:
        hi = edge if isinstance(edge, int) else 8 * knobs["cluster.bucket_mean"] + 8
        for k in range(hi, max(hi - 2200, 2), -1):
            if time.time() - t0 > budget_s:
                return None
            a = group(n_bg, k, seed)
            p = CR.sort_plan(a[0], a[1], a[2], **plan_knobs(knobs))
            want = edge if isinstance(edge, int) else p.slot_cap + (1 if edge.endswith("+1") else 0)
            b = p.bucket_of[-1]
            if p.count[b] == want and p.count.max() == want:
                if edge == "slot_cap+1":                       # one key fewer must sit exactly at the capacity
                    q = CR.sort_plan(a[0][:-1], a[1][:-1], a[2][:-1], **plan_knobs(knobs))
                    if q.slot_cap != p.slot_cap or q.count.max() != q.slot_cap:
                        continue
                return seed, k
    return None


def search_wide(edges=(4096, 4097), n=6000, seeds=range(1, 6)):
    """{edge: (seed, k)}: wide(n, seed, k) with a wide-key bucket of exactly `edge` keys, k descending from 4096"""
    found = {}
    for seed in seeds:
        for k in range(4096, 2000, -1):
            a = wide(n, seed, k)
            p = CR.sort_plan(a[0], a[1], a[2])
            for b in np.flatnonzero(np.isin(p.count, edges)):
                if (p.total_bits[b] > 51 or p.cls[b] == "G") and p.count.max() == p.count[b]:
                    found.setdefault(int(p.count[b]), (seed, k))
            if len(found) == len(edges):
                return found
    return found


if __name__ == "__main__":
    print("wide", search_wide(), flush=True)
    for edge, knobs, n_bg in [(6400, {}, 20_000), (6401, {}, 20_000), (8192, {}, 20_000), (8193, {}, 20_000),
                              ("slot_cap+1", {"cluster.bucket_mean": 256}, 3000)]:
        print(edge, knobs, n_bg, "->", search_group(edge, knobs, n_bg), flush=True)
