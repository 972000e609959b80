// What the kernels of cluster_fast.hip and the host-only planner of their launches (clusterplan.cpp: `make asan` builds
// it) both read.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sdice.h"
#include "params.h"

constexpr int SPB = 8;                 // sample keys per bucket beyond 2 Mi junctions (12 up to there)
constexpr int BUCKET_MEAN = 2048;      // keys per bucket (mean)
constexpr int MAX_BUCKETS = 4096;      // splitters + per-bucket counters must fit LDS of the scatter kernel
constexpr int SLOT_FACTOR = 8;         // bucket slot capacity in HBM = 8 x mean
constexpr int64_t FAST_MAX_N = (int64_t)MAX_BUCKETS * BUCKET_MEAN;
static_assert(kSdParams[SD_P_CLUSTER_BUCKET_MEAN].dflt == BUCKET_MEAN, "the default is the largest mean the kernels take");
// status block (uint64 words)
constexpr int SB_FLAGS = 0, SB_NNZ = 2, SB_MAXLEN = 32, SB_REACH = 64, SB_WORDS = 96;
// word SB_STICKY lies BEHIND the words a chain clears: every flag is also OR-ed into it, and only the call that reports
// the status clears it -- the failure of an asynchronous chain survives the chains enqueued behind it
constexpr int SB_STICKY = SB_WORDS, SB_ALLOC_WORDS = SB_WORDS + 8;
constexpr int SB_SLOTS = 32;
constexpr int SC_KPT = 4;              // keys per thread of a scatter tile
constexpr int SORT_T = 1024;           // threads of a sort workgroup
constexpr int RDX_CAP = 8192;          // packed 64-bit keys a bucket may hold in LDS
constexpr size_t SORT_LDS_BYTES = (size_t)RDX_CAP * 8;     // 64 KB: two workgroups per CU
constexpr int NB_T = 512;              // threads = rows of a tile of the neighbour kernel

// true: sdice_cluster_dev takes the radix-sort path (cluster.hip) -- by size or by knob
bool sd_cluster_takes_legacy(const int64_t params[SD_P_COUNT], int64_t n);

struct SdClusterFacts {
    int64_t n;              // junctions, 1 .. FAST_MAX_N
    int nb_per_cu;          // workgroups of the neighbour kernel a CU holds at once (the occupancy query)
    int n_cu;
};
// Integers only; the byte figures are what Arena::alloc is asked for, in the order of allocation.
struct SdClusterPlan {
    int B, spb, S;
    int64_t slot_cap;
    int lds_cap, sample_sort, n_tiles;
    // the zero region: tile_state (+ ticket) | cursor | rank | bmax64 | col_done.  `zk4_bytes` is the first part, needed again
    // when only the neighbour kernel is re-run; the others are byte offsets into the region.
    int64_t zk4_bytes, zero_bytes, cursor_off, rank_off, bmax64_off, col_done_off;
    int64_t z_alloc_bytes, slots_bytes, row_bytes /* x 3: rowC, rowL, rowR2 */, spl_bytes;
    int64_t reserve_bytes;
    int rank_grid;          // side of the ranking grid (0: one bucket, no sample)
    int scatter_wg;         // 512 or 1024
    int64_t scatter_grid, scatter_lds, sort_grid, nb_grid;
};
void sd_cluster_fast_plan(const int64_t params[SD_P_COUNT], const SdClusterFacts& f, SdClusterPlan* p);
