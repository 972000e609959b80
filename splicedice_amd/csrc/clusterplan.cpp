// Host-only: the launch geometry of the fast clustering path (cluster.h; kernels and launches: cluster_fast.hip).  No
// HIP in here: `make asan` builds this file as it stands, and tests/host_sanitize/driver.cpp walks the plans on the CPU.
#include <algorithm>
#include "cluster.h"

static int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }      // (a >= 0, b > 0; no sum to overflow)

bool sd_cluster_takes_legacy(const int64_t params[SD_P_COUNT], int64_t n) {
    return n > FAST_MAX_N || params[SD_P_CLUSTER_GENERIC] != 0 || params[SD_P_CLUSTER_LEGACY] != 0;
}

void sd_cluster_fast_plan(const int64_t params[SD_P_COUNT], const SdClusterFacts& f, SdClusterPlan* p) {
    const int64_t n = f.n;
    *p = SdClusterPlan{};
    int64_t bucket_mean = params[SD_P_CLUSTER_BUCKET_MEAN];
    if (bucket_mean < 256 || bucket_mean > BUCKET_MEAN) bucket_mean = BUCKET_MEAN;
    const int64_t B = std::min<int64_t>(std::max<int64_t>(ceil_div(n, bucket_mean), 1), MAX_BUCKETS);
    p->B = (int)B;
    // samples per bucket: 12 up to 2 M junctions (tighter bucket sizes: the largest bucket IS the sort kernel's time; -1.4 % on
    // the whole quant step at 1 M), 8 beyond (the sample is ranked by brute force, O(S^2))
    int64_t spb = params[SD_P_CLUSTER_SPB];
    if (spb < 2 || spb > 64) spb = n <= ((int64_t)2 << 20) ? 12 : SPB;
    p->spb = (int)spb;
    p->S = B > 1 ? (int)(B * spb) : 0;
    const int64_t mean = ceil_div(n, B);
    p->slot_cap = B > 1 ? std::min(mean * SLOT_FACTOR, n) : n;
    int64_t lds_cap = params[SD_P_CLUSTER_LDS_CAP];      // (test knob: 0 = default; small values force the HBM sort)
    if (lds_cap <= 0 || lds_cap > RDX_CAP) lds_cap = RDX_CAP;
    if (lds_cap < 2) lds_cap = 2;
    p->lds_cap = (int)lds_cap;
    p->sample_sort = params[SD_P_CLUSTER_SAMPLE_SORT] != 0;
    p->n_tiles = (int)ceil_div(n, NB_T);
    // zero region: [tile states] (needed by every neighbour run) then [cursor | rank | bmax64 | col_done]
    const int64_t nb64 = ceil_div(n, 64) + 2;
    const int64_t n_cd = (p->S + 255) / 256 + 4;
    p->zk4_bytes = ((int64_t)p->n_tiles + 2) * 8;        // (+ the ticket counter of the tile loop behind the tile states)
    p->cursor_off = p->zk4_bytes;
    p->rank_off = p->cursor_off + B * 4;
    p->bmax64_off = p->rank_off + ((int64_t)p->S + 4) * 4;
    p->col_done_off = p->bmax64_off + nb64 * 4;
    p->zero_bytes = p->col_done_off + n_cd * 4;
    p->z_alloc_bytes = p->zero_bytes + 1024;
    p->slots_bytes = B * p->slot_cap * 16;
    p->row_bytes = n * 4;
    p->spl_bytes = B * 8 + 8;
    p->reserve_bytes = p->zero_bytes + p->slots_bytes + n * 12 + B * 16 + 16 * 4096;
    p->rank_grid = (int)ceil_div(p->S, 256);
    // tiles of 2048 keys (512 threads) for small inputs, 4096 (1024 threads) beyond
    // (4096-key tiles halve the global atomics: 27.5 -> 21.4 us at 1 M keys)
    p->scatter_wg = n <= (1 << 19) ? 512 : 1024;
    p->scatter_grid = ceil_div(n, (int64_t)p->scatter_wg * SC_KPT);
    p->scatter_lds = B * 16;
    p->sort_grid = B;
    // at most as many workgroups as the device holds at once (what the look-back's forward progress rests on); cluster.nb_grid
    // overrides it downwards (tests: a handful of workgroups walking many tiles each)
    int64_t grid = std::min<int64_t>(p->n_tiles, (int64_t)f.nb_per_cu * f.n_cu);
    const int64_t forced = params[SD_P_CLUSTER_NB_GRID];
    if (forced > 0) grid = std::min(grid, forced);
    p->nb_grid = std::max<int64_t>(grid, 1);
}
