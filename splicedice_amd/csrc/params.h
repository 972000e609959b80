// The tuning and test knobs of the library: THE table of their names and defaults.  sdice_set_param / sdice_get_param /
// sdice_param_info (ctx.hip) and every read (ctx->param(SD_P_...)) go through it; a read of a knob that has no row here
// does not compile.  Defaults are the measured optima on MI355X.  A read site may clamp or reinterpret the value it
// gets (noted in the meaning); the table holds what a caller sets and gets.
//   X(identifier, name, default, meaning)
#pragma once
#include <stdint.h>

#define SD_PARAM_TABLE(X)                                                                                               \
    /* PS tile kernel (ps.hip; tools/ab_ps.py compares settings in one process) */                                      \
    X(PS_LDS_BYTES, "ps.lds_bytes", 80 * 1024, "LDS budget of a tile in bytes, clamped to 8 .. 160 KiB (the default: two workgroups per CU)") \
    X(PS_TILE_ROWS, "ps.tile_rows", 0, "rows of a tile; 0 = from the LDS budget")                                       \
    X(PS_THREADS, "ps.threads", 1024, "threads of a tile workgroup: a multiple of 64 in 64 .. 1024")                    \
    X(PS_CHUNK_COLS, "ps.chunk_cols", 0, "columns of a column chunk; 0 = all columns up to 256, else 128")              \
    X(PS_XCD_REMAP, "ps.xcd_remap", 1, "1 = consecutive tiles go to one XCD (from 64 tiles on)")                        \
    X(PS_HALO_ROWS, "ps.halo_rows", -1, "rows staged on each side of a tile; -1 = 16, or what the clustering's reach asks for") \
    X(PS_ABLATE, "ps.ablate", 0, "timing experiments: selects an ablation instantiation of the first-generation kernel") \
    X(PS_QUANTIZE3, "ps.quantize3", 0, "1 = sdice_ps_dev stores float32(f'{ps:.3f}') (the text round trip fused)")      \
    X(PS_PRIO, "ps.prio", 1, "1 = window loads at raised wave priority")                                                \
    X(PS_NT_LOADS, "ps.nt_loads", 1, "1 = non-temporal window loads when the table is not cut into column chunks")      \
    X(PS_GEN1, "ps.gen1", 0, "1 = the first-generation tile kernel (any row width / tile shape) instead of the register-staged one") \
    X(PS_USE_REACH, "ps.use_reach", 1, "1 = size a tile's halo from the per-block reach the fast clustering recorded")  \
    X(PS_W16, "ps.w16", 1, "column-chunked tables at the default tile knobs: 1 = the 16-bit-window kernel from one whole tile of rows on, 2 = at any row count (tests), 0 = the register-staged kernel") \
    /* clustering (cluster.hip, cluster_fast.hip) */                                                                   \
    X(CLUSTER_GENERIC, "cluster.generic", 0, "1 = the radix-sort path with unpacked keys")                              \
    X(CLUSTER_LEGACY, "cluster.legacy", 0, "1 = the radix-sort path")                                                   \
    X(CLUSTER_LDS_CAP, "cluster.lds_cap", 8192, "largest bucket sorted in LDS, 2 .. 8192 (0 = 8192); small values force the in-HBM sort: tests") \
    X(CLUSTER_ABLATE, "cluster.ablate", 0, "timing experiments; acts only in a library built with -DSDICE_CLUSTER_ABLATE=1") \
    X(CLUSTER_NB_GRID, "cluster.nb_grid", 0, "workgroups of the neighbour kernel; 0 = as many as the device holds at once") \
    X(CLUSTER_SAMPLE_SORT, "cluster.sample_sort", 1, "1 = LDS-local sample sort of buckets of 512 .. 4096 keys, 0 = the workgroup-wide network") \
    X(CLUSTER_BUCKET_MEAN, "cluster.bucket_mean", 2048, "mean keys per bucket, 256 .. 2048 (anything else = 2048)")     \
    X(CLUSTER_SPB, "cluster.spb", 0, "samples per bucket, 2 .. 64; 0 = 12 up to 2 Mi junctions, 8 beyond")              \
    X(CLUSTER_MAX_NNZ, "cluster.max_nnz", 0, "longest neighbour list accepted before allocation; 0 = 0.9 x free HBM / 4 B") \
    /* radix sort (radix.hip) */                                                                                        \
    X(SORT_ROUNDS, "sort.rounds", 0, "radix-sort scheduling experiment: 4 or 12 rounds (anything else = 12)")           \
    /* rank-sum test (ranksum.hip) */                                                                                   \
    X(RANKSUM_VARIANT, "ranksum.variant", 0, "0 by group size, 1 lane, 2 block, 3 wave (sorting only), 4 lane pair, 5 counting + wave") \
    X(RANKSUM_ABLATE, "ranksum.ablate", 0, "timing experiments: passed to the counting and lane kernels")               \
    /* Fisher pair kernel (fisher.hip) */                                                                               \
    X(FISHER_TABLE_MAX, "fisher.table_max", 1 << 20, "entries of the log-factorial table; tables beyond it take lgamma in a second kernel") \
    X(FISHER_REFILL, "fisher.refill", 12, "idle lanes (1 .. 64) that trigger a hand-out of pairs")                      \
    X(FISHER_UNROLL, "fisher.unroll", 16, "walk steps per trip: 4, 8, 12, 16, 20 or 24")                                \
    X(FISHER_COUNT_STEPS, "fisher.count_steps", 0, "1 = the pair kernel counts issued / useful lane-steps (sdice_fisher_step_stats)") \
    /* BH correction (bh.hip, bh_cols.hip) */                                                                           \
    X(BH_COLUMNS_PATH, "bh.columns_path", 0, "per-column BH: 0 by size, 1 generic radix path, 2 sample-sort path")      \
    X(BH_VECTOR_PATH, "bh.vector_path", 0, "one vector: 0 by size, 1 radix path, 2 sample-sort path")                   \
    X(BH_MAX_GROUP, "bh.max_group", 0, "per-column BH: most columns corrected at once; 0 = what fits the free memory (small values: tests)") \
    X(BHV_MEAN, "bhv.mean", 2048, "one vector, sample sort: mean values per bucket (at least 512)")                     \
    X(BHV_CAP, "bhv.cap", 5632, "one vector, sample sort: slot capacity of a bucket (73 KB of LDS: two bucket workgroups per CU)") \
    X(BH_REG_CAP, "bh.reg_cap", 2048, "largest bucket ranked in LDS, 0 .. 2048; beyond it one wave sorts a copy in HBM (small values: tests)") \
    X(BH_MEAN, "bh.mean", 0, "mean values per bucket; 0 = 0.55 x the 4 values per thread of a bucket workgroup (563 at 256 threads)") \
    X(BH_ROWS_PER_BLOCK, "bh.rows_per_block", 2048, "rows per transpose workgroup")                                     \
    X(BH_FUSED_COUNT, "bh.fused_count", 1, "1 = the counting pass fused into the transpose")                            \
    X(BH_FINISH_COLS, "bh.finish_cols", 16, "columns per strip of the finish kernel: 16 or 8")                          \
    X(BH_FINISH_NT, "bh.finish_nt", 0, "1 = non-temporal gather loads in the finish kernel")                            \
    X(BH_WG, "bh.wg", 256, "threads of a bucket workgroup: 256, 512 or 1024")                                           \
    X(BH_BIG_WG, "bh.big_wg", 512, "threads of a workgroup of the second bucket kernel: 512 (4 values per thread) or 256 (8)") \
    X(BH_SPB, "bh.spb", 8, "samples per bucket")                                                                        \
    /* sample Gram sums (gram.hip) */                                                                                   \
    X(GRAM_ROWS_PER_WG, "gram.rows_per_wg", 0, "rows of a workgroup's slice, raised to a multiple of 64 (the smallest slice); 0 = by size: 4096, halved down to 256 while the grid is small") \
    /* Friedman and Page tests (friedman.hip) */                                                                        \
    X(FRIEDMAN_WAVE_MAX, "friedman.wave_max", 1024, "staged values of a row (sets x subjects rounded up to a power of two) up to which one wave takes the row; above it a workgroup does (0 = always the workgroup; tests)")

enum SdParam : int {
#define X(id, name, dflt, meaning) SD_P_##id,
    SD_PARAM_TABLE(X)
#undef X
    SD_P_COUNT
};

struct SdParamRow {
    const char* name;
    int64_t dflt;
};

constexpr SdParamRow kSdParams[SD_P_COUNT] = {
#define X(id, name, dflt, meaning) {name, dflt},
    SD_PARAM_TABLE(X)
#undef X
};
