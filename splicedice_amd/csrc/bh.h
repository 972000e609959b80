// What bh.hip (the entry points, the radix paths) and bh_cols.hip (the sample-sort paths) share, and the host-only
// arithmetic of the column-group loop and of the sample-sort launches (bhplan.cpp: `make asan` builds it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sdice.h"
#include "params.h"

// per pair column (bh_cols.hip): `segs` columns of m values of a row-major table, in place; scratch from the context arena
size_t sd_bh_cols_scratch(int64_t m, int64_t segs);
bool sd_bh_cols_supported(int64_t m, int64_t segs);
int sd_bh_cols_samplesort(sdice_ctx* ctx, int64_t m, int64_t segs, double* d_rm, int64_t pitch);
// one vector (bh_cols.hip)
bool sd_bh_vector_supported(int64_t n);
size_t sd_bh_vector_scratch(sdice_ctx* ctx, int64_t n);
int sd_bh_vector_samplesort(sdice_ctx* ctx, int64_t n, const double* d_p, const uint8_t* d_tested, bool masked, double* d_q);

// Columns of a table of `cols` that one pass corrects when a group of g columns needs per_column * g + fixed bytes of
// scratch: what `budget` holds, at least 1, at most cols and max_group; a group that is not the whole table and holds more
// than 16 columns is rounded down to a multiple of 16 (whole 128-byte lines of the row-major table).
int64_t sd_bh_column_group(int64_t budget, int64_t per_column, int64_t fixed, int64_t cols, int64_t max_group);

// ---- constants the kernels of bh_cols.hip and the planners below both read
constexpr int TILE_T = 512;         // threads of a scatter tile
constexpr int TILE_E = 8;           // values per thread
constexpr int TILE = TILE_T * TILE_E;
constexpr int MAX_B = 1024;         // buckets of a column / of the vector: one per thread of the widest workgroup
constexpr int POS_SHIFT = 18;       // pos word: bucket << 18 | slot inside the column (m <= 2^18, buckets <= 2^10)
constexpr int TC_COLS = 16, TC_ROWS = 128, TC_T = 256;      // the transpose tile and its workgroup
constexpr int BHS_REG_MAX = 2048;   // most values a bucket workgroup ranks in LDS (512 threads x 4, 256 x 8)
constexpr int BHS_SAMPLE_MAX = 8192;   // most samples of a column: sorted in 96 KB of LDS (12 B each)
constexpr int BHS_FUSED_LDS_MAX = 48 * 1024;   // splitters of a 16-column strip beside the transpose tile
// LDS of a bucket workgroup of T threads x K values: L[NS] (8 B) | CNT[2 NS + 4] (4 B) | wred[32] (8 B) | wtot[16] | hv[4]
constexpr size_t sd_bhs_bucket_lds(int T, int K) { return (size_t)T * K * 16 + 16 + 32 * 8 + 16 * 4 + 16; }
constexpr int BHV_T = 1024;         // threads of every bhv kernel but the ranking
constexpr int BHV_E = 4;            // values per thread in a count / scatter / finish tile
constexpr int BHV_EPT = 6;          // values per thread of a bucket workgroup (cap <= 6144)
constexpr int BHV_SPB = 16;         // samples per bucket of the vector
constexpr int64_t BHV_MIN_N = 16384, BHV_MAX_N = (int64_t)2 << 20;     // (up to 1024 buckets of 2048 on average)
// sub-buckets: up to 128 of ~16 values, 2 samples each (sizes ~ Gamma(2): a value meets ~24 candidates on average; with
// 64 sub-buckets of ~32 and 4 samples each -- Gamma(4) -- it met ~40, and the counting loop is the kernel's VALU load)
constexpr int BHV_SPS_LOG = 1, BHV_SPS = 1 << BHV_SPS_LOG, BHV_NSB_MAX = 256 / BHV_SPS, BHV_SUB_MEAN = 20;
// the __shared__ arrays of bhv_bucket_kernel: samK, ssk, smin (8 B) | samI, ssi, scount, sstart, srank, wsum (4 B)
constexpr size_t BHV_BUCKET_STATIC_LDS = (256 + BHV_NSB_MAX + 16) * 8 + (256 + 3 * BHV_NSB_MAX + 1 + 256 + 16) * 4;

// ---- launch geometry of the sample-sort paths (bhplan.cpp).  A planner reads the knobs in force (ctx->params) and a few
// facts and returns integers only: counts, grids, LDS bytes, the bytes of every arena piece.  A plan that cannot be made
// returns the status and message of the entry point.
struct SdBhsFacts {
    int64_t m, segs;        // rows and columns of the group
    int n_cu;
};
struct SdBhsPlan {
    int wg_threads;         // bucket workgroup: 256, 512 or 1024
    int B, reg_cap, spb, S, S2;
    int fused_count;        // 1 = the counting pass rides the transpose
    int rows_per_block, strips_per_xcd, tiles;
    int big_wg;             // 512 (4 values per thread) or 256 (8)
    int fcols, fnt, row_tiles;
    int64_t tgrid, tile_blocks, bucket_blocks, big_blocks, zoom_blocks, fin_blocks;
    int64_t lds_sample, lds_tile, lds_tc, lds_bucket, lds_big, lds_zoom;
    // arena pieces, in the order of allocation
    int64_t p_cm_bytes, keyS_bytes, spl_k_bytes, bmin_bytes, sfx_bytes, big_list_bytes, spl_i_bytes, gcount_bytes,
        cursor_bytes, start_bytes, zeroed_bytes, pos_cm_bytes, spill_bytes;     // (the last two: 0 when B == 1)
};
int sd_bhs_plan(const int64_t params[SD_P_COUNT], const SdBhsFacts& f, SdBhsPlan* p);

struct SdBhvPlan {
    int B, cap, S;
    int rank_grid;          // side of the ranking grid: ceil(S / 256)
    int tiles;
    int64_t lds_tile, lds_bucket;
    int64_t zwords;         // the zeroed block: rank[S] | cursor[B] | tile_done[rank_grid] | pad | m_eff | ovf_n | spill_n
    int m_eff_word;         // word of m_eff inside it (even: 8-byte aligned)
    // arena pieces, in the order of allocation
    int64_t z_bytes, keyS_bytes, qpart_bytes, ovfK_bytes, spillK_bytes, bmin_bytes, idxS_bytes, ovfI_bytes, spillI_bytes,
        bid_bytes, ovfB_bytes, spl_k_bytes, spl_i_bytes;
};
void sd_bhv_plan(const int64_t params[SD_P_COUNT], int64_t n, SdBhvPlan* p);
// the bound bh.hip reserves for the vector path (sd_bh_vector_scratch with the knobs spelled out)
size_t sd_bhv_scratch(const int64_t params[SD_P_COUNT], int64_t n);
