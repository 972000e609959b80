// Host-only: how many columns of a table the column BH corrects at once, and the launch geometry of the sample-sort
// paths of bh_cols.hip (bh.h).  No HIP in here: `make asan` builds this file as it stands, and
// tests/host_sanitize/driver.cpp walks the plans over sizes and knobs on the CPU.
#include <algorithm>
#include "bh.h"

void sdice_set_error(const char* fmt, ...);

static int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }      // (a >= 0, b > 0; no sum to overflow)

int64_t sd_bh_column_group(int64_t budget, int64_t per_column, int64_t fixed, int64_t cols, int64_t max_group) {
    int64_t g = budget > fixed ? (budget - fixed) / per_column : 0;
    g = std::max<int64_t>(1, std::min(g, std::min(cols, max_group)));
    if (g < cols && g > 16) g &= ~(int64_t)15;
    return g;
}

// scratch bytes the sample-sort path needs for `segs` columns of m values: transposed input (8 B per value), bucketed
// keys / results (8), position words (4), the in-HBM path's copies (8), per-bucket tables
size_t sd_bh_cols_scratch(int64_t m, int64_t segs) {
    const size_t vals = (size_t)m * (size_t)segs;
    return vals * 28 + (size_t)segs * (size_t)(MAX_B + 1) * 50 + (1 << 16);
}

bool sd_bh_cols_supported(int64_t m, int64_t segs) {
    return m >= 1 && m <= ((int64_t)1 << POS_SHIFT) && segs >= 1 && segs <= 0x7fffffff;
}

#define BHS_REFUSE(cond, msg)                                          \
    do {                                                               \
        if (!(cond)) {                                                 \
            sdice_set_error("sd_bh_cols_samplesort: %s", msg);         \
            return SDICE_ERR_ARG;                                      \
        }                                                              \
    } while (0)

int sd_bhs_plan(const int64_t params[SD_P_COUNT], const SdBhsFacts& f, SdBhsPlan* p) {
    const int64_t m = f.m, segs = f.segs;
    const int64_t GRID_MAX = (int64_t)1 << 31;
    *p = SdBhsPlan{};
    // buckets: bh.wg threads per bucket workgroup (256 / 512 / 1024: buckets of up to 1024 / 2048 / 4096 values), mean bucket
    // (bh.mean, default: half the workgroup's capacity)
    const int64_t wg_param = params[SD_P_BH_WG];
    const int wg_threads = wg_param >= 1024 ? 1024 : wg_param >= 512 ? 512 : 256;
    p->wg_threads = wg_threads;
    // A column stays ONE bucket only while that bucket keeps to the route a one-bucket column can take: ranked in LDS
    // straight from the p-values, by its workgroup or (listed) by the second kernel -- never the in-HBM path, which
    // writes through the spill buffer a one-bucket plan does not allocate.
    int64_t B = 1;
    if (m > std::min<int64_t>(4 * (int64_t)wg_threads, BHS_REG_MAX)) {
        int64_t mean = params[SD_P_BH_MEAN];
        // (25 000 x 19 900, 256 threads: mean 400 / 450 / 512 / 600 -> 14.7 / 14.3 / 14.1 / 13.9 ms: fewer, fuller workgroups
        //  against more buckets beyond the capacity, ~1 % at 0.55 of it)
        if (mean <= 0) mean = wg_threads * 4 * 55 / 100;
        mean = std::max<int64_t>(mean, ceil_div(m, (int64_t)MAX_B));
        B = ceil_div(m, mean);
        B = std::min<int64_t>(B, std::min<int64_t>(MAX_B, m / 2));     // (two rows per sample stride at least)
        B = std::max<int64_t>(B, 2);
    }
    p->B = (int)B;
    p->reg_cap = (int)std::min<int64_t>(BHS_REG_MAX, std::max<int64_t>(0, params[SD_P_BH_REG_CAP]));
    int64_t spb = std::max<int64_t>(params[SD_P_BH_SPB], 1);
    while (spb > 1 && spb > BHS_SAMPLE_MAX / B) spb >>= 1;      // spb B <= 8192: the sample is sorted in 96 KB of LDS
    while (spb > 1 && spb * B * 2 > m) spb >>= 1;
    p->spb = (int)spb;
    p->S = (int)(spb * B);
    p->S2 = 1;
    while (p->S2 < p->S) p->S2 <<= 1;

    const int64_t vals = m * segs, sb = segs * B;
    p->p_cm_bytes = p->keyS_bytes = vals * 8;
    p->spl_k_bytes = p->bmin_bytes = p->sfx_bytes = p->big_list_bytes = sb * 8;
    p->spl_i_bytes = p->gcount_bytes = p->cursor_bytes = sb * 4;
    p->start_bytes = segs * (B + 1) * 4;
    p->zeroed_bytes = 16;                                        // spill_n | big_count
    p->pos_cm_bytes = B > 1 ? vals * 4 : 0;
    p->spill_bytes = B > 1 ? vals * 8 : 0;

    const int64_t strips = ceil_div(segs, (int64_t)TC_COLS);
    BHS_REFUSE(strips < GRID_MAX, "bh: too many columns");
    p->rows_per_block = (int)std::max<int64_t>(TC_ROWS, std::min<int64_t>(params[SD_P_BH_ROWS_PER_BLOCK], m));
    p->strips_per_xcd = (int)ceil_div(strips, (int64_t)8);
    p->tgrid = (int64_t)p->strips_per_xcd * 8 * ceil_div(m, (int64_t)p->rows_per_block);
    BHS_REFUSE(p->tgrid < GRID_MAX, "bh: too many tiles");
    if (B > 1) {
        p->lds_sample = (int64_t)p->S2 * 12;
        p->lds_tile = B * 20;
        p->tiles = (int)ceil_div(m, (int64_t)TILE);
        p->tile_blocks = ceil_div(segs, (int64_t)8) * 8 * p->tiles;
        BHS_REFUSE(p->tile_blocks < GRID_MAX, "bh: too many tiles");
        // the splitters of a 16-column strip beside the transpose tile: up to ~190 buckets per column; beyond, the
        // transpose runs alone and the tiles of the scatter kernel count first
        p->lds_tc = (int64_t)TC_COLS * ((B - 1) * 12 + B * 4);
        p->fused_count = p->lds_tc <= BHS_FUSED_LDS_MAX && params[SD_P_BH_FUSED_COUNT] != 0;
        if (!p->fused_count) p->lds_tc = 0;
    }
    const int64_t n_buckets = segs * B;
    p->bucket_blocks = ceil_div(segs, (int64_t)8) * 8 * B;
    BHS_REFUSE(p->bucket_blocks < GRID_MAX, "bh: too many buckets");
    // threads of a bucket workgroup (4 values each): twice the mean bucket, so that ~1 % of the buckets (sizes ~ Gamma(8))
    // overflow to the second kernel
    p->lds_bucket = (int64_t)sd_bhs_bucket_lds(wg_threads, 4);
    // the listed buckets of 1 025 ... 2 048 values: 512 threads x 4 values (109 VGPRs) take 0.61 ms on the bench's table where
    // 256 x 8 (173 VGPRs, two waves per SIMD) take 0.77
    p->big_wg = params[SD_P_BH_BIG_WG] >= 512 ? 512 : 256;
    p->lds_big = (int64_t)(p->big_wg == 512 ? sd_bhs_bucket_lds(512, 4) : sd_bhs_bucket_lds(256, 8));
    p->big_blocks = std::max<int64_t>(1, std::min<int64_t>(n_buckets, (int64_t)f.n_cu * 4));
    p->zoom_blocks = std::max<int64_t>(1, std::min<int64_t>(n_buckets, (int64_t)f.n_cu * 6));
    p->lds_zoom = (int64_t)sd_bhs_bucket_lds(256, 4);
    // bh.finish_cols: columns per workgroup of the last kernel (16: full 128-byte lines out, 3.2 MB of results per strip
    // at 25 000 rows; 8: half lines, half the L2 footprint of the gather); bh.finish_nt: non-temporal gather loads
    p->fcols = params[SD_P_BH_FINISH_COLS] >= 16 ? 16 : 8;
    p->fnt = params[SD_P_BH_FINISH_NT] != 0;
    p->row_tiles = (int)ceil_div(m, (int64_t)(2048 / p->fcols));
    p->fin_blocks = ceil_div(ceil_div(segs, (int64_t)p->fcols), (int64_t)8) * 8 * p->row_tiles;
    BHS_REFUSE(p->fin_blocks < GRID_MAX, "bh: too many tiles");
    return SDICE_OK;
}

// One vector of n p-values.  Supported sizes: the sample fits the brute-force ranking and a bucket fits LDS.
bool sd_bh_vector_supported(int64_t n) { return n >= BHV_MIN_N && n <= BHV_MAX_N; }

// geometry of the one-vector path: buckets of ~2048 values, 16 samples per bucket (sizes ~ Gamma(16): sigma = mean / 4);
// a bucket beyond its slot / the LDS capacity (5632 = mean + 7 sigma) practically never occurs (slow path: one wave, HBM)
void sd_bhv_plan(const int64_t params[SD_P_COUNT], int64_t n, SdBhvPlan* p) {
    *p = SdBhvPlan{};
    int64_t mean = params[SD_P_BHV_MEAN];
    if (mean < 512) mean = 512;
    if (mean < ceil_div(n, (int64_t)MAX_B)) mean = ceil_div(n, (int64_t)MAX_B);
    const int64_t B = std::min<int64_t>(std::max<int64_t>(ceil_div(n, mean), 2), MAX_B);
    // 5632 x 13 B = 73 KB of LDS: two bucket workgroups per CU
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(params[SD_P_BHV_CAP], 64), BHV_T * BHV_EPT);
    p->B = (int)B;
    p->cap = (int)cap;
    p->S = (int)(BHV_SPB * B);
    p->rank_grid = (int)ceil_div(p->S, 256);
    p->tiles = (int)ceil_div(n, (int64_t)(BHV_T * BHV_E));
    p->lds_tile = B * 20;
    p->lds_bucket = (cap * 13 + 15) / 16 * 16;
    // one zeroed block: rank[S] | cursor[B] | tile_done[S / 256] | m_eff | ovf_n | spill_n, m_eff on an 8-byte boundary
    const int64_t front = p->S + B + p->rank_grid;
    p->m_eff_word = (int)(front + (front & 1));
    p->zwords = front + 8;
    p->z_bytes = p->zwords * 4;
    p->keyS_bytes = B * cap * 8;
    p->qpart_bytes = p->ovfK_bytes = p->spillK_bytes = n * 8;
    p->bmin_bytes = p->spl_k_bytes = B * 8;
    p->idxS_bytes = B * cap * 4;
    p->ovfI_bytes = p->spillI_bytes = n * 4;
    p->bid_bytes = p->ovfB_bytes = n * 2;
    p->spl_i_bytes = B * 4;
}

// slots (12 B x cap per bucket) + partial results (10 B per value) + the overflow list and the slow path's assembly area
// (14 + 12 B per value) + the sample ranks
size_t sd_bhv_scratch(const int64_t params[SD_P_COUNT], int64_t n) {
    SdBhvPlan p;
    sd_bhv_plan(params, n, &p);
    return (size_t)n * 36 + (size_t)p.B * (size_t)p.cap * 12 + (size_t)p.B * 80 + (1 << 16);
}
