// Host-only: tile geometry of the PS kernels (ps.h; kernels and dispatch: ps.hip).  No HIP in here: `make asan` builds
// this file as it stands, and tests/host_sanitize/driver.cpp walks the plans over sizes and knobs on the CPU.
#include <algorithm>
#include "ps.h"

void sdice_set_error(const char* fmt, ...);

static int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }      // (a >= 0, b > 0; no sum to overflow)

static int refuse(const char* msg) {
    sdice_set_error("sdice_ps_dev: %s", msg);
    return SDICE_ERR_ARG;
}

// with_w16: the 16-bit-window kernel may take the call (sd_ps_launch_plan); without it the plan is one of the two
// kernels that take any tile shape (sd_ps_plan)
static int plan(const int64_t params[SD_P_COUNT], const SdPsFacts& f, SdPsPlan* p, bool with_w16) {
    const int64_t n = f.n, s = f.s;
    *p = SdPsPlan{};
    const int vec = (s % 4 == 0 && f.aligned) ? 4 : 1;
    const int abl = (int)params[SD_P_PS_ABLATE];
    int64_t cw = s;
    const int64_t chunk_param = params[SD_P_PS_CHUNK_COLS];
    if (chunk_param > 0) cw = chunk_param;
    else if (s > 256) cw = 128;
    if (cw > s) cw = s;
    if (vec == 4) cw = (cw / 4) * 4;
    if (cw < vec) cw = vec;
    // kernel: 0 = second-generation register-staged kernel (ps_tile_v3_kernel, the default; in a launch plan column-chunked
    // tables go on to its 16-bit-window sibling, kernel 3, below), 2 = first-generation kernel
    // (ps_tile_kernel; also serves tables whose rows are not 16-byte vectors, column chunks whose vectors do not divide
    // 64, tile shapes beyond the register staging of the newer kernel, and the timing experiments)
    const bool pow2chunk = cw == s || (vec == 4 && cw / 4 <= 64 && 64 % (cw / 4) == 0);      // (vec 4: cw / 4 >= 1)
    int kern = params[SD_P_PS_GEN1] != 0 ? 2 : 0;
    if (vec != 4 || abl != 0 || !pow2chunk) kern = 2;
    if (s * PS_V3_MAX_TILE_ROWS >= PS_V3_MAX_TILE_CELLS) kern = 2;       // (the newer kernel addresses a tile's outputs by 32-bit offsets)
    int64_t lds = std::min(std::max(params[SD_P_PS_LDS_BYTES], PS_LDS_MIN), PS_LDS_MAX);   // (default: two workgroups per CU)
    int64_t threads = std::min<int64_t>(std::max<int64_t>(params[SD_P_PS_THREADS] / 64 * 64, 64), PS_THREADS_MAX);

    int64_t R = 0, H = 0;
    bool have_reach = false;
    const int64_t per_row = PS_WORDS_PER_ROW;
    // kernel 3 = the register-staged kernel with a 16-bit count window (ps_tile_w16_kernel): column-chunked tables that
    // the register-staged kernel would take, at ONE geometry -- a caller that sets a knob of the tile shape (ps.tile_rows,
    // ps.chunk_cols, ps.threads, ps.lds_bytes) gets the kernels that take any shape, and a table shorter than one tile
    // keeps the register-staged kernel too (ps.w16 = 2 takes it to the new one: tests)
    const int64_t w16_param = params[SD_P_PS_W16];
    if (with_w16 && w16_param != 0 && kern == 0 && s >= PS_W16_MIN_S && chunk_param <= 0 && params[SD_P_PS_TILE_ROWS] <= 0 &&
        params[SD_P_PS_THREADS] == kSdParams[SD_P_PS_THREADS].dflt && params[SD_P_PS_LDS_BYTES] == kSdParams[SD_P_PS_LDS_BYTES].dflt) {
        // 1024 threads, 80 KiB (two workgroups per CU), 256-column chunks: a wave loads one whole row segment, S = 500 is
        // two chunks.  (512 threads, 40 KiB, 128-column chunks -- four workgroups per CU -- was measured against it in one
        // process: 2.02 ms against 1.83 ms per step at 2 M x 500, EXPERIMENTS A.22)
        const int64_t T16 = PS_W16_THREADS, lds16 = PS_W16_LDS, cw16 = PS_W16_CHUNK, LV16 = cw16 / 4;
        // LDS budget (ints): a window row is cw16 / 2 words (two counts per word); the window is R + 2 H rows and the
        // all-zero row that pads a short last batch of neighbours.  The unconditional offset reads of such a batch run
        // at most 3 words past the 16 R staged offsets: into the R + 1 row pointers and the 16 per-wave words behind them
        const int64_t L = lds16 / 4 - PS_SPARE_WORDS_V3;
        auto words16 = [&](int64_t r, int64_t h) { return (r + 2 * h + 1) * (cw16 / 2) + per_row * r; };
        const bool reach16 = f.ctx_list && f.reach_rows_match && f.have_reach_words && params[SD_P_PS_USE_REACH] != 0;
        // staging caps: SIX own vectors per thread (rows <= 6 T / LV), one vector per halo run and a second one on the
        // few tiles whose run is longer (halo <= 2 T / LV), the low words of two row pointers (rows <= 2 T - 1)
        const int64_t r_cap = std::min<int64_t>(PS_W16_OWN_VECTORS * T16 / LV16, 2 * T16 - 1), h_cap = 2 * T16 / LV16;
        int64_t h = params[SD_P_PS_HALO_ROWS];
        const bool h_auto = h < 0;
        if (h_auto) {
            h = PS_HALO_AUTO;
            if (!reach16 && f.ctx_list && f.cluster_reach > 0 && f.cluster_reach < h) h = f.cluster_reach;
        }
        h = std::min(h, h_cap);
        int64_t r = std::min((L - (2 * h + 1) * (cw16 / 2)) / (cw16 / 2 + per_row), r_cap);
        if (reach16) r &= ~(int64_t)(PS_REACH_BLOCK - 1);                                    // tiles are whole 16-row reach blocks
        if (r >= PS_REACH_BLOCK && T16 % LV16 == 0 && words16(r, h) <= L && (w16_param == 2 || n >= r)) {
            // (with reach words the halo is a capacity, as in the loop below: what is left of the LDS goes to it)
            while (reach16 && h_auto && h < PS_HALO_REACH_MAX && h + 1 <= h_cap && words16(r, h + 1) <= L) h += 1;
            kern = PS_W16_KERN; cw = cw16; threads = T16; lds = lds16; R = r; H = h; have_reach = reach16;
        }
    }
    const int64_t LV = vec == 4 ? cw / 4 : cw;              // 16-byte vectors of a window row
    // tile geometry; a shape that the register staging of the second-generation kernel cannot hold (it stages FOUR
    // vectors of the tile's own rows, TWO of each halo run and the low words of TWO row pointers per thread) falls back
    // to the first-generation kernel, whose loops take any shape
    while (kern != PS_W16_KERN) {
        const bool newk = kern == 0;
        // LDS budget (ints): (R + 2H + 1) * cw window + 16 R staged neighbour offsets + (R + 1) row pointers + scratch
        const int64_t L = lds / 4 - (newk ? PS_SPARE_WORDS_V3 : PS_SPARE_WORDS_GEN1);      // (the newer kernel keeps 16 per-wave words behind the row pointers)
        auto words = [&](int64_t r, int64_t h) { return (r + 2 * h + 1) * cw + per_row * r; };
        have_reach = newk && f.ctx_list && f.reach_rows_match && f.have_reach_words && params[SD_P_PS_USE_REACH] != 0;
        H = params[SD_P_PS_HALO_ROWS];
        const bool h_auto = H < 0;
        if (h_auto) {
            // rows further than the halo are still summed exactly (global-memory path).  With reach bytes H is the
            // CAPACITY of the window on each side (a tile stages what its lists reach, 8 + 8 rows on average on
            // gene-shaped data, 22 at most); without them H rows are staged on each side: 16 cover >99.9 % of the
            // neighbours of gene-shaped data, less if the clustering saw a smaller reach
            H = PS_HALO_AUTO;
            if (!have_reach && f.ctx_list && f.cluster_reach > 0 && f.cluster_reach < H) H = f.cluster_reach;
        }
        // (a software-pipelined persistent variant -- one workgroup per CU, two LDS buffers, next tile's
        //  loads in flight during the gather -- was built and measured 30 % slower: the kernel is VALU-issue
        //  bound, and halving the resident waves costs more than hiding the load latency gains)
        // caps of the register staging: rows <= 4 T / LV (own rows), rows <= 2 T - 1 (row pointers: nr + 1 of them),
        // halo <= T / LV (each of the two runs takes one vector per thread)
        const int64_t r_cap = newk ? std::min<int64_t>(4 * threads / LV, 2 * threads - 1) : 2 * threads;
        const int64_t h_cap = newk ? threads / LV : (int64_t)1 << 20;
        if (H > h_cap) H = h_cap;
        const int64_t r_param = params[SD_P_PS_TILE_ROWS];
        auto fit_rows = [&](int64_t h) {
            int64_t r = r_param > 0 ? r_param : (L - (2 * h + 1) * cw) / (cw + per_row);
            return std::min(r, r_cap);
        };
        R = fit_rows(H);
        while (H > 0 && (R < std::min<int64_t>(8, r_cap) || words(R, H) > L)) {
            // window does not fit: shrink the halo first (misses fall back to global loads), then the tile
            H = H / 2;
            R = fit_rows(H);
        }
        if (R < 1) R = 1;
        while (R > 1 && words(R, H) > L) R -= 1;
        if (newk && (r_cap < 1 || R > r_cap || words(R, H) > L)) { kern = 2; continue; }
        if (words(R, H) > L) return refuse("row chunk does not fit LDS; lower ps.chunk_cols");
        // (trimming R so that R * V is a multiple of the block size was measured: slower -- the per-tile
        //  fixed cost outweighs the idle lanes of the last pass over the items)
        if (have_reach && R >= PS_REACH_BLOCK && r_param <= 0) R &= ~(int64_t)(PS_REACH_BLOCK - 1);   // tiles are whole 16-row reach blocks
        have_reach = have_reach && R % PS_REACH_BLOCK == 0;
        if (have_reach && h_auto) {
            // the rows lost to the rounding are window capacity: a tile stages only what its reach words ask for, so a
            // larger capacity costs nothing and keeps the rare far-reaching tile off the global-memory path
            // (2 M x 500: 96-row tiles either way, capacity 16 -> 24, 1.686 -> 1.650 ms)
            while (H < PS_HALO_REACH_MAX && H + 1 <= h_cap && words(R, H + 1) <= L) H += 1;
        }
        break;
    }
    if (R > n) R = n;

    p->kern = kern;
    p->vec = vec;
    p->chunk_cols = (int)cw;
    p->tile_rows = (int)R;
    p->halo = (int)H;
    p->col_cap = (int)(PS_OFFSETS_PER_ROW * R);
    p->n_tiles = (int)ceil_div(n, R);
    p->n_chunks = (int)ceil_div(s, cw);
    p->prio = params[SD_P_PS_PRIO] != 0;
    // window loads that do not linger in the L2: -4 % at 1 M x 100 (0.179 -> 0.172 ms in one process); with column chunks
    // the lines shared by two chunks and the halo rows want the L2 (+1.7 % at 2 M x 500): unchunked tables only
    p->nt = params[SD_P_PS_NT_LOADS] != 0 && p->n_chunks == 1;
    p->use_reach = have_reach;
    p->lv_shift = 0;                                        // column chunks: log2(row segments per 1 KiB piece)
    for (int b = 0; b <= 6; ++b) if ((cw / 4) == (64 >> b)) p->lv_shift = b;
    p->q3 = params[SD_P_PS_QUANTIZE3] != 0;
    p->ablate = abl;
    p->threads = (int)threads;
    p->lds_bytes = lds;
    int64_t gx = p->n_tiles;
    if (params[SD_P_PS_XCD_REMAP] && p->n_tiles >= PS_XCD_REMAP_MIN_TILES) {
        p->tiles_per_xcd = (int)ceil_div(p->n_tiles, PS_XCDS);
        gx = (int64_t)p->tiles_per_xcd * PS_XCDS;
    }
    p->grid = gx * p->n_chunks;
    if (p->grid >= (int64_t)1 << 31) return refuse("grid too large");
    return SDICE_OK;
}

int sd_ps_plan(const int64_t params[SD_P_COUNT], const SdPsFacts& f, SdPsPlan* p) { return plan(params, f, p, false); }

int sd_ps_launch_plan(const int64_t params[SD_P_COUNT], const SdPsFacts& f, SdPsPlan* p) { return plan(params, f, p, true); }
