// Launch geometry of the PS tile kernels (ps.hip), planned host-only (psplan.cpp: `make asan` builds it).
#pragma once
#include <stdint.h>
#include "sdice.h"
#include "params.h"

// the caps the kernels rest on
constexpr int64_t PS_LDS_MIN = 8 * 1024, PS_LDS_MAX = 160 * 1024;      // ps.lds_bytes is clamped to these
constexpr int PS_THREADS_MAX = 1024;
constexpr int PS_OFFSETS_PER_ROW = 16;     // staged neighbour offsets per tile row (col_cap = 16 R)
constexpr int PS_WORDS_PER_ROW = PS_OFFSETS_PER_ROW + 1;     // ... + the row pointer
constexpr int PS_SPARE_WORDS_V3 = 64, PS_SPARE_WORDS_GEN1 = 16;     // LDS words beside window, offsets and row pointers
constexpr int PS_REACH_BLOCK = 16;         // rows a reach word describes
constexpr int PS_HALO_AUTO = 16, PS_HALO_REACH_MAX = 32;
// the register-staged kernel addresses a tile's outputs by 32-bit offsets: s x (most rows of a tile, 2 T) < 2^30
constexpr int64_t PS_V3_MAX_TILE_ROWS = 2 * PS_THREADS_MAX, PS_V3_MAX_TILE_CELLS = (int64_t)1 << 30;
constexpr int PS_XCDS = 8, PS_XCD_REMAP_MIN_TILES = 64;
// the 16-bit-window kernel (ps_tile_w16_kernel): one geometry; a thread stages SIX vectors of the tile's own rows and one
// (on the few tiles with a longer run: two) of each halo run, and the row segments of a chunk divide the workgroup (a thread keeps its column in every vector)
constexpr int PS_W16_KERN = 3, PS_W16_OWN_VECTORS = 6;
constexpr int PS_W16_MIN_S = 257;          // column-chunked tables only
constexpr int64_t PS_W16_THREADS = 1024, PS_W16_LDS = 80 * 1024, PS_W16_CHUNK = 256;

struct SdPsFacts {
    int64_t n;
    int32_t s;
    bool aligned;           // counts and the wanted outputs are 16-byte aligned
    bool want_excl, want_ps;
    bool ctx_list;          // d_col is the context's own list (the last clustering's)
    bool reach_rows_match;  // ... whose reach words describe n rows
    bool have_reach_words;
    int cluster_reach;      // largest row distance the last clustering saw
};
struct SdPsPlan {
    int kern;               // 0 = register-staged kernel (ps_tile_v3_kernel), 2 = first-generation kernel (ps_tile_kernel),
                            // 3 = register-staged kernel with a 16-bit count window (ps_tile_w16_kernel)
    int vec;                // 4 or 1 columns per item
    int chunk_cols;
    int tile_rows, halo, col_cap, n_tiles, n_chunks, lv_shift, tiles_per_xcd;
    int use_reach, nt, prio, q3;
    int ablate;
    int threads;
    int64_t lds_bytes, grid;
};
// SDICE_ERR_ARG with the message of sdice_ps_dev when no tile fits.  Needs n >= 1, s >= 1.
int sd_ps_plan(const int64_t params[SD_P_COUNT], const SdPsFacts& f, SdPsPlan* p);
// What sdice_ps_dev launches: the plan of the 16-bit-window kernel (kern 3) where that kernel takes the call -- ps.w16 on,
// a column-chunked table that the register-staged kernel would take, no knob of the tile shape set, at least one whole
// tile of rows (or ps.w16 = 2) --, else sd_ps_plan's: the plan of the two kernels that take any tile shape.
int sd_ps_launch_plan(const int64_t params[SD_P_COUNT], const SdPsFacts& f, SdPsPlan* p);
