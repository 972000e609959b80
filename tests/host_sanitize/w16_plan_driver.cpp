// Host-only walk of the PS launch planner (csrc/psplan.cpp, sd_ps_launch_plan) over the plans of the 16-bit-window kernel (kern 3): which calls get
// it, that every such plan keeps inside what ps_tile_w16_kernel rests on (LDS words with the padding row and the
// over-read slack, the register-staging caps), pinned plans, and the refusal that stays a refusal.  Built and run by
// tests/test_ps_w16_plan_cpu.py under AddressSanitizer + UndefinedBehaviorSanitizer; no HIP, no GPU.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "ps.h"

static char g_err[256];
void sdice_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad++ < 20) printf("line %d: %s  [%s]\n", __LINE__, #c, g_tag); } } while (0)
static char g_tag[256];

struct Knobs {
    int64_t v[SD_P_COUNT];
    Knobs() { for (int i = 0; i < SD_P_COUNT; ++i) v[i] = kSdParams[i].dflt; }
    Knobs& set(SdParam k, int64_t x) { v[k] = x; return *this; }
};

static SdPsFacts facts(int64_t n, int64_t s, bool aligned, bool reach, int cluster_reach = 0) {
    SdPsFacts f;
    f.n = n; f.s = (int32_t)s; f.aligned = aligned; f.want_excl = false; f.want_ps = true;
    f.ctx_list = reach || cluster_reach > 0; f.reach_rows_match = f.have_reach_words = reach; f.cluster_reach = cluster_reach;
    return f;
}

// what the kernel rests on
static void holds(const Knobs& k, const SdPsFacts& f, const SdPsPlan& p) {
    const int64_t R = p.tile_rows, H = p.halo, cw = p.chunk_cols, T = p.threads, LV = cw / 4;
    CHECK(p.vec == 4 && cw == 256 && T == 1024 && p.lds_bytes == 80 * 1024 && p.n_chunks == (f.s + 255) / 256 && p.n_chunks > 1);
    CHECK(T % LV == 0 && LV == (64 >> p.lv_shift) && p.nt == 0 && p.ablate == 0);
    // own rows: six vectors per thread; halo runs: two; row pointers: two
    CHECK(R >= 1 && R <= 6 * T / LV && R + 1 <= 2 * T && H >= 0 && H <= 2 * T / LV);
    // LDS in 4-byte words: window rows of cw / 2 words, R + 2 H of them and the all-zero row; 16 R offsets; R + 1 row
    // pointers rounded up to 4; 16 per-wave words.  A short last batch reads 3 offsets past the stage: inside the pointers
    const int64_t used = (R + 2 * H + 1) * (cw / 2) + 16 * R + ((R + 1 + 3) & ~(int64_t)3) + 16;
    CHECK(used <= p.lds_bytes / 4 && p.col_cap == 16 * R && ((R + 1 + 3) & ~(int64_t)3) + 16 >= 3);
    CHECK(((R + 2 * H + 1) * (cw / 2)) % 4 == 0);                      // the per-wave words are read as 16-byte vectors
    CHECK((int64_t)f.s * 2048 < (int64_t)1 << 30);                     // 32-bit offsets inside a tile
    CHECK(R <= f.n && (int64_t)p.n_tiles * R >= f.n && ((int64_t)p.n_tiles - 1) * R < f.n);
    CHECK(!p.use_reach || R % 16 == 0 || (p.n_tiles == 1 && R == f.n));
    CHECK(!p.use_reach || (f.ctx_list && f.reach_rows_match && f.have_reach_words && k.v[SD_P_PS_USE_REACH] != 0));
    if (p.tiles_per_xcd) CHECK((int64_t)p.tiles_per_xcd * 8 >= p.n_tiles && p.grid == (int64_t)p.tiles_per_xcd * 8 * p.n_chunks);
    else CHECK(p.grid == (int64_t)p.n_tiles * p.n_chunks);
    CHECK(p.grid >= 1 && p.grid < (int64_t)1 << 31);
}

int main() {
    const int64_t I31 = ((int64_t)1 << 31) - 1;
    const std::vector<int64_t> ns = {1, 15, 16, 95, 96, 97, 193, 1000, 2000000, I31};
    const std::vector<int64_t> ss = {4, 100, 256, 257, 258, 260, 500, 516, 1000, 4096, (1 << 19) - 4, 1 << 19};
    const std::vector<int64_t> halos = {-1, 0, 1, 15, 16, 17, 24, 31, 32, 33, 64, 1 << 20, INT64_MAX};
    int64_t plans = 0, w16_plans = 0;
    for (int64_t w16 : {0, 1, 2, 3, -1}) for (int64_t n : ns) for (int64_t s : ss) for (int al = 0; al < 2; ++al)
        for (int reach = 0; reach < 2; ++reach) for (int64_t h : halos) for (int64_t use : {1, 0}) {
            const Knobs k = Knobs().set(SD_P_PS_W16, w16).set(SD_P_PS_HALO_ROWS, h).set(SD_P_PS_USE_REACH, use);
            const SdPsFacts f = facts(n, s, al != 0, reach != 0, reach ? 22 : 0);
            snprintf(g_tag, sizeof g_tag, "w16 %lld n %lld s %lld aligned %d reach %d halo %lld use %lld", (long long)w16, (long long)n,
                     (long long)s, al, reach, (long long)h, (long long)use);
            SdPsPlan p;
            if (sd_ps_launch_plan(k.v, f, &p) != SDICE_OK) { CHECK(strstr(g_err, "grid too large") && n == I31); continue; }
            ++plans;
            // the halo the window is planned with, and the rows it then leaves to a tile
            const int64_t h0 = std::min<int64_t>(h < 0 ? 16 : h, 32);
            int64_t r = std::min<int64_t>((80 * 1024 / 4 - 64 - (2 * h0 + 1) * 128) / (128 + 17), 96);
            if (reach && use) r &= ~(int64_t)15;
            const bool eligible = w16 != 0 && al && s % 4 == 0 && s > 256 && s * 2048 < (int64_t)1 << 30 && (w16 == 2 || n >= r);
            CHECK((p.kern == PS_W16_KERN) == eligible);
            if (p.kern != PS_W16_KERN) { CHECK(p.kern == 0 || p.kern == 2); continue; }
            ++w16_plans;
            holds(k, f, p);
            CHECK(p.tile_rows == std::min(r, n) && p.use_reach == (reach && use));
            if (h >= 0) CHECK(p.halo == h0);
            else CHECK(p.halo == (reach && use ? 24 : 16));          // reach words: what the LDS leaves beside 96 rows
        }
    CHECK(w16_plans > 1000 && w16_plans < plans / 2);
    // a knob of the tile shape keeps the kernels that take any shape, whatever ps.w16 says
    for (int64_t w16 : {1, 2}) {
        const SdPsFacts f = facts(2000000, 500, true, true, 22);
        snprintf(g_tag, sizeof g_tag, "tile knobs, w16 %lld", (long long)w16);
        SdPsPlan p;
        for (const Knobs& k : {Knobs().set(SD_P_PS_TILE_ROWS, 96), Knobs().set(SD_P_PS_CHUNK_COLS, 256), Knobs().set(SD_P_PS_THREADS, 512),
                               Knobs().set(SD_P_PS_LDS_BYTES, 160 * 1024), Knobs().set(SD_P_PS_GEN1, 1), Knobs().set(SD_P_PS_ABLATE, 1)}) {
            Knobs kk = k;
            CHECK(sd_ps_launch_plan(kk.set(SD_P_PS_W16, w16).v, f, &p) == SDICE_OK && p.kern != PS_W16_KERN);
        }
        // ... and the cluster's reach sizes the halo of a foreign-free list without reach words
        CHECK(sd_ps_launch_plan(Knobs().set(SD_P_PS_W16, w16).set(SD_P_PS_USE_REACH, 0).v, facts(2000000, 500, true, false, 5), &p) == SDICE_OK &&
              p.kern == PS_W16_KERN && p.halo == 5 && p.tile_rows == 96);
    }
    {   // pinned: the headline shape with and without reach words, the e2e shard, a one-row table under ps.w16 = 2
        struct { Knobs k; SdPsFacts f; std::vector<int64_t> want; } cases[] = {
            // kern vec cw R H col_cap n_tiles n_chunks lv_shift tiles_per_xcd use_reach nt threads lds grid
            {Knobs(), facts(2000000, 500, true, true, 22), {3, 4, 256, 96, 24, 1536, 20834, 2, 0, 2605, 1, 0, 1024, 81920, 41680}},
            {Knobs(), facts(2000000, 500, true, false), {3, 4, 256, 96, 16, 1536, 20834, 2, 0, 2605, 0, 0, 1024, 81920, 41680}},
            {Knobs(), facts(625000, 1000, true, true, 22), {3, 4, 256, 96, 24, 1536, 6511, 4, 0, 814, 1, 0, 1024, 81920, 26048}},
            {Knobs(), facts(95, 500, true, false), {0, 4, 128, 95, 16, 1520, 1, 4, 1, 0, 0, 0, 1024, 81920, 4}},
            {Knobs().set(SD_P_PS_W16, 2), facts(1, 260, true, false), {3, 4, 256, 1, 16, 16, 1, 2, 0, 0, 0, 0, 1024, 81920, 2}},
        };
        for (const auto& c : cases) {
            SdPsPlan p;
            snprintf(g_tag, sizeof g_tag, "pinned n %lld s %d", (long long)c.f.n, c.f.s);
            CHECK(sd_ps_launch_plan(c.k.v, c.f, &p) == SDICE_OK);
            const std::vector<int64_t> got = {p.kern, p.vec, p.chunk_cols, p.tile_rows, p.halo, p.col_cap, p.n_tiles, p.n_chunks, p.lv_shift,
                                              p.tiles_per_xcd, p.use_reach, p.nt, p.threads, p.lds_bytes, p.grid};
            CHECK(got == c.want);
        }
    }
    {   // refusals stay refusals: a chunk that fits no tile, a grid beyond 2^31
        SdPsPlan p;
        snprintf(g_tag, sizeof g_tag, "refusals");
        for (int64_t w16 : {0, 1, 2}) {
            CHECK(sd_ps_launch_plan(Knobs().set(SD_P_PS_W16, w16).set(SD_P_PS_CHUNK_COLS, 50000).v, facts(20, 50000, true, false), &p) == SDICE_ERR_ARG &&
                  strstr(g_err, "row chunk does not fit LDS"));
            CHECK(sd_ps_launch_plan(Knobs().set(SD_P_PS_W16, w16).set(SD_P_PS_XCD_REMAP, 0).v, facts(I31, (1 << 19) - 4, true, false), &p) == SDICE_ERR_ARG &&
                  strstr(g_err, "grid too large"));
        }
    }
    {   // sd_ps_plan itself never names the kernel: it stays the planner of the two kernels that take any tile shape
        SdPsPlan p, q;
        snprintf(g_tag, sizeof g_tag, "sd_ps_plan");
        for (int64_t w16 : {0, 1, 2}) for (int64_t n : ns) for (int64_t s : ss) {
            const Knobs k = Knobs().set(SD_P_PS_W16, w16);
            const SdPsFacts f = facts(n, s, true, true, 22);
            const int rc = sd_ps_plan(k.v, f, &p);
            CHECK(rc != SDICE_OK || p.kern == 0 || p.kern == 2);
            // ... and where the new kernel does not take the call the launch plan IS sd_ps_plan's
            const int rl = sd_ps_launch_plan(k.v, f, &q);
            CHECK(rl == rc);
            if (rc == SDICE_OK && q.kern != PS_W16_KERN) {
                auto all = [](const SdPsPlan& x) {
                    return std::vector<int64_t>{x.kern, x.vec, x.chunk_cols, x.tile_rows, x.halo, x.col_cap, x.n_tiles, x.n_chunks, x.lv_shift,
                                                x.tiles_per_xcd, x.use_reach, x.nt, x.prio, x.q3, x.ablate, x.threads, x.lds_bytes, x.grid};
                };
                CHECK(all(p) == all(q));
            }
        }
    }
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("w16 plan driver: ok (%lld plans, %lld for the 16-bit-window kernel)\n", (long long)plans, (long long)w16_plans);
    return 0;
}
