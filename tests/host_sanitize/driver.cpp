// Sanitizer driver for the threaded host C++ of the library (csrc/textio.cpp, csrc/juncio.cpp):
// built by `make -C splicedice_amd/csrc asan` / `tsan` together with those two files (no HIP, no GPU)
// and run by tests/test_host_sanitizers.py.  It pushes every host entry point through its threaded
// path: table writer (3 modes) -> table reader round trip, column writer, cluster writer, junction
// parser on the golden inputs (all file types) and the row lookup; then the argument checks of the pair
// tests (csrc/paircheck.cpp) and of the column lists (csrc/colcheck.cpp) on both sides of their bounds, the
// column-group arithmetic of BH (csrc/bhplan.cpp), and the launch planners of PS, clustering and BH (csrc/psplan.cpp,
// clusterplan.cpp, bhplan.cpp): every plan of the sweeps in plan_sweeps.h must keep inside the limits the kernels rest
// on, and a table of plans is pinned field for field.
// Any ASan / UBSan / TSan report makes the process exit non-zero.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "sdice.h"
#include "paircheck.h"      // splicedice_amd/csrc: the argument checks of the pair tests
#include "colcheck.h"       //                      ... and of the column lists
#include "bh.h"             //                      the column groups of BH
#include "stagelayout.h"    //                      the result block of a host entry point
#include "plan_sweeps.h"    // ps.h, cluster.h, bh.h: the launch planners and the inputs they are walked over

static char g_err[1024];
void sdice_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, g_err); return 1; } } while (0)
#define CHECK_V(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, g_err); ++bad; return; } } while (0)

// ---- what the kernels rest on, per plan (0 = holds)
static const int64_t LDS_MAX = 160 * 1024, GRID_MAX = (int64_t)1 << 31;
static int64_t round256(int64_t b) { return b == 0 ? 256 : (b + 255) / 256 * 256; }      // as Arena::alloc rounds

static int ps_plan_holds(const int64_t* k, const SdPsFacts& f, const SdPsPlan& p) {
    const int64_t R = p.tile_rows, H = p.halo, cw = p.chunk_cols, T = p.threads, s = f.s;
    CHECK(p.vec == 4 || p.vec == 1);
    CHECK(T >= 64 && T <= PS_THREADS_MAX && T % 64 == 0);
    CHECK(p.lds_bytes >= PS_LDS_MIN && p.lds_bytes <= PS_LDS_MAX && p.lds_bytes <= LDS_MAX);
    CHECK(cw >= p.vec && cw <= s && cw % p.vec == 0 && (int64_t)p.n_chunks * cw >= s && ((int64_t)p.n_chunks - 1) * cw < s);
    CHECK(H >= 0);
    const int64_t window = (R + 2 * H + 1) * cw + PS_WORDS_PER_ROW * R;
    if (p.kern == 0) {                  // the register-staged kernel
        const int64_t LV = cw / 4;
        CHECK(p.vec == 4 && f.aligned && s % 4 == 0 && p.ablate == 0);
        CHECK(cw == s || (LV <= 64 && 64 % LV == 0));
        CHECK(s * 2048 < (int64_t)1 << 30);
        CHECK(R <= std::min<int64_t>(4 * T / LV, 2 * T - 1) && H <= T / LV);
        CHECK(window <= p.lds_bytes / 4 - 64);
        // tiles begin on whole 16-row reach blocks (a table shorter than a tile is ONE tile, cut to its n rows)
        CHECK(!p.use_reach || R % 16 == 0 || (p.n_tiles == 1 && R == f.n));
        if (p.n_chunks > 1 || cw != s) CHECK(LV == (64 >> p.lv_shift));
    } else {                            // the first-generation kernel
        CHECK(p.kern == 2 && !p.use_reach);
        CHECK(R <= 2 * T);
        CHECK(window <= p.lds_bytes / 4 - 16);
    }
    CHECK(!p.use_reach || (f.ctx_list && f.reach_rows_match && f.have_reach_words && k[SD_P_PS_USE_REACH] != 0));
    CHECK(R >= 1 && R <= f.n && p.col_cap == 16 * R && (int64_t)p.n_tiles * R >= f.n && ((int64_t)p.n_tiles - 1) * R < f.n);
    CHECK(p.grid >= 1 && p.grid < GRID_MAX);
    if (p.tiles_per_xcd) CHECK((int64_t)p.tiles_per_xcd * 8 >= p.n_tiles && p.grid == (int64_t)p.tiles_per_xcd * 8 * p.n_chunks);
    else CHECK(p.grid == (int64_t)p.n_tiles * p.n_chunks);
    CHECK(!p.nt || p.n_chunks == 1);
    return 0;
}

static int cluster_plan_holds(const SdClusterFacts& f, const SdClusterPlan& p) {
    const int64_t n = f.n;
    CHECK(p.B >= 1 && p.B <= MAX_BUCKETS);
    CHECK((p.S == 0) == (p.B == 1));
    CHECK(p.spb >= 2 && p.spb <= 64 && (p.S == 0 || p.S == p.B * p.spb));
    if (p.S >= 1) CHECK(n / p.S >= 1);                    // the stride sample_pos divides by
    CHECK(p.slot_cap >= 1 && p.slot_cap <= n && (p.B > 1 || p.slot_cap == n));
    CHECK(p.lds_cap >= 2 && p.lds_cap <= RDX_CAP);
    CHECK(p.scatter_lds == (int64_t)p.B * 16 && p.scatter_lds <= LDS_MAX);
    CHECK((p.scatter_wg == 512 || p.scatter_wg == 1024) && p.scatter_grid * p.scatter_wg * SC_KPT >= n && p.scatter_grid < GRID_MAX);
    CHECK(p.sort_grid == p.B);
    CHECK((int64_t)p.rank_grid * 256 >= p.S && (int64_t)p.rank_grid * p.rank_grid < GRID_MAX);
    CHECK((int64_t)p.n_tiles * NB_T >= n);
    // the look-back's forward progress: never more workgroups than the device holds at once
    CHECK(p.nb_grid >= 1 && p.nb_grid <= std::max<int64_t>(1, std::min<int64_t>(p.n_tiles, (int64_t)f.nb_per_cu * f.n_cu)));
    // the zero region: tile_state (+ ticket) | cursor | rank | bmax64 | col_done, in that order, none overlapping
    CHECK(((int64_t)p.n_tiles + 1) * 8 <= p.zk4_bytes && p.zk4_bytes % 8 == 0);
    CHECK(p.cursor_off == p.zk4_bytes);
    CHECK(p.rank_off >= p.cursor_off + (int64_t)p.B * 4);
    CHECK(p.bmax64_off >= p.rank_off + (int64_t)p.S * 4);
    CHECK(p.col_done_off >= p.bmax64_off + (n + 63) / 64 * 4);
    CHECK(p.zero_bytes >= p.col_done_off + (int64_t)p.rank_grid * 4 && p.zero_bytes <= p.z_alloc_bytes);
    CHECK(p.slots_bytes == (int64_t)p.B * p.slot_cap * 16 && p.row_bytes == n * 4 && p.spl_bytes >= (int64_t)p.B * 8);
    CHECK(p.reserve_bytes >= round256(p.z_alloc_bytes) + round256(p.slots_bytes) + 3 * round256(p.row_bytes) + round256(p.spl_bytes));
    return 0;
}

static int bhs_plan_holds(const SdBhsFacts& f, const SdBhsPlan& p) {
    const int64_t m = f.m, segs = f.segs;
    CHECK(m <= (int64_t)1 << POS_SHIFT);
    CHECK(p.wg_threads == 256 || p.wg_threads == 512 || p.wg_threads == 1024);
    CHECK(p.B >= 1 && p.B <= MAX_B);
    CHECK(p.spb >= 1 && p.S == p.spb * p.B && p.S <= BHS_SAMPLE_MAX);
    if (p.B > 1) CHECK(2 * (int64_t)p.S <= m);           // every sample stride of bhs_sample_kernel has a row
    CHECK(p.S2 >= p.S && (p.S2 & (p.S2 - 1)) == 0 && (p.S2 == 1 || p.S2 / 2 < p.S) && (int64_t)p.S2 * 12 <= LDS_MAX);
    CHECK(p.reg_cap >= 0 && p.reg_cap <= BHS_REG_MAX);
    // one bucket: ranked in LDS from the p-values (the in-HBM path would write through the spill buffer B == 1 lacks)
    if (p.B == 1) CHECK(m <= std::min<int64_t>(4 * p.wg_threads, BHS_REG_MAX));
    if (p.B > 1) {
        CHECK(p.lds_sample == (int64_t)p.S2 * 12 && p.lds_tile == (int64_t)p.B * 20 && p.lds_tile <= 64 * 1024);
        CHECK((int64_t)p.tiles * TILE >= m && p.tile_blocks >= segs * p.tiles && p.tile_blocks < GRID_MAX);
        if (p.fused_count) CHECK(p.lds_tc == TC_COLS * ((int64_t)(p.B - 1) * 12 + (int64_t)p.B * 4) && p.lds_tc <= BHS_FUSED_LDS_MAX);
        CHECK(p.pos_cm_bytes == m * segs * 4 && p.spill_bytes == m * segs * 8);
    } else {
        CHECK(!p.fused_count && p.pos_cm_bytes == 0 && p.spill_bytes == 0);
    }
    CHECK(p.rows_per_block >= TC_ROWS);
    CHECK((int64_t)p.strips_per_xcd * 8 * TC_COLS >= segs && p.tgrid >= 1 && p.tgrid < GRID_MAX);
    CHECK(p.tgrid / ((int64_t)p.strips_per_xcd * 8) * p.rows_per_block >= m);
    CHECK(p.bucket_blocks >= segs * p.B && p.bucket_blocks < GRID_MAX);
    CHECK(p.big_blocks >= 1 && p.big_blocks <= std::max<int64_t>(1, segs * p.B) && p.zoom_blocks >= 1 && p.zoom_blocks < GRID_MAX);
    CHECK(p.lds_bucket == (int64_t)sd_bhs_bucket_lds(p.wg_threads, 4) && p.lds_bucket <= LDS_MAX);
    CHECK((p.big_wg == 512 || p.big_wg == 256) && p.lds_big == (int64_t)sd_bhs_bucket_lds(512, 4) && p.lds_zoom <= p.lds_big);
    CHECK((p.fcols == 16 || p.fcols == 8) && (int64_t)p.row_tiles * (2048 / p.fcols) >= m && p.fin_blocks < GRID_MAX);
    CHECK(p.fin_blocks >= (segs + p.fcols - 1) / p.fcols * p.row_tiles);
    CHECK(p.p_cm_bytes == m * segs * 8 && p.keyS_bytes == m * segs * 8 && p.zeroed_bytes == 16);
    CHECK(p.start_bytes == segs * (p.B + 1) * 4 && p.gcount_bytes == segs * p.B * 4 && p.big_list_bytes == segs * p.B * 8);
    const int64_t pieces[] = {p.p_cm_bytes, p.keyS_bytes, p.spl_k_bytes, p.bmin_bytes, p.sfx_bytes, p.big_list_bytes, p.spl_i_bytes,
                              p.gcount_bytes, p.cursor_bytes, p.start_bytes, p.zeroed_bytes};
    int64_t sum = p.B > 1 ? round256(p.pos_cm_bytes) + round256(p.spill_bytes) : 0;
    for (int64_t b : pieces) sum += round256(b);
    CHECK((int64_t)sd_bh_cols_scratch(m, segs) >= sum);
    return 0;
}

static int bhv_plan_holds(const int64_t* k, int64_t n, const SdBhvPlan& p) {
    CHECK(sd_bh_vector_supported(n));
    CHECK(p.B >= 2 && p.B <= BHV_T && p.B <= MAX_B);
    CHECK(p.S == BHV_SPB * p.B && n / p.S >= 1 && n / p.S <= UINT32_MAX && n <= UINT32_MAX);     // bhv_sample_pos: 32 bits
    CHECK(p.cap >= 64 && p.cap <= BHV_T * BHV_EPT);
    CHECK(p.lds_bucket >= (int64_t)p.cap * 13 && p.lds_bucket % 16 == 0 && p.lds_bucket + (int64_t)BHV_BUCKET_STATIC_LDS <= LDS_MAX);
    CHECK(p.lds_tile == (int64_t)p.B * 20 && p.lds_tile <= 64 * 1024);
    CHECK((int64_t)p.rank_grid * 256 >= p.S && (int64_t)p.tiles * BHV_T * BHV_E >= n);
    CHECK(p.m_eff_word % 2 == 0 && p.m_eff_word >= p.S + p.B + p.rank_grid && p.zwords >= p.m_eff_word + 6 && p.z_bytes == p.zwords * 4);
    CHECK(p.keyS_bytes == (int64_t)p.B * p.cap * 8 && p.idxS_bytes == (int64_t)p.B * p.cap * 4 && p.qpart_bytes == n * 8 && p.bid_bytes == n * 2);
    const int64_t pieces[] = {p.z_bytes, p.keyS_bytes, p.qpart_bytes, p.ovfK_bytes, p.spillK_bytes, p.bmin_bytes, p.idxS_bytes,
                              p.ovfI_bytes, p.spillI_bytes, p.bid_bytes, p.ovfB_bytes, p.spl_k_bytes, p.spl_i_bytes};
    int64_t sum = 0;
    for (int64_t b : pieces) sum += round256(b);
    CHECK((int64_t)sd_bhv_scratch(k, n) >= sum);
    return 0;
}

// a plan as the list of its fields, in the order of the struct
static Vals fields(const SdPsPlan& p) {
    return {p.kern, p.vec, p.chunk_cols, p.tile_rows, p.halo, p.col_cap, p.n_tiles, p.n_chunks, p.lv_shift, p.tiles_per_xcd, p.use_reach, p.nt,
            p.prio, p.q3, p.ablate, p.threads, p.lds_bytes, p.grid};
}
static Vals fields(const SdClusterPlan& p) {
    return {p.B, p.spb, p.S, p.slot_cap, p.lds_cap, p.sample_sort, p.n_tiles, p.zk4_bytes, p.zero_bytes, p.cursor_off, p.rank_off, p.bmax64_off,
            p.col_done_off, p.z_alloc_bytes, p.slots_bytes, p.row_bytes, p.spl_bytes, p.reserve_bytes, p.rank_grid, p.scatter_wg, p.scatter_grid,
            p.scatter_lds, p.sort_grid, p.nb_grid};
}
static Vals fields(const SdBhsPlan& p) {
    return {p.wg_threads, p.B, p.reg_cap, p.spb, p.S, p.S2, p.fused_count, p.rows_per_block, p.strips_per_xcd, p.tiles, p.big_wg, p.fcols, p.fnt,
            p.row_tiles, p.tgrid, p.tile_blocks, p.bucket_blocks, p.big_blocks, p.zoom_blocks, p.fin_blocks, p.lds_sample, p.lds_tile, p.lds_tc,
            p.lds_bucket, p.lds_big, p.lds_zoom, p.p_cm_bytes, p.keyS_bytes, p.spl_k_bytes, p.bmin_bytes, p.sfx_bytes, p.big_list_bytes,
            p.spl_i_bytes, p.gcount_bytes, p.cursor_bytes, p.start_bytes, p.zeroed_bytes, p.pos_cm_bytes, p.spill_bytes};
}
static Vals fields(const SdBhvPlan& p) {
    return {p.B, p.cap, p.S, p.rank_grid, p.tiles, p.lds_tile, p.lds_bucket, p.zwords, p.m_eff_word, p.z_bytes, p.keyS_bytes, p.qpart_bytes,
            p.ovfK_bytes, p.spillK_bytes, p.bmin_bytes, p.idxS_bytes, p.ovfI_bytes, p.spillI_bytes, p.bid_bytes, p.ovfB_bytes, p.spl_k_bytes,
            p.spl_i_bytes};
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: driver <tmpdir> <junction file>:<type> ...\n"); return 2; }
    const std::string tmp = argv[1];
    const int64_t n = 20011; const int s = 37;
    std::vector<std::string> nm(n);
    std::string names; std::vector<int64_t> off(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) { nm[i] = "chr" + std::to_string(i % 23) + ":" + std::to_string(i * 7) + "-" + std::to_string(i * 7 + 100) + ":+"; names += nm[i]; off[i + 1] = (int64_t)names.size(); }
    std::vector<float> f32((size_t)n * s); std::vector<double> f64((size_t)n * s); std::vector<int32_t> i32((size_t)n * s);
    unsigned x = 12345u;
    for (size_t k = 0; k < f32.size(); ++k) {
        x = x * 1664525u + 1013904223u;
        f32[k] = (x >> 8) % 97 == 0 ? NAN : (float)((x >> 9) % 1001) / 1000.0f;
        f64[k] = (double)(x >> 3) / 536870912.0 * ((x & 7) == 0 ? 1e-30 : 1.0);
        i32[k] = (int32_t)((x >> 7) % 5000);
    }
    std::string hdr = "cluster";
    for (int c = 0; c < s; ++c) hdr += "\tS" + std::to_string(c);
    hdr += "\n";
    const std::string p3 = tmp + "/t3.tsv", p0 = tmp + "/t0.tsv", pr = tmp + "/tr.tsv", pc = tmp + "/tc.tsv", pk = tmp + "/tk.tsv";
    for (int threads : {1, 0, 7}) {
        CHECK(sdice_write_table(p3.c_str(), hdr.c_str(), n, s, names.data(), off.data(), f32.data(), 0, 0, threads) == 0);
        CHECK(sdice_write_table(p0.c_str(), hdr.c_str(), n, s, names.data(), off.data(), i32.data(), 2, 1, threads) == 0);
        CHECK(sdice_write_table(pr.c_str(), hdr.c_str(), n, s, names.data(), off.data(), f64.data(), 1, 2, threads) == 0);
        // round trip: '.3f' text of k/1000 values reads back as the same float32; repr text of float64 is exact
        sdice_table* t = nullptr; int64_t rn = 0, nb = 0, hb = 0; int32_t rs = 0;
        CHECK(sdice_table_open(p3.c_str(), &t, &rn, &rs, &nb, &hb) == 0 && rn == n && rs == s);
        std::vector<char> rh((size_t)hb + 1), rnames((size_t)nb + 1); std::vector<int64_t> roff(n + 1); std::vector<float> back((size_t)n * s);
        CHECK(sdice_table_read(t, rh.data(), rnames.data(), roff.data(), back.data(), 0, threads) == 0);
        CHECK(sdice_table_close(t) == 0);
        for (size_t k = 0; k < back.size(); ++k) CHECK((isnan(back[k]) && isnan(f32[k])) || back[k] == f32[k]);
        CHECK(roff[n] == off[n] && memcmp(rnames.data(), names.data(), names.size()) == 0);
        CHECK(sdice_table_open(pr.c_str(), &t, &rn, &rs, &nb, &hb) == 0);
        std::vector<double> back64((size_t)n * s);
        rh.assign((size_t)hb + 1, 0); rnames.assign((size_t)nb + 1, 0);
        CHECK(sdice_table_read(t, rh.data(), rnames.data(), roff.data(), back64.data(), 1, threads) == 0);
        CHECK(sdice_table_close(t) == 0);
        for (size_t k = 0; k < back64.size(); ++k) CHECK(back64[k] == f64[k]);
        // column writer: mixed dtypes / modes
        std::vector<float> c0(n); std::vector<double> c1(n);
        for (int64_t i = 0; i < n; ++i) { c0[i] = f32[(size_t)i * s]; c1[i] = f64[(size_t)i * s]; }
        const void* cols[2] = {c0.data(), c1.data()}; const int32_t dt[2] = {0, 1}, md[2] = {2, 2};
        CHECK(sdice_write_columns(pc.c_str(), "event\tx\ty\n", n, names.data(), off.data(), 2, cols, dt, md, threads) == 0);
        // cluster writer: a ring of neighbours + an empty list
        std::vector<int64_t> rp(n + 1, 0); std::vector<int32_t> col;
        for (int64_t i = 0; i < n; ++i) { if (i % 5) { col.push_back((int32_t)((i + 1) % n)); col.push_back((int32_t)((i + n - 1) % n)); } rp[i + 1] = (int64_t)col.size(); }
        CHECK(sdice_write_clusters(pk.c_str(), n, names.data(), off.data(), rp.data(), col.data(), threads) == 0);
        col[3] = (int32_t)n + 5;                     // an out-of-range neighbour must be refused, not read
        CHECK(sdice_write_clusters(pk.c_str(), n, names.data(), off.data(), rp.data(), col.data(), threads) != 0);
        // junction bed writer: three chromosome names, an out-of-range chromosome index must be refused
        const std::string cn = "chr1chrXKI270728.1"; const int64_t co[4] = {0, 4, 8, 18};
        std::vector<int32_t> ch(n), lf(n), rt(n); std::string sd((size_t)n, '+');
        for (int64_t i = 0; i < n; ++i) { ch[i] = (int32_t)(i % 3); lf[i] = (int32_t)(i * 7); rt[i] = (int32_t)(i * 7 + 100 + i % 11); if (i % 2) sd[i] = '-'; }
        CHECK(sdice_write_junction_bed(pk.c_str(), n, cn.data(), co, 3, ch.data(), lf.data(), rt.data(), sd.data(), threads) == 0);
        if (n > 2) { ch[2] = 3; CHECK(sdice_write_junction_bed(pk.c_str(), n, cn.data(), co, 3, ch.data(), lf.data(), rt.data(), sd.data(), threads) != 0); }
    }
    // junction parser + lookup on every file given as path:type
    for (int a = 2; a < argc; ++a) {
        std::string arg = argv[a];
        const size_t c = arg.rfind(':');
        const std::string path = arg.substr(0, c); const int type = atoi(arg.c_str() + c + 1);
        for (int threads : {1, 0, 5}) {
            sdice_juncfile* f = nullptr; int64_t nl = 0, cb = 0; int32_t nc = 0;
            CHECK(sdice_junc_open(path.c_str(), type, &f, &nl, &nc, &cb) == 0);
            std::vector<int32_t> ci(nl + 1), l(nl + 1), r(nl + 1); std::vector<int8_t> st(nl + 1); std::vector<int64_t> sc(nl + 1), coff(nc + 1);
            std::vector<uint8_t> ad(nl + 1); std::vector<char> cn((size_t)cb + 1);
            CHECK(sdice_junc_read(f, 50, 50000, 5, 5, 1.0, 0, ci.data(), l.data(), r.data(), st.data(), sc.data(), ad.data(), cn.data(), coff.data(), threads) == 0);
            CHECK(sdice_junc_close(f) == 0);
            int64_t admitted = 0;
            for (int64_t i = 0; i < nl; ++i) admitted += ad[i];
            CHECK(nl > 0 && admitted > 0);
        }
    }
    {   // row lookup: every row finds itself, a stranger does not
        std::vector<int32_t> rc(n), rl(n), rr(n), out(n + 1); std::vector<int8_t> rs8(n);
        for (int64_t i = 0; i < n; ++i) { rc[i] = (int32_t)(i / 1000); rl[i] = (int32_t)(i % 1000) * 10; rr[i] = rl[i] + 5; rs8[i] = 0; }
        CHECK(sdice_junc_lookup(n, rc.data(), rl.data(), rr.data(), rs8.data(), n, rc.data(), rl.data(), rr.data(), rs8.data(), out.data(), 0) == 0);
        for (int64_t i = 0; i < n; ++i) CHECK(out[i] == (int32_t)i);
        int32_t qc = 3, ql = 7, qr = 8; int8_t qs = 1; int32_t o1 = 0;
        CHECK(sdice_junc_lookup(n, rc.data(), rl.data(), rr.data(), rs8.data(), 1, &qc, &ql, &qr, &qs, &o1, 1) == 0 && o1 == -1);
    }
    {   // count columns side by side + transpose, key packing, row names (the ingest's second half)
        const int64_t nr = 20000; const int32_t ns = 6;
        std::vector<int32_t> rc(nr), rl(nr), rr(nr); std::vector<int8_t> rs8(nr);
        for (int64_t i = 0; i < nr; ++i) { rc[i] = (int32_t)(i / 5000); rl[i] = (int32_t)(i % 5000) * 10; rr[i] = rl[i] + 7; rs8[i] = (int8_t)(i & 1); }
        std::vector<int32_t> table_t((size_t)ns * nr, 0), table((size_t)ns * nr, -1);
        std::vector<uint8_t> low((size_t)ns * nr, 0);
        std::vector<int64_t> score(nr);
        for (int64_t i = 0; i < nr; ++i) score[i] = i % 9;
        std::vector<std::thread> pool;
        std::atomic<int> bad{0};
        for (int32_t c = 0; c < ns; ++c)
            pool.emplace_back([&, c] {
                if (sdice_junc_count_column(nr, rc.data(), rl.data(), rr.data(), rs8.data(), nr, rc.data(), rl.data(), rr.data(), rs8.data(),
                                            score.data(), 5, table_t.data() + (size_t)c * nr, low.data() + (size_t)c * nr) != 0) bad++;
            });
        for (auto& th : pool) th.join();
        CHECK(bad == 0);
        CHECK(sdice_transpose_i32(ns, nr, table_t.data(), table.data(), 4) == 0);
        for (int64_t i = 0; i < nr; i += 997) for (int32_t c = 0; c < ns; ++c) CHECK(table[(size_t)i * ns + c] == (int32_t)(i % 9) && low[(size_t)c * nr + i] == (i % 9 < 5));
        int32_t rank_of[4] = {2, 0, 3, 1};
        std::vector<int32_t> crank(nr); std::vector<uint64_t> keys(nr); std::vector<uint8_t> admit(nr, 1);
        int64_t nk = 0; int32_t packable = 0;
        CHECK(sdice_junc_pack_keys(nr, rc.data(), rank_of, 4, rl.data(), rr.data(), rs8.data(), admit.data(), crank.data(), keys.data(), &nk, &packable) == 0);
        CHECK(nk == nr && packable == 1 && crank[5000] == 0 && (keys[1] >> 52) == 2);
        const char cnames[] = "chrAchrBBchrCchrDDD"; int64_t coff[5] = {0, 4, 9, 13, 19};
        std::vector<char> strand(nr); for (int64_t i = 0; i < nr; ++i) strand[i] = rs8[i] ? '-' : '+';
        std::vector<char> nm((size_t)nr * 40); std::vector<int64_t> noff(nr + 1); int64_t need = 0;
        CHECK(sdice_junction_names(nr, cnames, coff, 4, rc.data(), rl.data(), rr.data(), strand.data(), nm.data(), (int64_t)nm.size(), noff.data(), &need) == 0);
        CHECK(need == noff[nr] && std::string(nm.data() + noff[1], (size_t)(noff[2] - noff[1])) == "chrA:10-17:-");
        CHECK(sdice_junction_names(nr, cnames, coff, 4, rc.data(), rl.data(), rr.data(), strand.data(), nm.data(), 10, noff.data(), &need) != 0);
        CHECK(sdice_host_threads() >= 1 && sdice_textio_trim() == 0);
    }
    {   // the argument checks of the pair tests (csrc/paircheck.cpp) on both sides of every bound; a refusal names its cause
        const int64_t T = (int64_t)1 << 53, big = INT64_MAX;
        #define REFUSED(call, word) CHECK((call) == SDICE_ERR_ARG && strstr(g_err, word))
        for (bool walk : {false, true}) {
            // the two largest totals add up to 2^53 (accepted) and to 2^53 + 1
            int32_t i3[3] = {1, 1, 0}; int64_t e3[3] = {(T >> 1) - 1, (T >> 1) - 1, 5};
            CHECK(sd_check_pair_counts("t", 1, 3, i3, e3, walk) == SDICE_OK);
            e3[1] += 1;
            REFUSED(sd_check_pair_counts("t", 1, 3, i3, e3, walk), "add up to");
            // sample 0 holds the largest inclusion count AND the largest exclusion sum: the products to judge are
            // 2^20 * 2^33 (its count, the second sum) and 2^13 * 2^40 = 2^53 -- and never 2^20 * 2^40
            int32_t i2[3] = {1 << 20, 1 << 13, 2}; int64_t e2[3] = {(int64_t)1 << 40, (int64_t)1 << 33, 7};
            CHECK(sd_check_pair_counts("t", 1, 3, i2, e2, walk) == SDICE_OK);
            e2[1] += 1;                                               // 2^20 * (2^33 + 1) is above 2^53
            if (walk) REFUSED(sd_check_pair_counts("t", 1, 3, i2, e2, true), "times another");
            else CHECK(sd_check_pair_counts("t", 1, 3, i2, e2, false) == SDICE_OK);
            int32_t i1[2] = {1, 1}; int64_t e1[2] = {big, big};       // no signed overflow on the way to the refusal
            REFUSED(sd_check_pair_counts("t", 1, 2, i1, e1, walk), "exclusion sum");
            e1[0] = 4; e1[1] = -1;
            REFUSED(sd_check_pair_counts("t", 1, 2, i1, e1, walk), "non-negative");
            i1[0] = -1; e1[1] = 4;
            REFUSED(sd_check_pair_counts("t", 1, 2, i1, e1, walk), "non-negative");
            CHECK(sd_check_pair_counts("t", 0, 2, nullptr, nullptr, walk) == SDICE_OK);      // n = 0: nothing is read
            int64_t e0[1] = {T - 1};
            CHECK(sd_check_pair_counts("t", 1, 1, i1 + 1, e0, walk) == SDICE_OK);            // s = 1: one sample, no pair
        }
        // two rows: the second one is judged on its own maxima
        int32_t ir[4] = {1 << 30, 0, 1, 1}; int64_t er[4] = {0, 1 << 20, T - 2, 0};
        CHECK(sd_check_pair_counts("t", 2, 2, ir, er, true) == SDICE_OK);
        const int32_t self[4] = {0, 1, 2, 2}, past[4] = {0, 1, 5, 2}, neg[4] = {0, 1, -1, 2};
        CHECK(sd_check_pair_list("t", 5, 1, self) == SDICE_OK);
        REFUSED(sd_check_pair_list("t", 5, 2, self), "with itself");
        REFUSED(sd_check_pair_list("t", 5, 2, past), "must lie in");
        REFUSED(sd_check_pair_list("t", 5, 2, neg), "must lie in");
        CHECK(sd_check_pair_list("t", 5, 0, nullptr) == SDICE_OK);
        int64_t tab[8] = {1, 5, 7, 3, (int64_t)1 << 26, 0, 0, (int64_t)1 << 27};            // the second: a d = 2^53
        CHECK(sd_check_tables("t", 2, tab) == SDICE_OK);
        tab[4] = 3; tab[7] = 3002399751580331;                                               // a d = 2^53 + 1
        REFUSED(sd_check_tables("t", 2, tab), "table 1");
        tab[7] = (int64_t)1 << 27; tab[4] = 0; tab[5] = ((int64_t)1 << 26) + 1; tab[6] = (int64_t)1 << 27;  // b c = 2^53 + 2^27
        REFUSED(sd_check_tables("t", 2, tab), "table 1");
        tab[5] = T; tab[6] = 0; tab[7] = 1;                                                  // total 2^53 + 1
        REFUSED(sd_check_tables("t", 2, tab), "table 1");
        tab[5] = big; tab[7] = big;                                                          // (no overflow in the total)
        REFUSED(sd_check_tables("t", 2, tab), "table 1");
        tab[2] = -7;
        REFUSED(sd_check_tables("t", 2, tab), "non-negative");
        CHECK(sd_check_tables("t", 0, nullptr) == SDICE_OK);
        const int32_t ends[4] = {8191, 0, 0, 8191};
        std::vector<uint32_t> packed;
        sd_pack_pair_list(2, ends, packed);
        CHECK(packed.size() == 2 && packed[0] == 0x1fff0000u && packed[1] == 0x00001fffu);
        sd_pack_pair_list(0, nullptr, packed);
        CHECK(packed.empty());
        #undef REFUSED
    }
    {   // the argument checks of the column lists (csrc/colcheck.cpp) on both sides of every bound; a refusal names its cause
        #define REFUSED(call, word) CHECK((call) == SDICE_ERR_ARG && strstr(g_err, word) && strstr(g_err, "fn: ") == g_err)
        const int s = 9;
        const int32_t a[3] = {0, 4, s - 1}, b[3] = {1, 2, 3}, low[3] = {6, -1, 2}, past[3] = {6, s, 2}, twice[3] = {5, 6, 5},
                      shared[3] = {7, 4, 6};
        CHECK(check_columns("fn", {a, b}, 3, s, "range", "once") == SDICE_OK);            // 0 and s - 1 are columns
        CHECK(check_columns("fn", {a}, 0, 0, "range", "once") == SDICE_OK);               // nothing listed, no table
        REFUSED(check_columns("fn", {low}, 3, s, "range", "once"), "range");
        REFUSED(check_columns("fn", {b, past}, 3, s, "range", "once"), "range");
        REFUSED(check_columns("fn", {twice}, 3, s, "range", "once"), "once");
        REFUSED(check_columns("fn", {a, shared}, 3, s, "range", "once"), "once");
        CHECK(check_columns("fn", {a}, 3, s - 1, "range", "once") == SDICE_ERR_ARG);      // s - 1 is no column of s - 1
        // two groups of their own lengths, limit 4: the lists first, then the counts
        const int32_t st1[3] = {0, 1, 2}, st2[3] = {2, 2, 0}, neg[3] = {0, -1, 0}, zero[3] = {0, 0, 0}, four[4] = {1, 2, 3, 5}, five[5] = {1, 2, 3, 5, 6};
        CHECK(check_two_groups("fn", a, 3, b, 3, s, 4) == SDICE_OK);
        CHECK(check_two_groups("fn", a, 1, four, 4, s, 4) == SDICE_OK);                   // counts 1 and the limit
        CHECK(check_two_groups("fn", a, 3, b, 3, 6, 4) == SDICE_ERR_ARG);                 // (s - 1 = 8 is no column of 6)
        REFUSED(check_two_groups("fn", a, 3, low, 3, s, 4), "index out of range");
        REFUSED(check_two_groups("fn", past, 3, b, 3, s, 4), "index out of range");
        REFUSED(check_two_groups("fn", twice, 3, b, 3, s, 4), "once over both lists");
        REFUSED(check_two_groups("fn", a, 3, shared, 3, s, 4), "once over both lists");
        REFUSED(check_two_groups("fn", a, 3, five, 5, s, 4), "at most 4 each");           // limit + 1: the lists are not read
        REFUSED(check_two_groups("fn", past, 5, b, 3, s, 4), "at most 4 each");
        REFUSED(check_two_groups("fn", a, 0, b, 3, s, 4), "each needs 1..4");
        REFUSED(check_two_groups("fn", low, 3, b, 0, s, 4), "each needs 1..4");
        REFUSED(check_two_groups("fn", a, -1, b, 3, s, 4), "each needs 1..4");
        REFUSED(check_two_groups("fn", a, 3, four, 4, 6, 4), "index out of range");       // the list's fault comes first
        REFUSED(check_two_groups("fn", b, 3, four + 3, 1, 3, 4), "index out of range");
        REFUSED(check_two_groups("fn", nullptr, 3, nullptr, 4, 6, 4), "more selected columns than the table has");
        CHECK(check_two_groups("fn", nullptr, 3, nullptr, 3, 6, 4) == SDICE_OK);          // device lists: the counts alone
        // ... with stratum ids in [0, n_strata), n_strata in 1..3
        CHECK(check_two_groups("fn", a, 3, b, 3, s, 4, st1, st2, 3, 3) == SDICE_OK);
        CHECK(check_two_groups("fn", a, 3, b, 3, s, 4, zero, zero, 1, 3) == SDICE_OK);               // one stratum
        REFUSED(check_two_groups("fn", a, 3, b, 3, s, 4, st1, st2, 2, 3), "stratum id outside");      // id == n_strata
        REFUSED(check_two_groups("fn", a, 3, b, 3, s, 4, st2, neg, 3, 3), "stratum id outside");      // id -1
        REFUSED(check_two_groups("fn", a, 3, low, 3, s, 4, neg, st2, 3, 3), "stratum id outside");    // (entry by entry, g1 first)
        REFUSED(check_two_groups("fn", a, 3, b, 3, s, 4, st1, st2, 0, 3), "0 strata");
        REFUSED(check_two_groups("fn", a, 3, low, 3, s, 4, neg, neg, 4, 3), "4 strata");              // (the lists are not read)
        REFUSED(check_two_groups("fn", a, 0, b, 3, s, 4, st1, st2, 0, 3), "each needs 1..4");         // (the counts before the strata)
        CHECK(check_two_groups("fn", nullptr, 3, nullptr, 3, s, 4, nullptr, nullptr, 3, 3) == SDICE_OK);
        // the sets of the k-set tests
        #undef REFUSED
        #define REFUSED(call, word) CHECK((call) == SDICE_ERR_ARG && strstr(g_err, word))
        std::vector<int32_t> sp(KW_MAX_SETS + 2);
        for (int i = 0; i <= KW_MAX_SETS + 1; ++i) sp[i] = 3 * i;
        CHECK(kw_check_sets("fn", sp.data(), 2, 6) == SDICE_OK);
        CHECK(kw_check_sets("fn", sp.data(), KW_MAX_SETS, 3 * KW_MAX_SETS) == SDICE_OK);
        REFUSED(kw_check_sets("fn", nullptr, 2, 6), "set_ptr is NULL");
        REFUSED(kw_check_sets("fn", sp.data(), 1, 6), "must be 2..64");
        REFUSED(kw_check_sets("fn", sp.data(), KW_MAX_SETS + 1, 1000), "must be 2..64");
        REFUSED(kw_check_sets("fn", sp.data() + 1, 2, 100), "set_ptr[0] must be 0");       // (starts at 3)
        REFUSED(kw_check_sets("fn", sp.data(), 2, 5), "more selected columns than the table has");
        int32_t flat[4] = {0, 3, 3, 7}, back[4] = {0, 4, 3, 7}, wide[3] = {0, 3, KW_MAX_N}, wider[3] = {0, 3, KW_MAX_N + 1};
        REFUSED(kw_check_sets("fn", flat, 3, 9), "must increase");
        REFUSED(kw_check_sets("fn", back, 3, 9), "must increase");
        CHECK(kw_check_sets("fn", wide, 2, KW_MAX_N) == SDICE_OK);
        REFUSED(kw_check_sets("fn", wider, 2, KW_MAX_N + 1), "fn: 16385 selected columns");
        #undef REFUSED
    }
    {   // the column groups of BH (csrc/bhplan.cpp): (budget - fixed) / per_column, at least 1, at most cols and max_group,
        // a multiple of 16 when it is more than 16 and not the whole table
        const int64_t T = 1000000000000, BIG = INT64_MAX;
        struct { int64_t budget, cols, max_group, want; } cases[] = {
            {T, 37, 65535, 37},                 // everything fits
            {0, 37, 65535, 1},
            {999, 37, 65535, 1},                // budget below `fixed`
            {1000, 37, 65535, 1},
            {1199, 37, 65535, 1},  {1200, 37, 65535, 2},
            {3100, 37, 65535, 16},              // room for 21
            {2700, 37, 65535, 16},              // room for 17
            {2600, 37, 65535, 16},              // room for 16
            {2599, 37, 65535, 15},              // room for 15, not rounded
            {4699, 37, 65535, 32}, {4700, 37, 65535, 37},     // room for 36 | the whole table: not rounded
            {T, 70000, 65535, 65520},
            {T, 37, 5, 5}, {T, 37, 1, 1}, {T, 16, 21, 16}, {T, 37, 21, 16}, {T, 37, 37, 37}, {T, 37, 36, 32},
            {BIG, 37, 65535, 37}, {BIG - 1, 70000, 65535, 65520}, {BIG, BIG, BIG, (BIG - 1000) / 100 & ~(int64_t)15},
        };
        for (const auto& c : cases) CHECK(sd_bh_column_group(c.budget, 100, 1000, c.cols, c.max_group) == c.want);
        CHECK(sd_bh_column_group(BIG, 1, 0, BIG, BIG) == BIG);                             // the whole table at the limit
        CHECK(sd_bh_column_group(BIG, BIG, BIG, 37, 65535) == 1 && sd_bh_column_group(0, BIG, BIG, 37, 65535) == 1);
    }
    {   // the result block of a host entry point (csrc/stagelayout.h): every field on a 256-byte boundary, none overlaps
        // the one before, the block ends where the last field, rounded up, does
        const std::vector<std::vector<int64_t>> layouts = {
            {0},                                                        // a single empty field
            {131, 131 * 8, 131 * 8, 131 * 4, 3 * 131 * 4},              // bytes, then 8-byte elements: they need the alignment
            {1, 0, 255, 256, 257, 8, 131 * 8, 4096, 511, 0, 131, 70 * 70 * 8, 3},       // 13 fields of mixed sizes
        };
        for (const auto& bytes : layouts) {
            const int k = (int)bytes.size();
            std::vector<int64_t> at(bytes.size(), -1);
            const int64_t total = sd_stage_layout(bytes.data(), k, at.data());
            CHECK(at[0] == 0);
            for (int i = 0; i < k; ++i) CHECK(at[i] % 256 == 0);
            for (int i = 1; i < k; ++i) CHECK(at[i] >= at[i - 1] + bytes[i - 1]);
            CHECK(total == at[k - 1] + (bytes[k - 1] + 255) / 256 * 256);
        }
    }
    {   // the launch planners over the sweeps of plan_sweeps.h: every plan keeps inside what the kernels rest on
        int64_t plans = 0, refused = 0, bad = 0;
        sweep_ps(true, [&](const int64_t* k, const SdPsFacts& f) {
            SdPsPlan p;
            const int rc = sd_ps_plan(k, f, &p);
            ++plans;
            if (rc == SDICE_OK) bad += ps_plan_holds(k, f, p);
            else { ++refused; bad += !(rc == SDICE_ERR_ARG && (strstr(g_err, "sdice_ps_dev: row chunk does not fit LDS") || strstr(g_err, "sdice_ps_dev: grid too large"))); }
        });
        CHECK(bad == 0 && refused > 0 && refused < plans / 2);
        sweep_cluster(true, [&](const int64_t* k, const SdClusterFacts& f) {
            SdClusterPlan p;
            CHECK_V(!sd_cluster_takes_legacy(k, f.n));
            sd_cluster_fast_plan(k, f, &p);
            bad += cluster_plan_holds(f, p);
        });
        CHECK(bad == 0);
        {
            Knobs k;
            CHECK(!sd_cluster_takes_legacy(k.v, FAST_MAX_N) && sd_cluster_takes_legacy(k.v, FAST_MAX_N + 1));
            CHECK(sd_cluster_takes_legacy(Knobs().set(SD_P_CLUSTER_LEGACY, 1).v, 1000) && sd_cluster_takes_legacy(Knobs().set(SD_P_CLUSTER_GENERIC, 1).v, 1000));
        }
        plans = refused = 0;
        sweep_bhs(true, [&](const int64_t* k, const SdBhsFacts& f) {
            SdBhsPlan p;
            CHECK_V(sd_bh_cols_supported(f.m, f.segs));
            const int rc = sd_bhs_plan(k, f, &p);
            ++plans;
            if (rc == SDICE_OK) bad += bhs_plan_holds(f, p);
            else { ++refused; bad += !(rc == SDICE_ERR_ARG && strstr(g_err, "sd_bh_cols_samplesort: bh: too many")); }
        });
        CHECK(bad == 0 && refused > 0 && refused < plans / 2);
        CHECK(!sd_bh_cols_supported(((int64_t)1 << POS_SHIFT) + 1, 1) && !sd_bh_cols_supported(0, 1) && !sd_bh_cols_supported(1, 0));
        sweep_bhv(true, [&](const int64_t* k, int64_t n) {
            SdBhvPlan p;
            sd_bhv_plan(k, n, &p);
            bad += bhv_plan_holds(k, n, p);
        });
        CHECK(bad == 0);
        CHECK(!sd_bh_vector_supported(BHV_MIN_N - 1) && !sd_bh_vector_supported(BHV_MAX_N + 1));
    }
    {   // pinned plans, whole structs (fields in the order of the struct): the default knobs at the shapes the benchmark and
        // DESIGN.md name, and one plan per fallback of the PS kernel choice
        auto psf = [](int64_t n, int32_t s, bool aligned, bool reach) {
            SdPsFacts f;
            f.n = n; f.s = s; f.aligned = aligned; f.want_excl = false; f.want_ps = true;
            f.ctx_list = f.reach_rows_match = f.have_reach_words = reach; f.cluster_reach = reach ? 22 : 0;
            return f;
        };
        struct { Knobs k; SdPsFacts f; Vals want; } ps_cases[] = {
            // kern vec cw R H col_cap n_tiles n_chunks lv_shift tiles_per_xcd use_reach nt prio q3 ablate threads lds grid
            {Knobs(), psf(2000000, 500, true, true), {0, 4, 128, 96, 24, 1536, 20834, 4, 1, 2605, 1, 0, 1, 0, 0, 1024, 81920, 83360}},     // 96-row tiles, capacity 24
            {Knobs(), psf(2000000, 500, true, false), {0, 4, 128, 111, 16, 1776, 18019, 4, 1, 2253, 0, 0, 1, 0, 0, 1024, 81920, 72096}},
            {Knobs(), psf(1000000, 100, true, false), {0, 4, 100, 146, 16, 2336, 6850, 1, 0, 857, 0, 1, 1, 0, 0, 1024, 81920, 6856}},
            {Knobs(), psf(625000, 1000, true, false), {0, 4, 128, 111, 16, 1776, 5631, 8, 1, 704, 0, 0, 1, 0, 0, 1024, 81920, 45056}},
            {Knobs(), psf(5000000, 1000, true, false), {0, 4, 128, 111, 16, 1776, 45046, 8, 1, 5631, 0, 0, 1, 0, 0, 1024, 81920, 360384}},
            // the fallbacks to the first-generation kernel (kern 2)
            {Knobs(), psf(1000000, 99, true, false), {2, 1, 99, 148, 16, 2368, 6757, 1, 0, 845, 0, 1, 1, 0, 0, 1024, 81920, 6760}},                  // s % 4 != 0
            {Knobs(), psf(1000000, 100, false, false), {2, 1, 100, 146, 16, 2336, 6850, 1, 0, 857, 0, 1, 1, 0, 0, 1024, 81920, 6856}},               // a misaligned table
            {Knobs().set(SD_P_PS_CHUNK_COLS, 96), psf(2000000, 500, true, false), {2, 4, 96, 153, 16, 2448, 13072, 6, 0, 1634, 0, 0, 1, 0, 0, 1024, 81920, 78432}},
            {Knobs().set(SD_P_PS_THREADS, 64), psf(2000000, 500, true, false), {0, 4, 128, 8, 2, 128, 250000, 4, 1, 31250, 0, 0, 1, 0, 0, 64, 81920, 1000000}},      // (stays register-staged: 8-row tiles)
            {Knobs(), psf(1000, 1 << 19, true, false), {2, 4, 128, 112, 16, 1792, 9, 4096, 1, 0, 0, 0, 1, 0, 0, 1024, 81920, 36864}},                  // s >= 2^19
            {Knobs().set(SD_P_PS_GEN1, 1), psf(1000000, 100, true, true), {2, 4, 100, 146, 16, 2336, 6850, 1, 0, 857, 0, 1, 1, 0, 0, 1024, 81920, 6856}},
        };
        for (const auto& c : ps_cases) { SdPsPlan p; CHECK(sd_ps_plan(c.k.v, c.f, &p) == SDICE_OK && fields(p) == c.want); }
        // B spb S slot_cap lds_cap sample_sort n_tiles zk4 zero cursor rank bmax64 col_done z_alloc slots row spl reserve rank_grid
        // scatter_wg scatter_grid scatter_lds sort_grid nb_grid (4 neighbour workgroups per CU, 256 CUs)
        struct { int64_t n; Vals want; } cl_cases[] = {
            {1000000, {489, 12, 5868, 16360, 8192, 1, 1954, 15648, 103708, 15648, 17604, 41092, 103600, 104732, 128000640, 4000000, 3920, 140177708, 23, 1024, 245, 7824, 489, 1024}},
            {2000000, {977, 12, 11724, 16384, 8192, 1, 3907, 31272, 207300, 31272, 35180, 82092, 207100, 208324, 256114688, 8000000, 7824, 280403156, 46, 1024, 489, 15632, 977, 1024}},
        };
        for (const auto& c : cl_cases) { SdClusterPlan p; sd_cluster_fast_plan(Knobs().v, SdClusterFacts{c.n, 4, 256}, &p); CHECK(fields(p) == c.want); }
        struct { int64_t m, segs; Vals want; } bhs_cases[] = {      // 256 CUs
            {25000, 19900, {256, 45, 2048, 8, 360, 512, 1, 2048, 156, 7, 512, 16, 0, 196, 16224, 139328, 895680, 1024, 1536, 244608, 6144, 900, 11328, 16736, 33120, 16736, 3980000000, 3980000000, 7164000, 7164000, 7164000, 7164000, 3582000, 3582000, 3582000, 3661600, 16, 1990000000, 3980000000}},
            {200000, 200, {256, 356, 2048, 8, 2848, 4096, 0, 2048, 2, 49, 512, 16, 0, 1563, 1568, 9800, 71200, 1024, 1536, 25008, 49152, 7120, 0, 16736, 33120, 16736, 320000000, 320000000, 569600, 569600, 569600, 569600, 284800, 284800, 284800, 285600, 16, 160000000, 320000000}},
        };
        for (const auto& c : bhs_cases) { SdBhsPlan p; CHECK(sd_bhs_plan(Knobs().v, SdBhsFacts{c.m, c.segs, 256}, &p) == SDICE_OK && fields(p) == c.want); }
        {
            SdBhvPlan p;
            sd_bhv_plan(Knobs().v, 1000000, &p);
            CHECK(fields(p) == Vals({489, 5632, 7824, 31, 245, 9780, 73216, 8352, 8344, 33408, 22032384, 8000000, 8000000, 8000000, 3912, 11016192, 4000000, 4000000, 2000000, 2000000, 3912, 1956}) && sd_bhv_scratch(Knobs().v, 1000000) == 69153232);
        }
        {   // the one-bucket rule at its edges (bh.wg 1024: 2049 .. 4096 rows were one bucket before the rule)
            SdBhsPlan p;
            const Knobs wide_wg = Knobs().set(SD_P_BH_WG, 1024);
            CHECK(sd_bhs_plan(wide_wg.v, SdBhsFacts{2048, 9, 256}, &p) == SDICE_OK && p.B == 1 && p.spill_bytes == 0);
            for (int64_t m : {2049, 3000, 4096, 4097})
                CHECK(sd_bhs_plan(wide_wg.v, SdBhsFacts{m, 9, 256}, &p) == SDICE_OK && p.B == 2 && p.spill_bytes == m * 9 * 8);
            CHECK(sd_bhs_plan(Knobs().v, SdBhsFacts{1024, 9, 256}, &p) == SDICE_OK && p.B == 1);
            CHECK(sd_bhs_plan(Knobs().v, SdBhsFacts{1025, 9, 256}, &p) == SDICE_OK && p.B == 2);
        }
    }
    printf("host sanitizer driver: ok\n");
    return 0;
}
