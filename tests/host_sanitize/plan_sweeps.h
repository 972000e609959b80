// The inputs the launch planners (csrc/psplan.cpp, clusterplan.cpp, bhplan.cpp) are walked over: sizes and knobs on both
// sides of every bound the plans have.  `wide` adds knob values beyond 32 bits (INT64_MAX edges), which only the
// invariants are checked on.  A sweep calls f(params, facts) for every input.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include <vector>
#include "params.h"
#include "ps.h"
#include "cluster.h"
#include "bh.h"

struct Knobs {
    int64_t v[SD_P_COUNT];
    Knobs() { for (int i = 0; i < SD_P_COUNT; ++i) v[i] = kSdParams[i].dflt; }
    Knobs& set(SdParam k, int64_t x) { v[k] = x; return *this; }
};
typedef std::vector<int64_t> Vals;
static inline Vals with_wide(Vals v, bool wide) {
    if (wide) { v.push_back(INT64_MAX); v.push_back(((int64_t)1 << 31) + 1); v.push_back(INT64_MIN + 1); }
    return v;
}

template <class F> void sweep_ps(bool wide, F f) {
    const int64_t I31 = ((int64_t)1 << 31) - 1;
    const Vals ns = {1, 7, 95, 96, 97, 1000, 625000, I31};
    const Vals ss = {1, 3, 4, 5, 8, 64, 100, 128, 252, 256, 257, 260, 500, 1000, 1024, 4096, 16384,
                     (1 << 19) - 4, 1 << 19, (1 << 19) + 4, I31 - 2, I31};
    struct Reach { bool list, match, words; int reach; };
    const Reach reaches[] = {{false, false, false, 0}, {true, false, false, 5}, {true, false, true, 40}, {true, true, true, 22},
                             {true, true, false, 0}, {false, true, true, 3}};
    auto facts = [&](const Knobs& k, const Vals& n_list, const Vals& s_list) {
        for (int64_t n : n_list) for (int64_t s : s_list) for (int al = 0; al < 2; ++al) for (const Reach& r : reaches) {
            SdPsFacts x;
            x.n = n; x.s = (int32_t)s; x.aligned = al != 0; x.want_excl = false; x.want_ps = true;
            x.ctx_list = r.list; x.reach_rows_match = r.match; x.have_reach_words = r.words; x.cluster_reach = r.reach;
            f(k.v, x);
        }
    };
    // one knob at a time, every size
    facts(Knobs(), ns, ss);
    struct { SdParam k; Vals v; } singles[] = {
        {SD_P_PS_LDS_BYTES, with_wide({-1, 0, 8191, 8192, 8193, 40960, 163839, 163840, 163841}, wide)},
        {SD_P_PS_TILE_ROWS, with_wide({-1, 1, 7, 15, 16, 17, 96, 2047, 2048, 2049, 4096}, wide)},
        {SD_P_PS_THREADS, with_wide({-1, 0, 63, 64, 65, 128, 512, 1000, 1023, 1025, 4096}, wide)},
        {SD_P_PS_CHUNK_COLS, with_wide({-1, 1, 3, 4, 8, 12, 96, 128, 256, 260, 1024, 4096}, wide)},
        {SD_P_PS_HALO_ROWS, with_wide({-2, 0, 1, 15, 16, 17, 64, 1024, 1 << 20, (1 << 20) + 1}, wide)},
        {SD_P_PS_XCD_REMAP, {0}}, {SD_P_PS_ABLATE, {1, 8}}, {SD_P_PS_QUANTIZE3, {1}}, {SD_P_PS_PRIO, {0}},
        {SD_P_PS_NT_LOADS, {0}}, {SD_P_PS_GEN1, {1}}, {SD_P_PS_USE_REACH, {0}},
    };
    for (const auto& sg : singles) for (int64_t x : sg.v) facts(Knobs().set(sg.k, x), ns, ss);
    // the knobs that shape a tile, crossed, both kernel generations
    const Vals ns2 = {7, 1000, I31}, ss2 = {4, 100, 128, 256, 260, 500, 1000, 4096, 1 << 19};
    for (int64_t lds : {8192, 81920, 163840}) for (int64_t th : {64, 256, 1024}) for (int64_t ch : {0, 4, 96, 128, 256})
        for (int64_t tr : {0, 1, 96, 4096}) for (int64_t h : {-1, 0, 64}) for (int64_t g1 : {0, 1})
            facts(Knobs().set(SD_P_PS_LDS_BYTES, lds).set(SD_P_PS_THREADS, th).set(SD_P_PS_CHUNK_COLS, ch)
                      .set(SD_P_PS_TILE_ROWS, tr).set(SD_P_PS_HALO_ROWS, h).set(SD_P_PS_GEN1, g1), ns2, ss2);
}

template <class F> void sweep_cluster(bool wide, F f) {
    const Vals ns = {1, 2, 127, 128, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4096, 1 << 19, (1 << 19) + 1, 1000000,
                     (2 << 20) - 1, 2 << 20, (2 << 20) + 1, FAST_MAX_N - 1, FAST_MAX_N};
    for (int64_t bm : with_wide({-1, 0, 255, 256, 257, 1000, 2047, 2048, 2049}, wide))
        for (int64_t spb : with_wide({-1, 0, 1, 2, 3, 12, 64, 65}, wide))
            for (int64_t lc : with_wide({-5, 0, 1, 2, 3, 8191, 8192, 8193}, wide))
                for (int64_t nbg : with_wide({-1, 0, 1, 7, 100000}, wide))
                    for (int64_t ss : {0, 1}) for (int dev = 0; dev < 2; ++dev) for (int64_t n : ns) {
                        const int per_cu = dev ? 4 : 1, n_cu = dev ? 256 : 1;
                        Knobs k;
                        k.set(SD_P_CLUSTER_BUCKET_MEAN, bm).set(SD_P_CLUSTER_SPB, spb).set(SD_P_CLUSTER_LDS_CAP, lc)
                            .set(SD_P_CLUSTER_NB_GRID, nbg).set(SD_P_CLUSTER_SAMPLE_SORT, ss);
                        f(k.v, SdClusterFacts{n, per_cu, n_cu});
                    }
}

template <class F> void sweep_bhs(bool wide, F f) {
    const int64_t M = (int64_t)1 << POS_SHIFT, I31 = ((int64_t)1 << 31) - 1;
    const Vals ms = {1, 2, 3, 15, 16, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 2252, 2253, 3000, 4095, 4096, 4097,
                     4504, 4505, 5000, 8191, 8192, 8193, 16384, 25000, 200000, M - 1, M};
    const Vals segs = {1, 3, 8, 9, 16, 17, 200, 19900, 1 << 20, I31 - 16, I31};
    auto facts = [&](const Knobs& k, const Vals& m_list, const Vals& seg_list) {
        for (int64_t m : m_list) for (int64_t sg : seg_list) for (int n_cu : {1, 256}) f(k.v, SdBhsFacts{m, sg, n_cu});
    };
    for (int64_t wg : with_wide({-1, 0, 256, 511, 512, 1023, 1024, 4096}, wide))
        for (int64_t mean : with_wide({-1, 0, 1, 2, 3, 100, 563, 900, 2252, 2500, 3000, 5000, 1 << 20}, wide))
            for (int64_t spb : with_wide({-1, 0, 1, 2, 8, 9, 64, 4096, 8192, 10000}, wide))
                facts(Knobs().set(SD_P_BH_WG, wg).set(SD_P_BH_MEAN, mean).set(SD_P_BH_SPB, spb), ms, {1, 9, 19900, I31});
    struct { SdParam k; Vals v; } singles[] = {
        {SD_P_BH_REG_CAP, with_wide({-1, 0, 1, 64, 2047, 2048, 2049}, wide)},
        {SD_P_BH_ROWS_PER_BLOCK, with_wide({-1, 0, 1, 127, 128, 129, 2048, 1 << 20}, wide)},
        {SD_P_BH_FUSED_COUNT, {0, 1}}, {SD_P_BH_FINISH_COLS, {0, 8, 15, 16, 17}}, {SD_P_BH_FINISH_NT, {0, 1}},
        {SD_P_BH_BIG_WG, {0, 256, 511, 512, 1024}},
    };
    for (const auto& sg : singles) for (int64_t x : sg.v) for (int64_t wg : {256, 512, 1024})
        facts(Knobs().set(sg.k, x).set(SD_P_BH_WG, wg), ms, segs);
}

// every supported length at the default knobs; the knobs at chosen lengths
template <class F> void sweep_bhv(bool wide, F f) {
    const Knobs dflt;
    for (int64_t n = BHV_MIN_N; n <= BHV_MAX_N; ++n) f(dflt.v, n);
    const Vals ns = {BHV_MIN_N, BHV_MIN_N + 1, 20000, 65536, 100003, 262144, 524287, 524288, 524289, 700001, 1 << 20,
                     (1 << 20) + 1, BHV_MAX_N - 1, BHV_MAX_N};
    for (int64_t mean : with_wide({-1, 0, 1, 511, 512, 513, 1024, 2047, 2048, 2049, 4096, 1 << 20}, wide))
        for (int64_t cap : with_wide({-1, 0, 63, 64, 65, 512, 5632, 6143, 6144, 6145}, wide))
            for (int64_t n : ns) f(Knobs().set(SD_P_BHV_MEAN, mean).set(SD_P_BHV_CAP, cap).v, n);
}
