// K16: exact conditional p-values of the rank-sum (K5) and the signed-rank (K13) test on small rows -- compare_sample_sets --exact.
//
// The asymptotic call runs first and fills every output; the kernels here read the rows again from the ps table through
// the column lists (nothing of K5's or K13's intermediate buffers), overwrite p on the eligible tested rows and write
// exact[row] = 1 there, 0 elsewhere.  Everything is an integer up to the one float64 division that gives p.
//
// Rank-sum.  A tested row with N = n1' + n2' <= 32 kept values is eligible (C(32, 16) = 601 080 390 fits 32 bits).
//   doubled mid-rank r_i = 2 #(v_j < v_i) + #(v_j == v_i) + 1 by the order bits of the float32 values (-0.0 == +0.0 one
//       tie group, made with integer operations only: no floating add that a flush-to-zero mode could turn into 0)
//   k = min(n1', n2') (set 1 on a tie), W = doubled rank sum of that set, D = |W - k(N+1)|
//   cnt[j][t] = number of j-subsets of the items seen so far whose doubled rank sum is j(j+1) + t; an item of rank r does
//       cnt[j][t] += cnt[j-1][t + 2j - r] for j descending (each item enters a subset once).  j(j+1) is the smallest sum
//       of j doubled mid-ranks, j(2N-j+1) the largest, so level j uses 2j(N-j)+1 <= 2k(N-k)+1 = Wp words: at 16 v 16
//       17 x 513 words, 34.9 KB.  Only the levels that can still reach k are touched: max(1, k-(N-1-i)) .. min(i+1, k).
//   p = sum of cnt[k][t] over |t + k(k+1) - k(N+1)| >= D  /  sum of cnt[k][t]   (the total is C(N, k))
// Signed-rank.  A tested row with 1 <= n' <= 31 non-zero differences is eligible (2^31 fits 32 bits); n' = 0 keeps p = 1
// and is exact.  The differences are K13's: integer thousandths on a row of 3-decimal PS values, x - y in float32 on any
// other row.  Doubled mid-ranks of |d|, W = doubled rank sum of the positive differences, D = |2W - n'(n'+1)|,
//   cnt[s] += cnt[s - r] for s descending over 0 .. n'(n'+1) (at most 993 words),
//   p = sum of cnt[s] over |2s - n'(n'+1)| >= D  /  2^n'.
//
// Rows and lanes.  A group of G lanes of one wave owns a row, 64 / G rows side by side in a wave; G is the largest power
// of two (8..64) that is not above the widest table line of the launch (Wp, or n'(n'+1)+1), so a 3 v 3 row (4 x 19 words)
// takes 16 lanes and a workgroup of 256 threads 16 such rows.  The lanes of a group walk a table line side by side, lane
// gl the words gl, gl + G, ...: consecutive words, no bank conflict inside a group, and the group's LDS stride is G
// modulo 32 words so that groups side by side start on different banks.  The lanes of a group run in lockstep (one wave,
// group-uniform control flow), so the steps of the recurrence are separated by wave-scope fences only: no workgroup
// barrier, no atomics -- a row has one owner.  LDS per group: 32 keys + 32 ranks + the largest table the launch's
// n1, n2 (m) allow; the workgroup has as many groups as fit 64 KB (one wave for the 16 v 16 table).  The workgroups
// stride over the rows of the table, at most 8 per CU.
#include "common.h"
#include "rowsum.h"

namespace {

constexpr int EX_MAX_N = 32;             // kept values of an eligible rank-sum row
constexpr int EX_MAX_NP = 31;            // non-zero differences of an eligible signed-rank row
constexpr int EX_SLOTS = 32;             // keys (and ranks) a group holds
constexpr int EX_HEAD = 2 * EX_SLOTS;    // words in front of a group's table
constexpr int EX_THREADS = 256;
constexpr int EX_LDS_BYTES = 64 * 1024;

// order-preserving bits of a non-NaN float, either zero as +0.0, by integer operations only (on purpose not rowsum.h's
// f32_ord, whose `v + 0.0f` a flush-to-zero mode could turn into 0)
__device__ __forceinline__ uint32_t ex_ord(float v) {
    uint32_t b = __float_as_uint(v);
    if ((b << 1) == 0u) b = 0u;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the lane group of a thread (its width is a run-time value of the launch: not rowsum.h's LaneGroup<P>)
struct ExGroup {
    int G, gl, g0, grp;                  // lanes, lane in the group, the group's first lane in the wave, group in the workgroup
    unsigned long long mask;
    __device__ __forceinline__ explicit ExGroup(int g) : G(g) {
        const int lane = threadIdx.x & 63;
        gl = lane & (G - 1);
        g0 = lane - gl;
        grp = threadIdx.x / G;
        mask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    }
    // the group's bits of a ballot, and the number of them below this lane
    __device__ __forceinline__ unsigned long long vote(bool b) const { return (__ballot(b) >> g0) & mask; }
    __device__ __forceinline__ int below(unsigned long long m) const { return __popcll(m & ((1ull << gl) - 1ull)); }
    __device__ __forceinline__ uint32_t add(uint32_t v) const {
        for (int ofs = 1; ofs < G; ofs <<= 1) v += (uint32_t)__shfl_xor((int)v, ofs);
        return v;
    }
};

// doubled mid-ranks R[0..cnt) of the codes V[i] >> shift
__device__ __forceinline__ void ex_ranks(const ExGroup& g, const uint32_t* V, int* R, int cnt, int shift) {
    for (int i = g.gl; i < cnt; i += g.G) {
        const uint32_t vi = V[i] >> shift;
        int less = 0, eq = 0;
        for (int j = 0; j < cnt; ++j) {
            const uint32_t vj = V[j] >> shift;
            less += vj < vi ? 1 : 0;
            eq += vj == vi ? 1 : 0;
        }
        R[i] = 2 * less + eq + 1;
    }
}

__global__ void __launch_bounds__(EX_THREADS) exact_ranksum_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                   const int32_t* __restrict__ g1, int n1,
                                                                   const int32_t* __restrict__ g2, int n2, int G, int gpb,
                                                                   int stride, const uint8_t* __restrict__ tested,
                                                                   double* __restrict__ p, uint8_t* __restrict__ exact) {
    extern __shared__ uint32_t ex_lds[];
    const ExGroup g(G);
    uint32_t* V = ex_lds + (size_t)g.grp * stride;       // [32] order bits of the kept values, set 1 first
    int* R = reinterpret_cast<int*>(V + EX_SLOTS);       // [32] doubled mid-ranks
    uint32_t* T = V + EX_HEAD;                           // [k + 1][Wp]
    const int cap = stride - EX_HEAD;
    for (int64_t row = (int64_t)blockIdx.x * gpb + g.grp; row < n; row += (int64_t)gridDim.x * gpb) {
        SD_WAVE_SYNC();                                  // the previous row's readers are done with the group's LDS
        if (!tested[row]) {
            if (g.gl == 0) exact[row] = 0;
            continue;
        }
        const float* prow = ps + row * s;
        int base = 0, c1 = 0;
        for (int set = 0; set < 2; ++set) {
            const int32_t* idx = set ? g2 : g1;
            const int cnt = set ? n2 : n1;
            for (int q0 = 0; q0 < cnt; q0 += G) {
                const int q = q0 + g.gl;
                float v = __builtin_nanf("");
                if (q < cnt) v = prow[idx[q]];
                const bool kept = v == v;
                const unsigned long long m = g.vote(kept);
                const int pos = base + g.below(m);
                if (kept && pos < EX_SLOTS) V[pos] = ex_ord(v);
                base += __popcll(m);
            }
            if (set == 0) c1 = base;
        }
        const int N = base, c2 = N - c1;
        const int k = c1 <= c2 ? c1 : c2;
        const int Wp = 2 * k * (N - k) + 1;
        if (N > EX_MAX_N || k < 3 || (k + 1) * Wp > cap) {   // (the last two cannot happen on a row the rank-sum call tested)
            if (g.gl == 0) exact[row] = 0;
            continue;
        }
        SD_WAVE_SYNC();
        ex_ranks(g, V, R, N, 0);
        for (int e = g.gl; e < (k + 1) * Wp; e += G) T[e] = e == 0 ? 1u : 0u;
        SD_WAVE_SYNC();
        const int m0 = c1 <= c2 ? 0 : c1;                // the smaller set is V[m0 .. m0 + k)
        uint32_t w = 0;
        for (int i = m0 + g.gl; i < m0 + k; i += G) w += (uint32_t)R[i];
        w = g.add(w);
        for (int i = 0; i < N; ++i) {
            const int r = R[i];
            const int jhi = i + 1 < k ? i + 1 : k;
            const int jlo = k - (N - 1 - i) > 1 ? k - (N - 1 - i) : 1;
            for (int j = jhi; j >= jlo; --j) {
                uint32_t* dst = T + j * Wp;
                const uint32_t* src = dst - Wp;
                const int wj = 2 * j * (N - j), sh = 2 * j - r;
                for (int t = g.gl; t <= wj; t += G) {
                    const int u = t + sh;
                    if (u >= 0 && u < Wp) dst[t] += src[u];
                }
                SD_WAVE_SYNC();                          // level j - 1 is read above and written next
            }
        }
        const int centre = k * (N + 1), off = k * (k + 1);
        const int D = (int)w > centre ? (int)w - centre : centre - (int)w;
        uint32_t tail = 0, total = 0;
        for (int t = g.gl; t < Wp; t += G) {
            const uint32_t c = T[k * Wp + t];
            const int dev = t + off - centre;
            total += c;
            if ((dev < 0 ? -dev : dev) >= D) tail += c;
        }
        tail = g.add(tail);
        total = g.add(total);
        if (g.gl == 0) {
            p[row] = (double)tail / (double)total;
            exact[row] = 1;
        }
    }
}

__global__ void __launch_bounds__(EX_THREADS) exact_signedrank_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                      const int32_t* __restrict__ a,
                                                                      const int32_t* __restrict__ b, int m, int G, int gpb,
                                                                      int stride, const uint8_t* __restrict__ tested,
                                                                      double* __restrict__ p, uint8_t* __restrict__ exact) {
    extern __shared__ uint32_t ex_lds[];
    const ExGroup g(G);
    uint32_t* V = ex_lds + (size_t)g.grp * stride;       // [32] K13's keys of the non-zero differences
    int* R = reinterpret_cast<int*>(V + EX_SLOTS);       // [32] doubled mid-ranks of |d|
    uint32_t* T = V + EX_HEAD;                           // [n'(n'+1) + 1]
    const int cap = stride - EX_HEAD;
    for (int64_t row = (int64_t)blockIdx.x * gpb + g.grp; row < n; row += (int64_t)gridDim.x * gpb) {
        SD_WAVE_SYNC();
        if (!tested[row]) {
            if (g.gl == 0) exact[row] = 0;
            continue;
        }
        const float* prow = ps + row * s;
        // a row of 3-decimal PS values or not: every kept value decides
        bool offgrid = false;
        for (int q = g.gl; q < m; q += G) {
            const float x = prow[a[q]], y = prow[b[q]];
            if (x == x && y == y) offgrid = offgrid || !(key_of_ps(x).exact() && key_of_ps(y).exact());
        }
        const bool grid = g.vote(offgrid) == 0ull;
        int np = 0;
        for (int q0 = 0; q0 < m; q0 += G) {
            const int q = q0 + g.gl;
            uint32_t key = PAD32;
            if (q < m) {
                const float x = prow[a[q]], y = prow[b[q]];
                if (x == x && y == y) key = pair_diff_key(x, y, grid);
            }
            const bool valid = key != PAD32;
            const unsigned long long mk = g.vote(valid);
            const int pos = np + g.below(mk);
            if (valid && pos < EX_SLOTS) V[pos] = key;
            np += __popcll(mk);
        }
        const int L = np * (np + 1) + 1;
        if (np == 0 || np > EX_MAX_NP || L > cap) {      // n' = 0: p = 1 already, and that is exact
            if (g.gl == 0) exact[row] = np == 0 ? 1 : 0;
            continue;
        }
        SD_WAVE_SYNC();
        ex_ranks(g, V, R, np, 1);
        for (int e = g.gl; e < L; e += G) T[e] = e == 0 ? 1u : 0u;
        SD_WAVE_SYNC();
        uint32_t w = 0;
        for (int i = g.gl; i < np; i += G) w += (V[i] & 1u) ? (uint32_t)R[i] : 0u;
        w = g.add(w);
        int top = 0;                                     // the largest sum the items so far reach
        for (int i = 0; i < np; ++i) {
            const int r = R[i];
            top += r;
            // downwards in pieces of G words: a piece reads itself and words below it, which later pieces write
            for (int s0 = (top / G) * G; s0 + G > r; s0 -= G) {
                const int sum = s0 + g.gl;
                if (sum >= r && sum <= top) T[sum] += T[sum - r];
                SD_WAVE_SYNC();
            }
        }
        const int full = np * (np + 1);
        const int d2 = 2 * (int)w - full, D = d2 < 0 ? -d2 : d2;
        uint32_t tail = 0, total = 0;
        for (int sum = g.gl; sum < L; sum += G) {
            const uint32_t c = T[sum];
            const int dev = 2 * sum - full;
            total += c;
            if ((dev < 0 ? -dev : dev) >= D) tail += c;
        }
        tail = g.add(tail);
        total = g.add(total);
        if (g.gl == 0) {
            p[row] = (double)tail / (double)total;
            exact[row] = 1;
        }
    }
}

// Host: the lane group, the groups per workgroup, the LDS words per group and the grid of a launch whose largest table
// has `words` words in lines of `width` words
struct ExPlan {
    int G, gpb, stride;
    int64_t blocks;
    size_t lds;
};
ExPlan ex_plan(const sdice_ctx* ctx, int64_t n, int words, int width) {
    ExPlan pl;
    pl.G = 8;
    while (pl.G < 64 && pl.G * 2 <= width) pl.G *= 2;
    pl.stride = EX_HEAD + words;
    while (pl.stride % 32 != pl.G % 32) ++pl.stride;     // groups side by side start G banks apart
    const int per_wave = 64 / pl.G;
    const int fit = EX_LDS_BYTES / (pl.stride * 4);      // >= 1: the largest table is 17 x 513 words
    pl.gpb = std::min(EX_THREADS / pl.G, std::max(fit / per_wave, 1) * per_wave);
    pl.blocks = row_launch_blocks(ctx, sd_ceil_div(n, pl.gpb));
    pl.lds = (size_t)pl.gpb * pl.stride * 4;
    return pl;
}

int ex_launch_ranksum(sdice_ctx* ctx, int64_t n, int s, const float* d_ps, const int32_t* d_g1, int n1, const int32_t* d_g2,
                      int n2, const uint8_t* d_tested, double* d_p, uint8_t* d_exact) {
    // the largest table of an eligible row: N <= min(n1 + n2, 32) kept values, k <= min(n1, n2, N / 2) in the smaller set
    const int N = std::min(n1 + n2, EX_MAX_N), k = std::min(std::min(n1, n2), N / 2);
    const int width = 2 * k * (N - k) + 1;
    const ExPlan pl = ex_plan(ctx, n, (k + 1) * width, width);
    SD_ARG(pl.lds <= (size_t)EX_LDS_BYTES, "the exact table does not fit the LDS");
    SD_LAUNCH(ctx, "exact_ranksum_kernel", exact_ranksum_kernel, dim3((unsigned)pl.blocks), dim3(pl.gpb * pl.G), pl.lds, d_ps, n,
              s, d_g1, n1, d_g2, n2, pl.G, pl.gpb, pl.stride, d_tested, d_p, d_exact);
    return SDICE_OK;
}

int ex_launch_signedrank(sdice_ctx* ctx, int64_t n, int s, const float* d_ps, const int32_t* d_a, const int32_t* d_b, int m,
                         const uint8_t* d_tested, double* d_p, uint8_t* d_exact) {
    const int np = std::min(m, EX_MAX_NP), width = np * (np + 1) + 1;
    const ExPlan pl = ex_plan(ctx, n, width, width);
    SD_ARG(pl.lds <= (size_t)EX_LDS_BYTES, "the exact table does not fit the LDS");
    SD_LAUNCH(ctx, "exact_signedrank_kernel", exact_signedrank_kernel, dim3((unsigned)pl.blocks), dim3(pl.gpb * pl.G), pl.lds,
              d_ps, n, s, d_a, d_b, m, pl.G, pl.gpb, pl.stride, d_tested, d_p, d_exact);
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_ranksum_exact_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_g1,
                                       int32_t n1, const int32_t* d_g2, int32_t n2, uint8_t* d_tested, double* d_p,
                                       double* d_z, float* d_med1, float* d_med2, float* d_mean1, float* d_mean2,
                                       float* d_delta, uint8_t* d_exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0 && n1 >= 0 && n2 >= 0, "negative size");
    if (n == 0) return SDICE_OK;
    SD_ARG(d_exact, "NULL output");
    SD_ARG(std::max(n1, n2) <= 4096, "group larger than 4096 samples is not supported");
    SD_TRY(sdice_ranksum_dev(ctx, n, s, d_ps, d_g1, n1, d_g2, n2, d_tested, d_p, d_z, d_med1, d_med2, d_mean1, d_mean2, d_delta));
    if (n1 < 3 || n2 < 3) {
        SD_HIP(hipMemsetAsync(d_exact, 0, (size_t)n, ctx->stream));
        return SDICE_OK;
    }
    return ex_launch_ranksum(ctx, n, s, d_ps, d_g1, n1, d_g2, n2, d_tested, d_p, d_exact);
}

extern "C" int sdice_ranksum_exact(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* g1, int32_t n1,
                                   const int32_t* g2, int32_t n2, uint8_t* tested, double* p, double* z, float* med1,
                                   float* med2, float* mean1, float* mean2, float* delta, uint8_t* exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0 && n1 >= 0 && n2 >= 0, "negative size");
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med1 && med2 && mean1 && mean2 && delta && exact, "NULL output");
    SD_ARG((n1 == 0 || g1) && (n2 == 0 || g2), "NULL group index");
    SD_ARG(std::max(n1, n2) <= 4096, "group larger than 4096 samples is not supported");
    for (int i = 0; i < n1; ++i) SD_ARG(g1[i] >= 0 && g1[i] < s, "g1 index out of range");
    for (int i = 0; i < n2; ++i) SD_ARG(g2[i] >= 0 && g2[i] < s, "g2 index out of range");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    TwoSampleOut o;
    uint8_t* d_exact;
    float* d_ps;
    int32_t *dg1, *dg2;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dg1, g1, n1));
    SD_TRY(st.upload(&dg2, g2, n2));
    SD_TRY(stage_two_sample(st, n, {tested, p, z, med1, med2, mean1, mean2, delta}, &o, exact, &d_exact));
    SD_TRY(sdice_ranksum_exact_dev(ctx, n, s, d_ps, dg1, n1, dg2, n2, o.tested, o.p, o.z, o.med1, o.med2, o.mean1, o.mean2,
                                   o.delta, d_exact));
    return st.download_results();
}

extern "C" int sdice_signedrank_exact_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a,
                                          const int32_t* d_b, int32_t m, uint8_t* d_tested, double* d_p, double* d_z,
                                          float* d_med1, float* d_med2, float* d_mean1, float* d_mean2, float* d_delta,
                                          uint8_t* d_exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n == 0 || d_exact, "NULL output");
    SD_TRY(sdice_signedrank_dev(ctx, n, s, d_ps, d_a, d_b, m, d_tested, d_p, d_z, d_med1, d_med2, d_mean1, d_mean2, d_delta));
    if (n == 0) return SDICE_OK;
    if (m < 3) {
        SD_HIP(hipMemsetAsync(d_exact, 0, (size_t)n, ctx->stream));
        return SDICE_OK;
    }
    return ex_launch_signedrank(ctx, n, s, d_ps, d_a, d_b, m, d_tested, d_p, d_exact);
}

extern "C" int sdice_signedrank_exact(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a,
                                      const int32_t* b, int32_t m, uint8_t* tested, double* p, double* z, float* med1,
                                      float* med2, float* mean1, float* mean2, float* delta, uint8_t* exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    if (m > 4096) {
        sdice_set_error("sdice_signedrank_exact: %d pairs, at most %d are supported", (int)m, 4096);
        return SDICE_ERR_ARG;
    }
    SD_ARG(m >= 1, "the number of pairs must be 1..4096");
    SD_ARG(a && b, "pair index list is NULL");
    SD_TRY(check_columns(__func__, {a, b}, m, s, "column index out of range", "a column may appear once over both pair lists"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med1 && med2 && mean1 && mean2 && delta && exact, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    TwoSampleOut o;
    uint8_t* d_exact;
    float* d_ps;
    int32_t *da, *db;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&da, a, m));
    SD_TRY(st.upload(&db, b, m));
    SD_TRY(stage_two_sample(st, n, {tested, p, z, med1, med2, mean1, mean2, delta}, &o, exact, &d_exact));
    SD_TRY(sdice_signedrank_exact_dev(ctx, n, s, d_ps, da, db, m, o.tested, o.p, o.z, o.med1, o.med2, o.mean1, o.mean2, o.delta,
                                      d_exact));
    return st.download_results();
}
