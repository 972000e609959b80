// K21: Friedman's test and Page's L trend test per junction row across k MATCHED sample sets (sdice_friedman, sdice_page).
//
// cols is set-major: cols[j m + q] is the column of set j for subject q (its "block" of k values).  A block is kept when
// all k of its values are non-NaN; with fewer than 3 kept blocks (m') the row is not tested.  Per set the np.mean and
// np.median of its values over the kept blocks in subject order, bit for bit as the k-set tests report them.
//
// Arithmetic, in integers up to the last division.  Ranks are taken INSIDE a block:
//   r2(q, j) = 2 #{l: x_ql < x_qj} + #{l: x_ql == x_qj} + 1         (twice the mid-rank; float32 compares: -0.0 == +0.0)
//   D_j = sum_q r2(q, j) - m' (k + 1)                                (= 2 R_j - m' (k + 1);  sum_j D_j = 0)
//   C   = sum over the elements of (t^2 - 1), t the size of the element's tie group in its block  (= sum (t^3 - t))
//   den = m' (k^3 - k) - C
// Friedman:  Q = 3 (k - 1) sum D_j^2 / den,  W = 3 sum D_j^2 / (m' den)  -- every numerator and divisor is an exact float64
//            (3 (k - 1) sum D^2 < 2^50, m' den < 2^43), each statistic is ONE correctly rounded division;
//            p = chi2.sf(Q, k - 1) by kw_chi2_sf (rowsum.h).
// Page:      L = sum_j (j + 1) R_j (2 L is an integer);  A = 6 sum_j (j + 1) D_j,  B = k (k + 1) den,  z = A / sqrt(B): the
//            conditional (within-block permutation) variance given the row's ties, no continuity correction; two correctly
//            rounded operations, so z is within 2 ulp of the correctly rounded value; A == 0 gives +0.0 by a test on the
//            integer.  Reversing the sets negates A and nothing else.  p = erfc(|z| / sqrt 2) as the rank-sum path has it.
// den == 0 (every kept block fully tied): Q = W = z = 0, p = 1, the row stays tested.
// No PS value is ever subtracted from another, so a row of 3-decimal values and its off-grid image under an increasing
// map give the same integers; there is no separate path for rows on the grid, and none is needed: a block has at most 64
// values and its ranks come from k float compares per element, not from a histogram of the row.
//
// One kernel, friedman_kernel<PAGE, TEAM>: a team of TEAM waves owns a row.  TEAM = 1: every wave of the workgroup walks
// rows of its own in its own slice of the LDS and the team's barrier is a wave barrier; TEAM = 4: the workgroup is the
// team.  The host planner (fr_plan) takes the wave form while the staged row has at most `friedman.wave_max` values.
// (Several rows side by side in one wave, for rows of a few dozen values, is not built: nothing in this file would be
// shared with it; profiles/friedman_times.json holds what the one-row wave form costs on rows of 32 to 64 values.)
// Steps of a row, LDS: keepM[ceil(m / 64)] u64 | F[k][Pm] (Pm = m rounded up to a power of two) | r2S[k] | C | means, medians |
// per wave the leaves of the pairwise sum:
//   1. stage the k m selected values as floats, F[j][q], NaN from q = m on;
//   2. keepM: bit q of the block-complete mask, 64 subjects per ballot;
//   3. a wave per set: ordered compaction of the set's row of F by keepM (in place: a value moves to a slot at or below its
//      own, a round of 64 reads before it writes), NaN from m' on, numpy's pairwise sum -> the mean;
//   4. ranks, cut over the (set, block) elements: each takes the k values of its block (column q of F), adds r2 to its set's
//      integer in LDS and t^2 - 1 to C -- integer adds, so no result depends on an order of arrival and permuting sets or
//      subjects leaves Q, W, p and |z| bit for bit;
//   5. F becomes order bits (NaN: the padding) and every set's row is sorted by one bitonic network over all rows at once
//      -> the medians;
//   6. the team's first wave, set j in lane j: D_j, the sums over the lanes, the statistic, the stores.
#include "common.h"
#include <math.h>
#include <algorithm>
#include "rowsum.h"

namespace {

constexpr int FR_TEAM = RB_THREADS / 64;     // waves of the workgroup form
static_assert(KW_MAX_SETS <= 64, "set j lives in lane j of the epilogue");

struct FrOut {
    uint8_t* tested;
    double* p;
    double* a;           // Friedman: Q (may be NULL); Page: z
    double* b;           // Friedman: W; Page: L (may be NULL)
    int32_t* blocks;     // may be NULL
    float* med;          // [k][n]
    float* mean;         // [k][n]
    float* delta;
};

template <int TEAM>
__device__ __forceinline__ void fr_sync() {
    if constexpr (TEAM == 1) SD_WAVE_SYNC();
    else __syncthreads();
}

__device__ __forceinline__ long long fr_wave_sum(long long v) {
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs);
    return v;
}

template <bool PAGE, int TEAM>
__global__ void __launch_bounds__(RB_THREADS) friedman_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                              const int32_t* __restrict__ cols, int k, int m, int lg,
                                                              int leaf_cap, int tstride, FrOut o) {
    extern __shared__ __align__(16) unsigned char smemf[];
    constexpr int TN = TEAM * 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tw = TEAM == 1 ? 0 : wave;                             // this wave in its team
    const int tl = TEAM == 1 ? lane : (int)threadIdx.x;              // this thread in its team
    const int teams = TEAM == 1 ? (int)(blockDim.x >> 6) : 1;        // teams of the workgroup
    const int Pm = 1 << lg, nsel = k << lg, nr = (m + 63) >> 6;
    unsigned char* base = smemf + (size_t)(TEAM == 1 ? wave : 0) * tstride;
    unsigned long long* keepM = reinterpret_cast<unsigned long long*>(base);
    float* F = reinterpret_cast<float*>(keepM + nr);
    uint32_t* U = reinterpret_cast<uint32_t*>(F);
    unsigned* r2S = U + nsel;
    unsigned* tieS = r2S + k;
    float* meanS = reinterpret_cast<float*>(tieS + 1);
    float* medS = meanS + k;
    float* leaf_sum = medS + k + tw * (2 * leaf_cap + 1);
    int* leaf_off = reinterpret_cast<int*>(leaf_sum + leaf_cap);
    const float nanv = __builtin_nanf("");
    for (int64_t row = (int64_t)blockIdx.x * teams + (TEAM == 1 ? wave : 0); row < n; row += (int64_t)gridDim.x * teams) {
        const float* prow = ps + row * s;
        fr_sync<TEAM>();         // the previous row's readers are done with the team's LDS
        // ---- 1. stage
        for (int e = tl; e < nsel; e += TN) {
            const int j = e >> lg, q = e & (Pm - 1);
            float v = nanv;
            if (q < m) v = __builtin_nontemporal_load(prow + cols[j * m + q]);
            F[e] = v;
        }
        if (tl < k) r2S[tl] = 0u;
        if (tl == 0) *tieS = 0u;
        fr_sync<TEAM>();
        // ---- 2. the block-complete mask
        for (int r = tw; r < nr; r += TEAM) {
            const int q = (r << 6) + lane;
            bool c = q < m;
            if (c)
                for (int j = 0; j < k; ++j) {
                    const float v = F[(j << lg) + q];
                    c = c && v == v;
                }
            const unsigned long long mask = __ballot(c);
            if (lane == 0) keepM[r] = mask;
        }
        fr_sync<TEAM>();
        int mk = 0;
        for (int r = 0; r < nr; ++r) mk += __popcll(keepM[r]);
        if (mk < 3) {            // team-uniform: the row is not tested
            if (tw == 0) {
                if (lane < k) {
                    o.med[(int64_t)lane * n + row] = 0.f;
                    o.mean[(int64_t)lane * n + row] = 0.f;
                }
                if (lane == 0) {
                    o.tested[row] = 0; o.p[row] = 0.0; o.delta[row] = 0.f;
                    if (o.a) o.a[row] = 0.0;
                    if (o.b) o.b[row] = 0.0;
                    if (o.blocks) o.blocks[row] = 0;
                }
            }
            continue;
        }
        // ---- 3. a wave per set: compaction in subject order, the mean
        for (int j = tw; j < k; j += TEAM) {
            float* R = F + (j << lg);
            int at = 0;
            for (int r = 0; r < nr; ++r) {
                const unsigned long long mask = keepM[r];
                const bool kept = (mask >> lane) & 1ull;
                const float v = kept ? R[(r << 6) + lane] : 0.f;
                SD_WAVE_SYNC();
                if (kept) R[lanes_below(mask, at)] = v;
                at += __popcll(mask);
            }
            SD_WAVE_SYNC();
            for (int q = mk + lane; q < Pm; q += 64) R[q] = nanv;
            SD_WAVE_SYNC();
            // np.mean: the identity 0 plus the pairwise tree (m' <= 4096: one piece of np.add.reduce)
            const float sum = 0.0f + wave_pairwise_sum<PW_DEPTH>(FloatAt{R}, mk, lane, leaf_off, leaf_sum);
            if (lane == 0) meanS[j] = sum / (float)mk;
        }
        fr_sync<TEAM>();
        // ---- 4. ranks inside the blocks
        {
            unsigned tie = 0;
            for (int e = tl; e < nsel; e += TN) {
                const int j = e >> lg, q = e & (Pm - 1);
                if (q < mk) {
                    const float x = F[e];
                    unsigned lt = 0, eq = 0;
                    for (int l = 0; l < k; ++l) {
                        const float y = F[(l << lg) + q];
                        lt += y < x ? 1u : 0u;
                        eq += y == x ? 1u : 0u;
                    }
                    atomicAdd(&r2S[j], 2u * lt + eq + 1u);       // at most 4096 (2 * 64 + 1) per set
                    tie += eq * eq - 1u;                         // at most 16384 * 4095 per row
                }
            }
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) tie += __shfl_xor(tie, ofs);
            if (lane == 0 && tie) atomicAdd(tieS, tie);
        }
        fr_sync<TEAM>();
        // ---- 5. order bits, every set's row sorted, the medians
        for (int e = tl; e < nsel; e += TN) {
            const float v = F[e];
            U[e] = v == v ? f32_ord(v) : PAD32;
        }
        fr_sync<TEAM>();
        for (int kk = 2; kk <= Pm; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                for (int i = tl; i < nsel; i += TN) {
                    const int l = i ^ jj;
                    if (l > i) {
                        const bool asc = ((i & (Pm - 1)) & kk) == 0;         // kk == Pm: ascending in every row
                        const uint32_t x = U[i], y = U[l];
                        if ((x > y) == asc) { U[i] = y; U[l] = x; }
                    }
                }
                fr_sync<TEAM>();
            }
        }
        if (tl < k) medS[tl] = median_of_ord(U + (tl << lg), mk);            // np.median on float32
        fr_sync<TEAM>();
        // ---- 6. the statistic
        if (tw == 0) {
            long long D = 0, r2 = 0;
            float my_med = 0.f;
            if (lane < k) {
                r2 = (long long)r2S[lane];
                D = r2 - (long long)mk * (k + 1);
                my_med = medS[lane];
                o.med[(int64_t)lane * n + row] = my_med;
                o.mean[(int64_t)lane * n + row] = meanS[lane];
            }
            const float inf = __builtin_inff();
            const float dl = kw_wave_max(lane < k ? my_med : -inf) - kw_wave_min(lane < k ? my_med : inf);
            const long long den = (long long)mk * ((long long)k * k * k - k) - (long long)*tieS;
            double a = 0.0, b = 0.0, p = 1.0;
            if constexpr (PAGE) {
                const long long A = 6 * fr_wave_sum((long long)(lane + 1) * D);
                const long long L2 = fr_wave_sum((long long)(lane + 1) * r2);
                if (den != 0 && A != 0) {
                    a = (double)A / sqrt((double)((long long)k * (k + 1) * den));
                    p = erfc(fabs(a) * 0.70710678118654752440);
                }
                b = 0.5 * (double)L2;
            } else {
                const long long S = fr_wave_sum(D * D);
                if (den != 0) {
                    a = (double)(3 * (long long)(k - 1) * S) / (double)den;
                    b = (double)(3 * S) / (double)((long long)mk * den);
                    p = kw_chi2_sf(a, k - 1);
                }
            }
            if (lane == 0) {
                o.tested[row] = 1; o.p[row] = p; o.delta[row] = dl;
                if (o.a) o.a[row] = a;
                if (o.b) o.b[row] = b;
                if (o.blocks) o.blocks[row] = mk;
            }
        }
    }
}

// Host: the launch plan of a call -- the padded set length, the leaves of the pairwise sum, the team form and the LDS
struct FrPlan {
    int lg, leaf_cap, team, waves, tstride;
    size_t lds;
};
inline FrPlan fr_plan(int k, int m, int64_t wave_max) {
    FrPlan pl;
    pl.lg = 1;
    while ((1 << pl.lg) < m) ++pl.lg;                // Pm >= 2
    const int64_t nsel = (int64_t)k << pl.lg;        // below 2 * KW_MAX_N
    // leaves of numpy's pairwise recursion over m values: after d halvings a part is at most m / 2^d + 15 long, a leaf
    // from 128 down (rowsum.h, kw_plan)
    pl.leaf_cap = 1;
    while (pl.leaf_cap < (1 << PW_DEPTH) && m > 113 * pl.leaf_cap) pl.leaf_cap <<= 1;
    pl.team = nsel <= wave_max ? 1 : FR_TEAM;
    const int nr = (m + 63) / 64;
    pl.tstride = (int)((8 * nr + 4 * nsel + 4 * (3 * k + 1) + pl.team * 4 * (2 * pl.leaf_cap + 1) + 15) & ~(int64_t)15);
    const int fit = 64 * 1024 / pl.tstride;          // wave form: the workgroup is sized from the LDS a wave needs
    pl.waves = pl.team == 1 ? std::min(FR_TEAM, std::max(1, fit)) : FR_TEAM;
    pl.lds = (size_t)(pl.team == 1 ? pl.waves : 1) * pl.tstride;
    return pl;
}

template <bool PAGE>
int fr_dev(const char* fn, sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t k, int32_t m,
           const FrOut& o) {
    SD_ARG_AS(fn, ctx, "ctx is NULL");
    SD_ARG_AS(fn, n >= 0 && s >= 0, "negative size");
    SD_TRY(fr_check_sets(fn, nullptr, k, m, s));
    if (n == 0) return SDICE_OK;
    SD_ARG_AS(fn, o.tested && o.p && o.med && o.mean && o.delta && (!PAGE || o.a), "NULL output");
    SD_ARG_AS(fn, d_ps && d_cols, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const FrPlan pl = fr_plan(k, m, ctx->param(SD_P_FRIEDMAN_WAVE_MAX));
    if (pl.team == 1) {
        auto kern = friedman_kernel<PAGE, 1>;
        SD_LAUNCH_LDS(ctx, PAGE ? "page_wave_kernel" : "friedman_wave_kernel", kern,
                      dim3((unsigned)wave_launch_blocks(ctx, n, 1, pl.waves)), dim3(pl.waves * 64), pl.lds, d_ps, n, s, d_cols, k, m,
                      pl.lg, pl.leaf_cap, pl.tstride, o);
    } else {
        auto kern = friedman_kernel<PAGE, FR_TEAM>;
        SD_LAUNCH_LDS(ctx, PAGE ? "page_block_kernel" : "friedman_block_kernel", kern, dim3((unsigned)row_launch_blocks(ctx, n)),
                      dim3(RB_THREADS), pl.lds, d_ps, n, s, d_cols, k, m, pl.lg, pl.leaf_cap, pl.tstride, o);
    }
    return SDICE_OK;
}

template <bool PAGE>
int fr_host(const char* fn, sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t k, int32_t m,
            const FrOut& h) {
    SD_ARG_AS(fn, ctx, "ctx is NULL");
    SD_ARG_AS(fn, n >= 0 && s >= 0, "negative size");
    SD_ARG_AS(fn, cols, "cols is NULL");
    SD_TRY(fr_check_sets(fn, cols, k, m, s));
    if (n == 0) return SDICE_OK;
    SD_ARG_AS(fn, h.tested && h.p && h.med && h.mean && h.delta && (!PAGE || h.a), "NULL output");
    SD_ARG_AS(fn, ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t* dcols;
    FrOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dcols, cols, (int64_t)k * m));
    st.result(&d.tested, h.tested, n);
    st.result(&d.p, h.p, n);
    st.result(&d.a, h.a, n);
    st.result(&d.b, h.b, n);
    st.result(&d.blocks, h.blocks, n);
    st.result(&d.med, h.med, (int64_t)k * n);        // [k][n]
    st.result(&d.mean, h.mean, (int64_t)k * n);
    st.result(&d.delta, h.delta, n);
    SD_TRY(st.alloc_results());
    SD_TRY(fr_dev<PAGE>(fn, ctx, n, s, d_ps, dcols, k, m, d));
    return st.download_results();
}

}  // namespace

extern "C" int sdice_friedman_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t k,
                                  int32_t m, uint8_t* d_tested, double* d_p, double* d_q, double* d_w, int32_t* d_blocks,
                                  float* d_med, float* d_mean, float* d_delta) {
    return fr_dev<false>(__func__, ctx, n, s, d_ps, d_cols, k, m, FrOut{d_tested, d_p, d_q, d_w, d_blocks, d_med, d_mean, d_delta});
}

extern "C" int sdice_friedman(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t k, int32_t m,
                              uint8_t* tested, double* p, double* q, double* w, int32_t* blocks, float* med, float* mean,
                              float* delta) {
    return fr_host<false>(__func__, ctx, n, s, ps, cols, k, m, FrOut{tested, p, q, w, blocks, med, mean, delta});
}

extern "C" int sdice_page_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t k,
                              int32_t m, uint8_t* d_tested, double* d_p, double* d_z, double* d_l, int32_t* d_blocks,
                              float* d_med, float* d_mean, float* d_delta) {
    return fr_dev<true>(__func__, ctx, n, s, d_ps, d_cols, k, m, FrOut{d_tested, d_p, d_z, d_l, d_blocks, d_med, d_mean, d_delta});
}

extern "C" int sdice_page(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t k, int32_t m,
                          uint8_t* tested, double* p, double* z, double* l, int32_t* blocks, float* med, float* mean,
                          float* delta) {
    return fr_host<true>(__func__, ctx, n, s, ps, cols, k, m, FrOut{tested, p, z, l, blocks, med, mean, delta});
}
