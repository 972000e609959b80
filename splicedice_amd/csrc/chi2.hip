// pairwise --chi2: Yates-corrected chi-square test of independence for every sample pair.
//
// Replaces pairwise_fisher.py:133-136,179 with test_method = scipy.stats.chi2_contingency
// (scipy/stats/contingency.py, 1.15.3): for table [[a, b], [c, d]]
//   expected[i][j] = row_i * col_j / total                      (float64)
//   any expected == 0  -> scipy raises ValueError and the reference run aborts; here the table is
//                         counted in *n_bad (p = NaN) and the host raises
//   dof = 1, Yates: observed += sign(expected - observed) * min(0.5, |expected - observed|)
//   chi2 = sum (observed - expected)^2 / expected  (row-major order), p = chdtrc(1, chi2)
//        = erfc(sqrt(chi2 / 2))
// HBM-bound in principle (8 B per p-value, ~40 flops); same pair enumeration as the Fisher kernel.
#include "common.h"
#include <math.h>

namespace {

__device__ __forceinline__ double chi2_yates_p(double a, double b, double c, double d, bool& bad) {
    const double r0 = a + b, r1 = c + d, c0 = a + c, c1 = b + d, tot = r0 + r1;
    const double e[4] = {r0 * c0 / tot, r0 * c1 / tot, r1 * c0 / tot, r1 * c1 / tot};
    const double o[4] = {a, b, c, d};
    if (!(tot > 0.0) || e[0] == 0.0 || e[1] == 0.0 || e[2] == 0.0 || e[3] == 0.0) {
        bad = true;
        return __builtin_nan("");
    }
    double stat = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double diff = e[i] - o[i];
        const double mag = fmin(0.5, fabs(diff));
        const double dir = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
        const double oc = o[i] + mag * dir;
        const double t = oc - e[i];
        stat += t * t / e[i];
    }
    return erfc(sqrt(0.5 * stat));
}

// LIST: column q is the pair pair_tab[q] = i << 16 | j of a caller's list (sdice_pair_list_pack_dev) instead of the
// q-th pair in row-major order; n_bad then counts the listed tables only.
template <bool LIST>
__global__ void __launch_bounds__(256) chi2_pairs_kernel(const int32_t* __restrict__ incl,
                                                         const int64_t* __restrict__ excl, int64_t n, int s, int64_t n_pairs,
                                                         const unsigned* __restrict__ pair_tab, double* __restrict__ p,
                                                         unsigned long long* __restrict__ n_bad) {
    extern __shared__ double smd[];
    double* inc = smd;
    double* exc = smd + s;
    unsigned long long bad_count = 0;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        __syncthreads();
        for (int k = threadIdx.x; k < s; k += blockDim.x) {
            inc[k] = (double)incl[row * s + k];
            exc[k] = (double)excl[row * s + k];
        }
        __syncthreads();
        double* out = p + row * n_pairs;
        for (int64_t q = threadIdx.x; q < n_pairs; q += blockDim.x) {
            int i, j;
            if (LIST) {
                const unsigned ij = pair_tab[q];
                i = (int)(ij >> 16);
                j = (int)(ij & 0xffffu);
            } else {
                // invert q = i*s - i(i+1)/2 + (j-i-1)   (pairwise_fisher.py:142-147)
                const double bb = 2.0 * s - 1.0;
                i = (int)((bb - sqrt(bb * bb - 8.0 * (double)q)) * 0.5);
                if (i < 0) i = 0;
                if (i > s - 2) i = s - 2;
                while (i > 0 && (int64_t)i * s - (int64_t)i * (i + 1) / 2 > q) --i;
                while ((int64_t)(i + 1) * s - (int64_t)(i + 1) * (i + 2) / 2 <= q) ++i;
                j = (int)(q - ((int64_t)i * s - (int64_t)i * (i + 1) / 2)) + i + 1;
            }
            bool bad = false;
            out[q] = chi2_yates_p(inc[i], inc[j], exc[i], exc[j], bad);
            bad_count += bad ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad_count += __shfl_xor(bad_count, o);
    if ((threadIdx.x & 63) == 0 && bad_count) atomicAdd(n_bad, bad_count);
}

}  // namespace

// the pair kernel over n junctions: the m pairs of d_list, a caller's packed list, or (d_list == NULL) every pair
static int chi2_launch(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl, int64_t n_pairs,
                       const uint32_t* d_list, double* d_p, int64_t* d_n_bad) {
    int64_t blocks = n;
    const int64_t cap = (int64_t)ctx->n_cu * 32;
    if (blocks > cap) blocks = cap;
    const size_t lds = (size_t)s * 16;
    auto kern = d_list ? chi2_pairs_kernel<true> : chi2_pairs_kernel<false>;
    SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SD_LAUNCH(ctx, "chi2_pairs_kernel", kern, dim3((unsigned)blocks), dim3(256), lds, d_incl, d_excl, n, (int)s, n_pairs,
              (const unsigned*)d_list, d_p, reinterpret_cast<unsigned long long*>(d_n_bad));
    return SDICE_OK;
}

extern "C" int sdice_chi2_pairs_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                                    double* d_p, int64_t* d_n_bad) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(d_n_bad, "d_n_bad is NULL");
    SD_HIP(hipSetDevice(ctx->device));
    SD_HIP(hipMemsetAsync(d_n_bad, 0, 8, ctx->stream));
    if (n == 0 || s < 2) return SDICE_OK;
    SD_ARG(d_incl && d_excl && d_p, "NULL pointer");
    SD_ARG(s <= 8192, "more than 8192 samples per junction is not supported");
    return chi2_launch(ctx, n, s, d_incl, d_excl, (int64_t)s * (s - 1) / 2, nullptr, d_p, d_n_bad);
}

extern "C" int sdice_chi2_pair_list_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                                        int64_t m, const uint32_t* d_tab, double* d_p, int64_t* d_n_bad) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0 && m >= 0, "negative size");
    SD_ARG(d_n_bad, "d_n_bad is NULL");
    SD_ARG(s <= 8192, "more than 8192 samples per junction is not supported");
    SD_ARG(m <= SD_MAX_PAIRS, "more than 33550336 pairs in one list is not supported");
    SD_HIP(hipSetDevice(ctx->device));
    SD_HIP(hipMemsetAsync(d_n_bad, 0, 8, ctx->stream));
    if (n == 0 || m == 0) return SDICE_OK;
    SD_ARG(s >= 2, "a pair list needs at least two samples");
    SD_ARG(d_incl && d_excl && d_tab && d_p, "NULL pointer");
    return chi2_launch(ctx, n, s, d_incl, d_excl, m, d_tab, d_p, d_n_bad);
}

extern "C" int sdice_chi2_pairs(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, double* p,
                                int64_t* n_bad) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(n_bad, "n_bad is NULL");
    *n_bad = 0;
    if (n == 0 || s < 2) return SDICE_OK;
    SD_ARG(incl && excl && p, "NULL pointer");
    SD_TRY(sd_check_pair_counts(__func__, n, s, incl, excl, false));
    const int64_t n_pairs = (int64_t)s * (s - 1) / 2;
    HostStaging st(ctx);
    int32_t* di;
    int64_t *de, *db;
    double* dp;
    SD_TRY(st.upload(&di, incl, n * s));
    SD_TRY(st.upload(&de, excl, n * s));
    SD_TRY(st.alloc(&dp, n * n_pairs));
    SD_TRY(st.alloc(&db, 1));
    SD_TRY(sdice_chi2_pairs_dev(ctx, n, s, di, de, dp, db));
    SD_TRY(st.download(p, dp, n * n_pairs));
    return st.download(n_bad, db, 1);
}

extern "C" int sdice_chi2_pair_list(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, int64_t m,
                                    const int32_t* pairs, double* p, int64_t* n_bad) try {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0 && m >= 0, "negative size");
    SD_ARG(n_bad, "n_bad is NULL");
    *n_bad = 0;
    SD_ARG(m == 0 || pairs, "NULL pointer");
    SD_ARG(s <= 8192, "more than 8192 samples per junction is not supported");
    SD_ARG(m <= SD_MAX_PAIRS, "more than 33550336 pairs in one list is not supported");
    SD_TRY(sd_check_pair_list(__func__, s, m, pairs));
    if (n == 0 || m == 0) return SDICE_OK;
    SD_ARG(incl && excl && p, "NULL pointer");
    SD_TRY(sd_check_pair_counts(__func__, n, s, incl, excl, false));
    HostStaging st(ctx);
    int32_t* di;
    int64_t *de, *db;
    uint32_t* dt;
    double* dp;
    SD_TRY(st.upload(&di, incl, n * s));
    SD_TRY(st.upload(&de, excl, n * s));
    SD_TRY(st.alloc(&dt, m));
    SD_TRY(sdice_pair_list_pack_dev(ctx, s, m, pairs, dt));
    SD_TRY(st.alloc(&dp, n * m));
    SD_TRY(st.alloc(&db, 1));
    SD_TRY(sdice_chi2_pair_list_dev(ctx, n, s, di, de, m, dt, dp, db));
    SD_TRY(st.download(p, dp, n * m));
    return st.download(n_bad, db, 1);
} catch (const std::exception& e) {
    sdice_set_error("sdice_chi2_pair_list: %s", e.what());
    return SDICE_ERR_NOMEM;
} catch (...) {
    sdice_set_error("sdice_chi2_pair_list: unknown exception");
    return SDICE_ERR_STATE;
}
