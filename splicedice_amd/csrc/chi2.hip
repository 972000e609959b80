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
#include "pairs.h"

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
            if (LIST) sd_pair_unpack(pair_tab[q], i, j);
            else sd_pair_of(q, s, i, j);
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
    SD_LAUNCH_LDS(ctx, "chi2_pairs_kernel", kern, dim3((unsigned)blocks), dim3(256), lds, d_incl, d_excl, n, (int)s, n_pairs,
                  (const unsigned*)d_list, d_p, reinterpret_cast<unsigned long long*>(d_n_bad));
    return SDICE_OK;
}

// the launch of a checked call (pairs.h)
static int chi2_call(const PairCall& c) {
    return chi2_launch(c.ctx, c.n, c.s, c.incl, c.excl, c.cols(), static_cast<const uint32_t*>(c.tab), c.p, c.n_bad);
}

extern "C" int sdice_chi2_pairs_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                                    double* d_p, int64_t* d_n_bad) {
    return sd_pairs_dev({__func__, ctx, n, s, d_incl, d_excl, false, 0, nullptr, d_p, true, d_n_bad}, chi2_call);
}

extern "C" int sdice_chi2_pair_list_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                                        int64_t m, const uint32_t* d_tab, double* d_p, int64_t* d_n_bad) {
    return sd_pairs_dev({__func__, ctx, n, s, d_incl, d_excl, true, m, d_tab, d_p, true, d_n_bad}, chi2_call);
}

extern "C" int sdice_chi2_pairs(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, double* p,
                                int64_t* n_bad) {
    return sd_pairs_host({__func__, ctx, n, s, incl, excl, false, 0, nullptr, p, true, n_bad}, chi2_call);
}

extern "C" int sdice_chi2_pair_list(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, int64_t m,
                                    const int32_t* pairs, double* p, int64_t* n_bad) {
    return sd_pairs_host({__func__, ctx, n, s, incl, excl, true, m, pairs, p, true, n_bad}, chi2_call);
}
