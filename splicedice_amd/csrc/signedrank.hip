// K13: Wilcoxon signed-rank test per junction row over m matched column pairs (a[q], b[q]) + median / mean of each side.
//
// scipy.stats.wilcoxon(d, zero_method="wilcox", correction=False, alternative="two-sided", method="asymptotic") per row
// under the row rules of the two-set path: a pair is kept when both of its values are non-NaN, the row is tested when
// at least 3 pairs are kept.  Medians and means are np.median / np.mean of each side's kept values in pair order (equal
// pairs included).  The differences of the kept pairs lose their zeros, |d| gets average ranks, z is signed (positive
// when side 1 is larger) and p = erfc(|z| / sqrt 2); a tested row without a non-zero difference has z = 0, p = 1.
//
// Differences.  A row whose kept values all are 3-decimal PS values float32(key / 1000), key = 0..1000 (all that
// compare_sample_sets ever reads), takes d = key_a - key_b as an integer: equal printed differences tie, which a float
// subtraction of such values does not give (float32(0.3) - float32(0.2) != float32(0.2) - float32(0.1)).  Any other
// row takes d = x - y in float32.  The choice is a ballot per row and the only difference between the two kinds of row.
//
// Arithmetic, in integers up to the last step (as kruskal.hip):
//   sort key of a kept non-zero pair = (code << 1) | (d > 0), code = |key_a - key_b| or the bits of |d| (below 2^31),
//       0xFFFFFFFF pads; sorted ascending, a tie run is a run of equal `key >> 1`
//   r2   = 2 * average rank = first + last + 2 over the run [first, last]
//   W2   = sum of r2 over d > 0 (= 2 R+),   T = sum over runs of t^3 - t,   n' = number of non-zero differences
//   z    = (2 W2 - n'(n'+1)) / sqrt((2 n'(n'+1)(2n'+1) - T) / 3)
//        = (R+ - n'(n'+1)/4) / sqrt((n'(n'+1)(2n'+1) - T/2) / 24)
//
// Kernels:
//   signedrank_lane_kernel<P>: m <= 8 (P = 4 or 8), the small matched cohorts.  One LANE per row, the pairs in registers:
//       three sorting networks without a cross-lane step, the tie runs walked one after another, the sums in numpy's
//       order without a compaction (below 8 values numpy adds them one by one; 8 values are P = 8 with nothing dropped).
//       A wave reads 64 consecutive rows and stores 64 consecutive results.
//   signedrank_group_kernel<P>: 9 <= m <= 64.  A group of P = next_pow2(m) lanes owns a row, one pair per lane, 64 / P
//       rows per wave side by side: three bitonic networks of __shfl_xor inside the group (the keys, the two sides'
//       order-preserving bits for the medians), run bounds from a ballot of run starts, group reductions by xor
//       exchanges.  The kept values are compacted through the wave's LDS for the numpy-order sums (at most 64 values:
//       one leaf of numpy's pairwise recursion).  Lane i of the wave keeps the results of the chunk's i-th row; the
//       double precision finish and the stores happen once per chunk, for all its rows at once.
//   signedrank_block_kernel: 65 <= m <= 4096, one workgroup per row, modelled on kruskal_block_kernel: ordered
//       compaction of the kept pairs, numpy pairwise sums, one LDS bitonic sort that carries the three arrays through
//       the same barriers, run bounds by binary search.
// (A wave-per-row kernel with several elements per lane for 65..1024 pairs was left out: the block kernel computes the
// same thing and paired cohorts of that size are rare.)
//
// rowsum.h: PsKey, the order bits of a float, the key of a difference (pair_diff_key, exactrank.hip's too), the lane groups
// with their sums, sort and median, the block's compaction, pairwise sum, bitonic network and run bounds, the stores of a
// row, the output pointers with their zeroing and staging, the launch sizes and the column check; dd.h: the double-double
// arithmetic; erfc_dd.h: erfc by its series in that arithmetic (shared with jonckheere.hip).
#include "common.h"
#include <math.h>
#include "rowsum.h"
#include "dd.h"
#include "erfc_dd.h"

namespace {

constexpr int SR_MAX_PAIRS = 4096;
constexpr int SR_GROUP_MAX = 64;         // pairs the lane-group kernel takes
constexpr int SR_LEAF_MAX = 64;          // leaves of numpy's pairwise recursion over 4096 values (PW_DEPTH levels)

// p where most rows are (p >= 2.2e-5, x^2 = xn / xd <= SR_DD_X2_MAX) is erfc in double-double arithmetic (erfc_dd.h), x^2
// taken from the two integers, both below 2^53
__device__ double sr_erfc_dd(double xn, double xd) { return erfc_dd_x2(dd_div_d({xn, 0.0}, xd)); }

// z and p of a tested row from the integer pieces
__device__ __forceinline__ void sr_finish(int np, long long w2, long long tie, double& z, double& p) {
    if (np == 0) { z = 0.0; p = 1.0; return; }           // every kept pair equal
    const long long nn = (long long)np * (np + 1);
    const long long num = 2 * w2 - nn;                   // 4 (R+ - n'(n'+1)/4)
    const long long v2 = 2 * nn * (2 * np + 1) - tie;    // 48 Var(R+), > 0
    z = (double)num / sqrt((double)v2 / 3.0);
    // erfc's argument |z| / sqrt 2 = sqrt(3 num^2 / (2 v2)) from the integers themselves (3 num^2 < 2^53): two roundings,
    // not z's three and a product -- down the tail every rounding of the argument costs p about z^2 of them
    const double xn = (double)(3 * num * num), xd = (double)(2 * v2);
    if (num == 0) p = 1.0;
    else if (xn <= SR_DD_X2_MAX * xd) p = sr_erfc_dd(xn, xd);
    else p = erfc(sqrt(xn / xd));
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
template <int P>
__global__ void __launch_bounds__(256) signedrank_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                               const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                               int m, int ch, TwoSampleOut o) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    __shared__ float cx[4][64], cy[4][64];               // the kept values of the wave's rows, compacted, in pair order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    float* X = cx[wave] + g0;
    float* Y = cy[wave] + g0;
    const int ca = gl < m ? a[gl] : 0, cb = gl < m ? b[gl] : 0;
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_pack = 0, s_tie = 0;                         // tested << 31 | W2 << 8 | n'  (W2 <= 64 * 65, n' <= 64); T <= 64^3
      float s_med1 = 0.f, s_med2 = 0.f, s_mean1 = 0.f, s_mean2 = 0.f;
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf(""), y = x;
        if (ri < rows_here && gl < m) {
            const float* prow = ps + (row0 + ri) * s;
            x = __builtin_nontemporal_load(prow + ca);
            y = __builtin_nontemporal_load(prow + cb);
        }
        const bool kept = x == x && y == y;
        const unsigned long long km = (__ballot(kept) >> g0) & G::MASK;
        const int nv = __popcll(km);
        const bool offgrid = kept && !(key_of_ps(x).exact() && key_of_ps(y).exact());
        const bool grid = ((__ballot(offgrid) >> g0) & G::MASK) == 0ull;
        // ---- the numpy-order sums over the compacted values
        SD_WAVE_SYNC();          // the previous pass's readers are done with the wave's LDS
        if (kept) {
            const int pos = __popcll(km & ((1ull << gl) - 1ull));
            X[pos] = x;
            Y[pos] = y;
        }
        SD_WAVE_SYNC();
        const float sum1 = 0.0f + group_sum(X, nv, gl);      // np.sum starts from the identity 0: -0.0 values sum to +0.0
        const float sum2 = 0.0f + group_sum(Y, nv, gl);
        // ---- the medians
        const uint32_t ox = group_sort<P, uint32_t>(kept ? f32_ord(x) : PAD32, gl);
        const uint32_t oy = group_sort<P, uint32_t>(kept ? f32_ord(y) : PAD32, gl);
        const float med1 = group_median(ox, g0, nv), med2 = group_median(oy, g0, nv);
        // ---- the ranks of |d|
        const uint32_t key = group_sort<P, uint32_t>(kept ? pair_diff_key(x, y, grid) : PAD32, gl);
        const bool valid = key != PAD32;
        const int np = __popcll((__ballot(valid) >> g0) & G::MASK);
        const uint32_t prev = __shfl_up(key, 1);
        const bool start = valid && (gl == 0 || (prev >> 1) != (key >> 1));
        const unsigned long long sm = (__ballot(start) >> g0) & G::MASK;       // bit i: a tie run starts at position i
        const unsigned long long upto = (2ull << gl) - 1ull;                 // positions 0..gl
        int w2 = 0, tie = 0;
        if (valid) {
            const int first = 63 - __clzll((long long)(sm & upto));
            const unsigned long long above = sm & ~upto;
            const int last = above ? (__ffsll((long long)above) - 2) : np - 1;
            if (key & 1u) w2 = first + last + 2;
            const int t = last - first + 1;
            if (start) tie = t * t * t - t;
        }
        w2 = group_add<P>(w2);
        tie = group_add<P>(tie);
        // ---- to the lanes that keep the rows of this pass: lane r0 + q takes group q's
        const int src = G::src(lane, r0);
        const bool mine = G::mine(lane, r0);
        const int pack = nv >= 3 ? (int)(0x80000000u | ((unsigned)w2 << 8) | (unsigned)np) : 0;
        const int t_pack = __shfl(pack, src), t_tie = __shfl(tie, src);
        const float t_med1 = __shfl(med1, src), t_med2 = __shfl(med2, src);
        const float t_mean1 = __shfl(sum1 / (float)nv, src), t_mean2 = __shfl(sum2 / (float)nv, src);
        if (mine) { s_pack = t_pack; s_tie = t_tie; s_med1 = t_med1; s_med2 = t_med2; s_mean1 = t_mean1; s_mean2 = t_mean2; }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = s_pack < 0;
        double z = 0.0, p = 0.0;
        if (tested) sr_finish(s_pack & 0xff, (long long)((s_pack >> 8) & 0x7fffff), (long long)s_tie, z, p);
        store_two_sample(o, row, tested, p, z, s_med1, s_med2, s_mean1, s_mean2);
      }
    }
}

// ------------------------------------------------------------------ lane path: one lane per row, m <= 8
// ascending sort of P values in registers: the bitonic network, every index a compile-time constant
template <int P>
__device__ __forceinline__ void sr_sort_regs(uint32_t (&v)[P]) {
#pragma unroll
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t lo = min(v[i], v[l]), hi = max(v[i], v[l]);
                    const bool asc = (i & k) == 0;
                    v[i] = asc ? lo : hi;
                    v[l] = asc ? hi : lo;
                }
            }
        }
    }
}

template <int P>
__device__ __forceinline__ uint32_t sr_pick(const uint32_t (&v)[P], int idx) {
    uint32_t r = v[0];
#pragma unroll
    for (int i = 1; i < P; ++i) r = idx == i ? v[i] : r;
    return r;
}

// np.median of the nv smallest of the sorted order-preserving values
template <int P>
__device__ __forceinline__ float sr_regs_median(const uint32_t (&sorted)[P], int nv) {
    const int h = nv >> 1;
    const float v1 = f32_unord(sr_pick<P>(sorted, h));
    const float v0 = f32_unord(sr_pick<P>(sorted, h > 0 ? h - 1 : 0));
    return (nv & 1) ? v1 : (v0 + v1) / 2.0f;
}

// numpy pairwise_sum of the kept values (NaN = not kept) in pair order: below 8 values one after another from 0, at 8
// values (P = 8, nothing dropped) the eight accumulators hold one value each and only their fold is left
template <int P>
__device__ __forceinline__ float sr_regs_sum(const float (&v)[P], int nv) {
    float r = 0.f;
#pragma unroll
    for (int q = 0; q < P; ++q)
        if (v[q] == v[q]) r += v[q];
    if constexpr (P == 8) {
        const float tree = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        if (nv == 8) r = tree;
    }
    return r;
}

template <int P>
__global__ void __launch_bounds__(256) signedrank_lane_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                              const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                              int m, TwoSampleOut o) {
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        const float* prow = ps + row * s;
        float x[P], y[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            x[q] = y[q] = __builtin_nanf("");
            if (q < m) {                                 // uniform
                x[q] = __builtin_nontemporal_load(prow + a[q]);
                y[q] = __builtin_nontemporal_load(prow + b[q]);
            }
        }
        int nv = 0;
        bool grid = true;
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const bool kept = x[q] == x[q] && y[q] == y[q];
            if (!kept) x[q] = y[q] = __builtin_nanf("");  // a NaN on both sides marks a dropped pair from here on
            nv += kept ? 1 : 0;
            grid = grid && (!kept || (key_of_ps(x[q]).exact() && key_of_ps(y[q]).exact()));
        }
        const float sum1 = 0.0f + sr_regs_sum<P>(x, nv), sum2 = 0.0f + sr_regs_sum<P>(y, nv);
        uint32_t ux[P], uy[P], kd[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const bool kept = x[q] == x[q];
            ux[q] = kept ? f32_ord(x[q]) : PAD32;
            uy[q] = kept ? f32_ord(y[q]) : PAD32;
            kd[q] = kept ? pair_diff_key(x[q], y[q], grid) : PAD32;
        }
        sr_sort_regs<P>(ux);
        sr_sort_regs<P>(uy);
        sr_sort_regs<P>(kd);
        const float med1 = sr_regs_median<P>(ux, nv), med2 = sr_regs_median<P>(uy, nv);
        // tie runs of the sorted keys, one after another: a run [first, i] with cp positive members adds cp r2 to W2
        int np = 0, w2 = 0, tie = 0, first = 0, cp = 0;
        uint32_t prev = PAD32;                          // no code is this large
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if (kd[i] != PAD32) {
                const uint32_t code = kd[i] >> 1;
                if (code != prev) { first = i; cp = 0; }
                prev = code;
                cp += (int)(kd[i] & 1u);
                ++np;
                bool ends = true;
                if (i + 1 < P) ends = (kd[i + 1 < P ? i + 1 : i] >> 1) != code;      // (a pad's code is a NaN pattern)
                if (ends) {
                    const int t = i - first + 1;
                    w2 += cp * (first + i + 2);
                    tie += t * t * t - t;
                }
            }
        }
        const bool tested = nv >= 3;
        double z = 0.0, p = 0.0;
        if (tested) sr_finish(np, (long long)w2, (long long)tie, z, p);
        store_two_sample(o, row, tested, p, z, med1, med2, sum1 / (float)nv, sum2 / (float)nv);
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
__global__ void __launch_bounds__(RB_THREADS) signedrank_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                      const int32_t* __restrict__ a,
                                                                      const int32_t* __restrict__ b, int m, int P, TwoSampleOut o) {
    extern __shared__ __align__(16) unsigned char smems[];
    uint32_t* KX = reinterpret_cast<uint32_t*>(smems);         // [P] side 1: first the compacted floats, then their order bits
    uint32_t* KY = KX + P;                                      // [P] side 2
    uint32_t* KD = KY + P;                                      // [P] the sort keys of the differences
    float* FX = reinterpret_cast<float*>(KX);
    float* FY = reinterpret_cast<float*>(KY);
    __shared__ float leaf_sum[SR_LEAF_MAX];
    __shared__ float scratch8[SR_LEAF_MAX * 8];
    __shared__ int leaf_off[SR_LEAF_MAX + 1];
    __shared__ int wcnt[RB_THREADS / 64];
    __shared__ unsigned long long accS[2];                      // W2, T
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        // ordered compaction of the pairs of ps[row, (a[q], b[q])] without a NaN
        const int nv = block_compact_by(
            m, wcnt,
            [=](int q) {
                float2 v = {__builtin_nanf(""), __builtin_nanf("")};
                if (q < m) { v.x = prow[a[q]]; v.y = prow[b[q]]; }
                return v;
            },
            [=](int, int pos, bool valid, float2 v) {
                if (valid) { FX[pos] = v.x; FY[pos] = v.y; }
            });
        if (nv < 3) {                                           // block-uniform
            if (tid == 0) store_two_sample(o, row, false, 0.0, 0.0, 0.f, 0.f, 0.f, 0.f);
            continue;                                           // (the compaction ended with a barrier)
        }
        // np.sum: the identity 0 plus the pairwise tree
        const float sum1 = 0.0f + block_pairwise_sum<PW_DEPTH>(FX, nv, leaf_off, leaf_sum, scratch8, SR_LEAF_MAX);
        const float sum2 = 0.0f + block_pairwise_sum<PW_DEPTH>(FY, nv, leaf_off, leaf_sum, scratch8, SR_LEAF_MAX);
        // ---- grid row or not; keys of the differences, order bits of the two sides, padding last
        int off = 0;
        for (int i = tid; i < nv; i += RB_THREADS) off |= !(key_of_ps(FX[i]).exact() && key_of_ps(FY[i]).exact());
        const bool grid = __syncthreads_or(off) == 0;
        for (int i = tid; i < P; i += RB_THREADS) {
            uint32_t kx = PAD32, ky = PAD32, kd = PAD32;
            if (i < nv) {
                const float x = FX[i], y = FY[i];
                kx = f32_ord(x); ky = f32_ord(y); kd = pair_diff_key(x, y, grid);
            }
            KX[i] = kx; KY[i] = ky; KD[i] = kd;
        }
        if (tid < 2) accS[tid] = 0ull;
        __syncthreads();
        block_bitonic(P, [=](int i, int l, int desc) {           // the three arrays, each on its own, through the same barriers
            const bool asc = desc == 0;
            uint32_t* const arr[3] = {KX, KY, KD};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t x = arr[q][i], y = arr[q][l];
                if ((x > y) == asc) { arr[q][i] = y; arr[q][l] = x; }
            }
        });
        int np = 0;                                             // first padding key: the number of non-zero differences
        {
            int hi = nv;
            while (np < hi) { const int mid = (np + hi) >> 1; if (KD[mid] != PAD32) np = mid + 1; else hi = mid; }
        }
        // ---- ranks
        long long w2 = 0, tie = 0;
        for (int q = tid; q < np; q += RB_THREADS) {
            const uint32_t key = KD[q], code = key >> 1;
            const RunBounds run = run_bounds(KD, np, code, ProjAbove1{});
            if (key & 1u) w2 += run.first + run.past + 1;
            if (q == run.first) {
                const long long t = run.past - run.first;
                tie += t * t * t - t;
            }
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            w2 += __shfl_xor(w2, ofs);
            tie += __shfl_xor(tie, ofs);
        }
        if (lane == 0) {
            if (w2) atomicAdd(&accS[0], (unsigned long long)w2);
            if (tie) atomicAdd(&accS[1], (unsigned long long)tie);
        }
        __syncthreads();
        if (tid == 0) {
            const float med1 = median_of_ord(KX, nv), med2 = median_of_ord(KY, nv);    // np.median on float32
            double z, p;
            sr_finish(np, (long long)accS[0], (long long)accS[1], z, p);
            store_two_sample(o, row, true, p, z, med1, med2, sum1 / (float)nv, sum2 / (float)nv);
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

template <int P>
int sr_launch_lane(sdice_ctx* ctx, const float* d_ps, int64_t n, int s, const int32_t* d_a, const int32_t* d_b, int m, TwoSampleOut o) {
    const int64_t blocks = row_launch_blocks(ctx, sd_ceil_div(n, 256));
    SD_LAUNCH(ctx, "signedrank_lane_kernel", (signedrank_lane_kernel<P>), dim3((unsigned)blocks), dim3(256), 0, d_ps, n, s,
              d_a, d_b, m, o);
    return SDICE_OK;
}

int sr_check_m(int32_t m) {
    if (m > SR_MAX_PAIRS) {
        sdice_set_error("sdice_signedrank: %d pairs, at most %d are supported", (int)m, SR_MAX_PAIRS);
        return SDICE_ERR_ARG;
    }
    SD_ARG(m >= 1, "the number of pairs must be 1..4096");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_signedrank_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a,
                                    const int32_t* d_b, int32_t m, uint8_t* d_tested, double* d_p, double* d_z,
                                    float* d_med1, float* d_med2, float* d_mean1, float* d_mean2, float* d_delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(sr_check_m(m));
    SD_ARG(2 * (int64_t)m <= s, "more paired columns than the table has (a column belongs to one pair only)");
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med1 && d_med2 && d_mean1 && d_mean2 && d_delta, "NULL output");
    SD_ARG(d_ps && d_a && d_b, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    TwoSampleOut o{d_tested, d_p, d_z, d_med1, d_med2, d_mean1, d_mean2, d_delta};
    if (m < 3) return zero_two_sample(ctx, n, o);            // no row can be tested
    if (m <= 4) return sr_launch_lane<4>(ctx, d_ps, n, s, d_a, d_b, m, o);
    if (m <= 8) return sr_launch_lane<8>(ctx, d_ps, n, s, d_a, d_b, m, o);
    if (m <= SR_GROUP_MAX)
        return with_group_launch<16>(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "signedrank_group_kernel", (signedrank_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_a, d_b, (int)m, ch, o);
            return SDICE_OK;
        });
    const int P = next_pow2(m, 128);
    const size_t lds = (size_t)P * 3 * 4;
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH_LDS(ctx, "signedrank_block_kernel", signedrank_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps,
                  n, (int)s, d_a, d_b, (int)m, P, o);
    return SDICE_OK;
}

extern "C" int sdice_signedrank(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a,
                                const int32_t* b, int32_t m, uint8_t* tested, double* p, double* z, float* med1,
                                float* med2, float* mean1, float* mean2, float* delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(sr_check_m(m));
    SD_ARG(a && b, "pair index list is NULL");
    SD_TRY(check_columns(__func__, {a, b}, m, s, "column index out of range", "a column may appear once over both pair lists"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med1 && med2 && mean1 && mean2 && delta, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    TwoSampleOut o;
    float* d_ps;
    int32_t *da, *db;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&da, a, m));
    SD_TRY(st.upload(&db, b, m));
    SD_TRY(stage_two_sample(st, n, {tested, p, z, med1, med2, mean1, mean2, delta}, &o));
    SD_TRY(sdice_signedrank_dev(ctx, n, s, d_ps, da, db, m, o.tested, o.p, o.z, o.med1, o.med2, o.mean1, o.mean2, o.delta));
    return st.download_results();
}
