// K22: the paired shift of m matched column pairs per junction row -- the Hodges-Lehmann one-sample estimate (R's
// "(pseudo)median": the median of the Walsh averages) with its distribution-free confidence interval.
//
// Per row: a pair (a[q], b[q]) is kept when both of its values are non-NaN, m' pairs are kept and the row is tested when
// m' >= 3 (sdice_signedrank's rule).  d = the differences of the kept pairs, sdice_signedrank's: the INTEGER key_a - key_b
// on a row whose kept values are all 3-decimal PS values (PsKey::exact()), x - y in float32 on any other row.  ZERO
// DIFFERENCES ARE KEPT: the estimator uses all m' differences, unlike the test, which drops them (Hollander & Wolfe
// sections 3.2-3.3).  The M = m'(m'+1)/2 Walsh sums S_ij = d_i + d_j, i <= j, in ascending order, W = S / 2:
//   shift = the median of W;  c = max(1, floor(M/2 - zq sqrt(m'(m'+1)(2m'+1)/24)));  lo = W_(c),  hi = W_(M + 1 - c)
// On a grid row S is an integer in -2000..2000 reported as S / 2000.0; on any other S = (double)d_i + (double)d_j, one
// float64 addition, reported as 0.5 S (include/sdice.h has the contract).
//
// No Walsh average is ever stored (the shape of shift.hip, K20).  An order statistic is the smallest t with
// #{(i <= j) : img(S_ij) <= t} >= k, found by bisection over the IMAGE of a sum: S + 2000 on a grid row (0..4000: 12
// steps), the order-preserving 64 bits of the float64 on any other (at most 64 steps).  Four are wanted: the two middle
// ones (one when M is odd), c and M + 1 - c.  With d sorted ascending the rounded sum is monotone in d_j, so
// {j : img(d_i + d_j) <= t} is a prefix of the sorted d of some length L_i, and position i counts the pairs i <= j < L_i:
// max(0, L_i - i).  A float32 d enters as d + 0.0f, so no d and no sum is -0.0 and equal sums have equal images.
//
// Kernels:
//   walsh_group_kernel<P>: m <= 64.  A group of P = next_pow2(m) >= 8 lanes owns a row, one pair per lane, 64 / P rows per
//       wave side by side.  One group_sort of the signed d (d + 1000 on a grid row, the order bits of the float on any
//       other); the lane in sorted position i finds L_i by log2 P + 1 probes of the sorted d through __shfl: no LDS at
//       all.  The four bisections run in one loop and share its passes, from the images of 2 d_min and 2 d_max, the four
//       counts of a lane packed two to a word for the group sums (each at most 2080).  When no bisected row of the pass is
//       off the grid (a ballot, wave-uniform) the images are 32-bit integers, otherwise 64-bit with a select per row.
//       Lane i of the wave keeps the chunk's i-th row; the double precision finish and the stores happen once per chunk.
//   walsh_block_kernel: 65 <= m <= 4096, one workgroup of four waves per row, the four order statistics one wave each: no
//       barrier and no cross-wave sum inside a bisection.
//       Grid rows (known after the one pass that loads the row) are never sorted: one histogram h[d + 1000] of 2048 bins
//       (2001 used) filled by LDS atomics, wave 0 scans it to E[u] = #{d + 1000 < u}; the ORDERED count #{(i, j) : S_ij <= t}
//       is sum_v h[v] E[t - v + 1] with the index clamped at both ends, and the wanted one (ordered + #{i : 2 d_i <= t}) / 2.
//       A lane owns the bins v = lane + 64 q (conflict-free reads of E), its 32 counts, at most 4096 each, two to a register.
//       Other rows: ONE bitonic network over the 32-bit order bits of d, padding last; lane i of a wave takes d_i,
//       d_(i + 64), ... and binary-searches the sorted d from its own position on.  The bisection starts from the images of
//       2 d_min and 2 d_max.
//   All counts fit 32 bits (the ordered count is at most 4096^2 = 2^24).  A row that keeps +-inf, or whose float32 d
//   overflows, is never bisected: its triple is NaN.  The switch at 64 pairs is the lane-group kernels' everywhere.
//
// rowsum.h: PsKey, f32_ord / f32_unord, LaneGroup, group_add, group_sort, block_bitonic, kw_load_bins / kw_scan_bins (the
// scan of 1024 bins by a wave, twice here), ShiftOut, the SH_ marks of a row, f64_ord / f64_unord, shift_targets (shared
// with shift.hip), the launch sizes and the width ladder; colcheck.h: the check of the pair lists.
#include "common.h"
#include <math.h>
#include "rowsum.h"

namespace {

constexpr int WA_MAX_PAIRS = 4096;
constexpr int WA_GROUP_MAX = 64;         // pairs the lane-group kernel takes
constexpr int WA_BINS = 2048;            // 2001 used
constexpr int WA_D_OFS = 1000;           // bin of a grid difference: d + 1000
constexpr int WA_TOP = 4 * WA_D_OFS;     // image of a grid sum: S + 2000 = the two bins added, 0..4000

// c = max(1, floor(M/2 - zq sqrt(m'(m'+1)(2m'+1)/24))) in float64 as written (the product is below 2^38: exact)
__device__ __forceinline__ int walsh_rank(int nv, int M, double zq) {
    const long long v24 = (long long)nv * (nv + 1) * (2 * nv + 1);
    const double c = floor((double)M / 2.0 - zq * sqrt((double)v24 / 24.0));
    return c < 1.0 ? 1 : (int)c;
}

// the images of the four order statistics -> shift, lo, hi of a tested row; a zero result is +0.0
__device__ __forceinline__ void walsh_finish(int flags, unsigned long long a, unsigned long long b, unsigned long long l,
                                             unsigned long long h, double& shift, double& lo, double& hi) {
    if (flags & SH_INF) {
        shift = lo = hi = __builtin_nan("");
    } else if (flags & SH_OFF) {
        const double wa = 0.5 * f64_unord(a);
        shift = ((flags & SH_ODD) ? wa : 0.5 * (wa + 0.5 * f64_unord(b))) + 0.0;
        lo = 0.5 * f64_unord(l) + 0.0;
        hi = 0.5 * f64_unord(h) + 0.0;
    } else {
        const int sa = (int)a - 2 * WA_D_OFS, sb = (int)b - 2 * WA_D_OFS;
        shift = ((flags & SH_ODD) ? (double)sa / 2000.0 : (double)(sa + sb) / 4000.0) + 0.0;
        lo = (double)((int)l - 2 * WA_D_OFS) / 2000.0 + 0.0;
        hi = (double)((int)h - 2 * WA_D_OFS) / 2000.0 + 0.0;
    }
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
// the two image widths; a sorted d as its lane holds it: d + 1000 on a grid row, the float's bits on any other
struct WalshGrid {
    using T = int;
    static __device__ __forceinline__ int of(uint32_t di, uint32_t dj, bool) { return (int)di + (int)dj; }
};
struct WalshAny {
    using T = unsigned long long;
    static __device__ __forceinline__ unsigned long long of(uint32_t di, uint32_t dj, bool off) {
        return off ? f64_ord((double)__uint_as_float(di) + (double)__uint_as_float(dj)) : (unsigned long long)((int)di + (int)dj);
    }
};

// The four bisections of the rows of a pass, side by side.  on: the row is bisected (uniform in the group); dv: lane g0 + j
// holds the j-th smallest d of the row's nv, gl its own position; k: the four targets.  -> res[q] = the image of the
// k[q]-th smallest Walsh sum, to every lane of the group (0 when !on)
template <int P, class Img>
__device__ __forceinline__ void walsh_group_select(bool on, bool off, uint32_t dv, int g0, int gl, int nv, const int (&k)[4],
                                                   unsigned long long (&res)[4]) {
    using T = typename Img::T;
    const uint32_t dmin = __shfl(dv, g0), dmax = __shfl(dv, g0 + max(nv - 1, 0));
    T lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lo[q] = on ? Img::of(dmin, dmin, off) : (T)0;
        hi[q] = on ? Img::of(dmax, dmax, off) : (T)0;
    }
    while (__ballot(lo[0] < hi[0] || lo[1] < hi[1] || lo[2] < hi[2] || lo[3] < hi[3]) != 0ull) {       // wave-uniform
        T t[4];
        int pos[4];                                      // L_i: the sorted d whose sum with this lane's lies at or below t
#pragma unroll
        for (int q = 0; q < 4; ++q) { t[q] = lo[q] + ((hi[q] - lo[q]) >> 1); pos[q] = 0; }
#pragma unroll
        for (int step = P; step > 0; step >>= 1) {       // (the first probe is of the last position: L_i may be P)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = pos[q] + step - 1;
                const uint32_t dj = __shfl(dv, g0 + min(j, P - 1));
                if (j < nv && Img::of(dv, dj, off) <= t[q]) pos[q] += step;
            }
        }
        // the counts of the four, two to a word (each sum is at most 64 * 65 / 2)
        int c01 = 0, c23 = 0;
        if (gl < nv) {
            c01 = max(pos[0] - gl, 0) | (max(pos[1] - gl, 0) << 16);
            c23 = max(pos[2] - gl, 0) | (max(pos[3] - gl, 0) << 16);
        }
        c01 = group_add<P>(c01);
        c23 = group_add<P>(c23);
        const int cnt[4] = {c01 & 0xffff, c01 >> 16, c23 & 0xffff, c23 >> 16};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (lo[q] < hi[q]) {
                if (cnt[q] >= k[q]) hi[q] = t[q];
                else lo[q] = t[q] + 1;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) res[q] = (unsigned long long)lo[q];
}

template <int P>
__global__ void __launch_bounds__(256) walsh_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                          const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                          int m, double zq, int ch, ShiftOut o) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    const int ca = gl < m ? a[gl] : 0, cb = gl < m ? b[gl] : 0;       // 3 <= m <= P
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_flags = 0, s_rank = 0;
      unsigned long long s_img[4] = {0ull, 0ull, 0ull, 0ull};
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf(""), y = x;
        if (ri < rows_here && gl < m) {
            const float* prow = ps + (row0 + ri) * s;
            x = __builtin_nontemporal_load(prow + ca);
            y = __builtin_nontemporal_load(prow + cb);
        }
        const bool kept = x == x && y == y;
        const int nv = __popcll((__ballot(kept) >> g0) & G::MASK);
        const PsKey kx = key_of_ps(x), ky = key_of_ps(y);
        const bool off = ((__ballot(kept && !(kx.exact() && ky.exact())) >> g0) & G::MASK) != 0ull;     // the row is off the grid
        const float df = (x - y) + 0.0f;                     // (-0.0 -> +0.0)
        const bool inf = ((__ballot(kept && !__builtin_isfinite(df)) >> g0) & G::MASK) != 0ull;         // (never on a grid row)
        const bool tested = nv >= 3;
        const int M = nv * (nv + 1) / 2;
        const int rank = walsh_rank(nv, M, zq);
        int k[4];
        shift_targets(M, rank, k);
        // ---- the sorted d, one per lane from the group's first lane on
        const uint32_t key = !kept ? PAD32 : (off ? f32_ord(df) : (uint32_t)(kx.key() - ky.key() + WA_D_OFS));
        const uint32_t sorted = group_sort<P, uint32_t>(key, gl);
        const uint32_t dv = off ? __float_as_uint(f32_unord(sorted)) : sorted;
        const bool on = tested && !inf;
        unsigned long long img[4];
        if (__ballot(on && off) == 0ull)                     // wave-uniform: every bisected row of the pass is on the grid
            walsh_group_select<P, WalshGrid>(on, off, dv, g0, gl, nv, k, img);
        else
            walsh_group_select<P, WalshAny>(on, off, dv, g0, gl, nv, k, img);
        const int flags = (tested ? SH_TESTED : 0) | (off ? SH_OFF : 0) | (inf ? SH_INF : 0) | ((M & 1) ? SH_ODD : 0);
        // ---- to the lanes that keep the rows of this pass: lane r0 + q takes group q's
        const int src = G::src(lane, r0);
        const bool mine = G::mine(lane, r0);
        const int t_flags = __shfl(flags, src), t_rank = __shfl(rank, src);
        unsigned long long t_img[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t_img[q] = __shfl(img[q], src);
        if (mine) {
            s_flags = t_flags; s_rank = t_rank;
#pragma unroll
            for (int q = 0; q < 4; ++q) s_img[q] = t_img[q];
        }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = (s_flags & SH_TESTED) != 0;
        double shift = 0.0, lo = 0.0, hi = 0.0;
        if (tested) walsh_finish(s_flags, s_img[0], s_img[1], s_img[2], s_img[3], shift, lo, hi);
        o.tested[row] = tested ? 1 : 0;
        o.shift[row] = shift;
        o.lo[row] = lo;
        o.hi[row] = hi;
        o.rank[row] = tested ? s_rank : 0;
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
struct WalshRowLds {
    unsigned h[WA_BINS];                     // the histogram of a grid row's d + 1000
    unsigned E[WA_BINS];                     // E[u] = #{d + 1000 < u}
    int nv, flags;
    unsigned long long res[4];
};

// the k-th smallest Walsh sum of a grid row by one wave -> its image
__device__ __forceinline__ unsigned long long walsh_wave_select_grid(const WalshRowLds& sh, int lane, int k) {
    unsigned a[16];                                      // the counts of the bins lane + 64 q, two to a register
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = sh.h[lane + 128 * q] | (sh.h[lane + 128 * q + 64] << 16);
    int lo = 0, hi = WA_TOP;
    while (lo < hi) {                                    // wave-uniform, 12 trips
        const int t = (lo + hi) >> 1;
        unsigned cnt = 0u;                               // ordered pairs (i, j) with bin_i + bin_j <= t
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int u = t + 1 - (lane + 128 * q);      // #{bin_j <= t - v} = E[t - v + 1]; the bins from 2001 on are empty
            cnt += (a[q] & 0xffffu) * sh.E[min(max(u, 0), WA_BINS - 1)];
            cnt += (a[q] >> 16) * sh.E[min(max(u - 64, 0), WA_BINS - 1)];
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) cnt += __shfl_xor(cnt, ofs);
        cnt = (cnt + sh.E[(t >> 1) + 1]) >> 1;           // + the pairs i == j: 2 bin_i <= t; then i <= j is half of it
        if (cnt >= (unsigned)k) hi = t;
        else lo = t + 1;
    }
    return (unsigned long long)lo;
}

// the k-th smallest Walsh sum of any row without an infinity by one wave: D[0..nv) the sorted order bits of d
__device__ __forceinline__ unsigned long long walsh_wave_select_any(const uint32_t* D, int nv, int lane, int k) {
    const auto val = [](uint32_t key) { return (double)f32_unord(key); };
    unsigned long long lo = f64_ord(val(D[0]) + val(D[0])), hi = f64_ord(val(D[nv - 1]) + val(D[nv - 1]));
    while (lo < hi) {                                    // wave-uniform
        const unsigned long long t = lo + ((hi - lo) >> 1);
        unsigned cnt = 0u;
        for (int i = lane; i < nv; i += 64) {
            const double di = val(D[i]);
            int a = i, b = nv;                           // first j >= i with d_i + d_j above t
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (f64_ord(di + val(D[mid])) <= t) a = mid + 1;
                else b = mid;
            }
            cnt += (unsigned)(a - i);
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) cnt += __shfl_xor(cnt, ofs);
        if (cnt >= (unsigned)k) hi = t;
        else lo = t + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(RB_THREADS) walsh_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                 const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                                 int m, double zq, int P, ShiftOut o) {
    extern __shared__ __align__(16) unsigned char smemwa[];
    uint32_t* A = reinterpret_cast<uint32_t*>(smemwa);          // [P] the order bits of d, padding last
    __shared__ __align__(16) WalshRowLds sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        for (int i = tid; i < WA_BINS; i += RB_THREADS) sh.h[i] = 0u;
        if (tid == 0) { sh.nv = 0; sh.flags = 0; }
        __syncthreads();
        // ---- one pass over the pairs: the count, the histogram of the differences on the grid, what the row holds beside
        // them, and the sort key of every pair (dropped pairs and padding last)
        int cv = 0, bad = 0;
        for (int j = tid; j < P; j += RB_THREADS) {
            uint32_t key = PAD32;
            if (j < m) {
                const float x = __builtin_nontemporal_load(prow + a[j]), y = __builtin_nontemporal_load(prow + b[j]);
                if (x == x && y == y) {
                    const PsKey kx = key_of_ps(x), ky = key_of_ps(y);
                    if (kx.exact() && ky.exact()) atomicAdd(&sh.h[kx.key() - ky.key() + WA_D_OFS], 1u);
                    else bad |= SH_OFF;
                    const float df = (x - y) + 0.0f;
                    if (!__builtin_isfinite(df)) bad |= SH_INF;
                    key = f32_ord(df);
                    ++cv;
                }
            }
            A[j] = key;
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            cv += __shfl_xor(cv, ofs);
            bad |= __shfl_xor(bad, ofs);
        }
        if (lane == 0) {
            atomicAdd(&sh.nv, cv);
            if (bad) atomicOr(&sh.flags, bad);
        }
        __syncthreads();
        const int nv = sh.nv;
        const bool tested = nv >= 3;                        // block-uniform, as everything up to the stores
        const int M = nv * (nv + 1) / 2;
        const int rank = walsh_rank(nv, M, zq);
        const int flags = (tested ? SH_TESTED : 0) | sh.flags | ((M & 1) ? SH_ODD : 0);
        int k[4];
        shift_targets(M, rank, k);
        const int kw = wave == 0 ? k[0] : (wave == 1 ? k[1] : (wave == 2 ? k[2] : k[3]));
        const bool skip = wave == 1 && (M & 1);             // the one middle sum is wave 0's
        if (tested && !(flags & SH_INF)) {
            if (!(flags & SH_OFF)) {
                // ---- a grid row: E[u] = #{bin < u} by wave 0, 1024 bins at a time (lane owns bins [16 lane, 16 lane + 16))
                if (wave == 0) {
                    unsigned run = 0u;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        unsigned w[16];
                        kw_load_bins(sh.h + half * 1024, lane, w);
                        int tot;
                        const int pre = kw_scan_bins(w, lane, tot);
                        unsigned at = run + (unsigned)(pre - tot);
                        run += (unsigned)__shfl(pre, 63);
#pragma unroll
                        for (int q = 0; q < 16; ++q) { const unsigned here = w[q]; w[q] = at; at += here; }
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            reinterpret_cast<uint4*>(sh.E + half * 1024)[lane * 4 + q] =
                                make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
                    }
                }
                __syncthreads();
                if (!skip) {
                    const unsigned long long r = walsh_wave_select_grid(sh, lane, kw);
                    if (lane == 0) sh.res[wave] = r;
                }
            } else {
                block_bitonic(P, [=](int i, int l, int desc) {
                    const bool asc = desc == 0;
                    const uint32_t ax = A[i], ay = A[l];
                    if ((ax > ay) == asc) { A[i] = ay; A[l] = ax; }
                });
                if (!skip) {
                    const unsigned long long r = walsh_wave_select_any(A, nv, lane, kw);
                    if (lane == 0) sh.res[wave] = r;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            double shift = 0.0, lo = 0.0, hi = 0.0;
            if (tested) walsh_finish(flags, sh.res[0], sh.res[1], sh.res[2], sh.res[3], shift, lo, hi);
            o.tested[row] = tested ? 1 : 0;
            o.shift[row] = shift;
            o.lo[row] = lo;
            o.hi[row] = hi;
            o.rank[row] = tested ? rank : 0;
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

// the refusals both entry points make: sdice_signedrank's of the pair count, and zq
int walsh_check(int32_t m, int32_t s, double zq) {
    if (m > WA_MAX_PAIRS) {
        sdice_set_error("sdice_walsh: %d pairs, at most %d are supported", (int)m, WA_MAX_PAIRS);
        return SDICE_ERR_ARG;
    }
    SD_ARG_AS("sdice_walsh", m >= 1, "the number of pairs must be 1..4096");
    SD_ARG_AS("sdice_walsh", 2 * (int64_t)m <= s, "more paired columns than the table has (a column belongs to one pair only)");
    SD_ARG_AS("sdice_walsh", zq == zq && zq > 0.0 && zq <= 1.7976931348623157e308, "zq must be finite and above 0");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_walsh_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a, const int32_t* d_b,
                               int32_t m, double zq, uint8_t* d_tested, double* d_shift, double* d_lo, double* d_hi,
                               int32_t* d_rank) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(walsh_check(m, s, zq));
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_shift && d_lo && d_hi && d_rank, "NULL output");
    SD_ARG(d_ps && d_a && d_b, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const ShiftOut o{d_tested, d_shift, d_lo, d_hi, d_rank};
    if (m < 3) {                                               // no row can be tested
        SD_HIP(hipMemsetAsync(d_tested, 0, (size_t)n, ctx->stream));
        for (double* q : {d_shift, d_lo, d_hi}) SD_HIP(hipMemsetAsync(q, 0, (size_t)n * 8, ctx->stream));
        SD_HIP(hipMemsetAsync(d_rank, 0, (size_t)n * 4, ctx->stream));
        return SDICE_OK;
    }
    if (m <= WA_GROUP_MAX)
        return with_group_launch(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "walsh_group_kernel", (walsh_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_a, d_b, (int)m, zq, ch, o);
            return SDICE_OK;
        });
    const int P = next_pow2(m, 128);
    const size_t lds = (size_t)P * 4;
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH_LDS(ctx, "walsh_block_kernel", walsh_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n, (int)s,
                  d_a, d_b, (int)m, zq, P, o);
    return SDICE_OK;
}

extern "C" int sdice_walsh(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a, const int32_t* b, int32_t m,
                           double zq, uint8_t* tested, double* shift, double* lo, double* hi, int32_t* rank) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(walsh_check(m, s, zq));
    SD_ARG(a && b, "pair index list is NULL");
    SD_TRY(check_columns(__func__, {a, b}, m, s, "column index out of range", "a column may appear once over both pair lists"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && shift && lo && hi && rank, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t *da, *db;
    ShiftOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&da, a, m));
    SD_TRY(st.upload(&db, b, m));
    st.result(&d.tested, tested, n);
    st.result(&d.shift, shift, n);
    st.result(&d.lo, lo, n);
    st.result(&d.hi, hi, n);
    st.result(&d.rank, rank, n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_walsh_dev(ctx, n, s, d_ps, da, db, m, zq, d.tested, d.shift, d.lo, d.hi, d.rank));
    return st.download_results();
}
