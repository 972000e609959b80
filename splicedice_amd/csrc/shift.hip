// K20: Hodges-Lehmann shift of two column groups per junction row with its distribution-free confidence interval.
//
// Per row: x = the row's values at the group-1 columns with NaNs dropped (n1' kept), y = group 2's (n2' kept), the row is
// tested when n1' >= 3 and n2' >= 3 (sdice_ranksum's rule).  M = n1' n2', N = n1' + n2', the differences d_ij = x_i - y_j
// in ascending order D_(1) <= ... <= D_(M):
//   shift = the median of D;  c = max(1, floor(M/2 - zq sqrt(M (N + 1) / 12)));  lo = D_(c),  hi = D_(M + 1 - c)
// On a row whose kept values are all 3-decimal PS values (PsKey::exact()) d is the INTEGER key_x - key_y, reported as
// k / 1000.0; on any other row d = (double)x - (double)y, one float64 subtraction (include/sdice.h has the contract).
//
// No difference is ever stored.  An order statistic D_(k) is the smallest t with #{d <= t} >= k, found by bisection over
// the IMAGE of a difference: an unsigned integer that orders as the differences do -- d + 1000 on a grid row (0..2000: 11
// steps), the order-preserving 64 bits of the float64 on any other (at most 64 steps).  Four order statistics are wanted,
// the two middle ones (one when M is odd), c and M + 1 - c, and #{d <= t} comes from the sorted y: the rounded
// subtraction is monotone in y, so {j : x_i - y_j <= t} is a tail of the sorted y for every x_i and one binary search
// finds where it starts.  The comparison is made on the image of the same (double)x - (double)y that the definition
// names.  Zeros enter as +0.0 (v + 0.0f, f32_unord), so no difference is -0.0 and equal differences have equal images.
//
// Kernels:
//   shift_group_kernel<P>: n1 + n2 <= 64.  A group of P = next_pow2(n1 + n2) lanes owns a row, one selected column per
//       lane (group 1's first), 64 / P rows per wave side by side.  One group_sort leaves the sorted y one per lane; a
//       group-1 lane keeps its x and reads y_j from the lane that holds it (__shfl: no LDS at all).  The four bisections
//       run in one loop and share its passes: log2 P probes each, the four counts of a lane packed two to a word for
//       the group sums.  When no tested row of the pass is off the grid (a ballot, wave-uniform) the images are 32-bit
//       integers, otherwise 64-bit with a select per row.  Lane i of the wave keeps the chunk's i-th row; the double
//       precision finish and the stores happen once per chunk.
//   shift_block_kernel: 65 <= n1 + n2 <= 8192, one workgroup of four waves per row, and the four order statistics are
//       one wave each, so the bisections need no barrier and no cross-wave sum.
//       Grid rows (known after the one pass that loads the row): two 1024-bin key histograms in LDS filled by LDS
//       atomics, wave 0 turns group 2's into E2[u] = #{y < u}; then #{d <= t} = sum_v h1[v] (n2' - E2[v - t]), a lane
//       owning the bins v = lane + 64 q (conflict-free reads) with its 16 h1 counts in registers.  No sort at all.
//       Other rows: ONE bitonic network over (group << 32 | f32_ord(v)), NaNs and padding last (ks.hip's), after which
//       the groups are two sorted segments; lane i of a wave takes x_i, x_(i + 64), ... and searches the sorted y.  The
//       bisection starts from the images of x_min - y_max and x_max - y_min, which the sorted segments give for free.
//       Sorting the differences outright where M is small was not built: the search is needed at 4096 v 4096 anyway, a
//       second path would add a dispatch threshold, and off-grid rows are the rare case of a PS table.
//   All counts fit 32 bits (M <= 2^24).  A row that keeps +-inf is never bisected: its triple is NaN.
//   The switch at 64 selected columns is the lane-group kernels' everywhere (one column per lane of a wave).
//
// rowsum.h: PsKey, f32_ord / f32_unord, LaneGroup, group_add, group_sort, block_bitonic, two_group_median_key,
// kw_load_bins / kw_scan_bins (the scan of a 1024-bin histogram by a wave), the launch sizes and the width ladder, and
// what walsh.hip (K22) shares with this file: ShiftOut, the SH_ marks of a row, f64_ord / f64_unord, shift_targets;
// colcheck.h: the check of the two groups.
#include "common.h"
#include <math.h>
#include "rowsum.h"

namespace {

constexpr int SH_MAX_GROUP = 4096;       // columns of one group
constexpr int SH_GROUP_MAX = 64;         // selected columns the lane-group kernel takes
constexpr int SH_BINS = 1024;            // 1001 used
constexpr int SH_GRID_OFS = 1000;        // image of a grid difference: d + 1000

// c = max(1, floor(M/2 - zq sqrt(M (N + 1) / 12))) in float64 as written (M (N + 1) < 2^38 is exact)
__device__ __forceinline__ int shift_rank(int M, int N, double zq) {
    const double c = floor((double)M / 2.0 - zq * sqrt((double)((long long)M * (N + 1)) / 12.0));
    return c < 1.0 ? 1 : (int)c;
}

// the images of the four order statistics -> shift, lo, hi of a tested row; a zero result is +0.0
__device__ __forceinline__ void shift_finish(int flags, unsigned long long a, unsigned long long b, unsigned long long l,
                                             unsigned long long h, double& shift, double& lo, double& hi) {
    if (flags & SH_INF) {
        shift = lo = hi = __builtin_nan("");
    } else if (flags & SH_OFF) {
        const double da = f64_unord(a);
        shift = ((flags & SH_ODD) ? da : 0.5 * (da + f64_unord(b))) + 0.0;
        lo = f64_unord(l) + 0.0;
        hi = f64_unord(h) + 0.0;
    } else {
        const int ka = (int)a - SH_GRID_OFS, kb = (int)b - SH_GRID_OFS;
        shift = ((flags & SH_ODD) ? (double)ka / 1000.0 : (double)(ka + kb) / 2000.0) + 0.0;
        lo = (double)((int)l - SH_GRID_OFS) / 1000.0 + 0.0;
        hi = (double)((int)h - SH_GRID_OFS) / 1000.0 + 0.0;
    }
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
// the two image widths; yv is a sorted y as its lane holds it: the key on a grid row, the float's bits on any other
struct ImgGrid {
    using T = int;
    static constexpr int TOP = 2 * SH_GRID_OFS;
    static __device__ __forceinline__ int of(int kx, double, uint32_t yv, bool) { return kx - (int)yv + SH_GRID_OFS; }
    static __device__ __forceinline__ int top(bool) { return TOP; }
};
struct ImgAny {
    using T = unsigned long long;
    static __device__ __forceinline__ unsigned long long of(int kx, double xd, uint32_t yv, bool off) {
        return off ? f64_ord(xd - (double)__uint_as_float(yv)) : (unsigned long long)(kx - (int)yv + SH_GRID_OFS);
    }
    static __device__ __forceinline__ unsigned long long top(bool off) { return off ? ~0ull : (unsigned long long)ImgGrid::TOP; }
};

// The four bisections of the rows of a pass, side by side.  on: the row is bisected (uniform in the group); hasx: this
// lane holds a kept value of group 1, (kx, xd) its key and its float64; yv: lane g0 + j holds the j-th smallest y; k:
// the four targets.  -> res[q] = the image of D_(k[q]), to every lane of the group (0 when !on)
template <int P, class Img>
__device__ __forceinline__ void group_select(bool on, bool off, bool hasx, int kx, double xd, uint32_t yv, int g0, int nv2,
                                             const int (&k)[4], unsigned long long (&res)[4]) {
    using T = typename Img::T;
    T lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { lo[q] = 0; hi[q] = on ? Img::top(off) : (T)0; }
    while (__ballot(lo[0] < hi[0] || lo[1] < hi[1] || lo[2] < hi[2] || lo[3] < hi[3]) != 0ull) {       // wave-uniform
        T t[4];
        int pos[4];                                      // values of y whose difference lies above t: a prefix of the sorted y
#pragma unroll
        for (int q = 0; q < 4; ++q) { t[q] = lo[q] + ((hi[q] - lo[q]) >> 1); pos[q] = 0; }
#pragma unroll
        for (int step = P >> 1; step > 0; step >>= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = pos[q] + step - 1;          // < P - 1
                const uint32_t yj = __shfl(yv, g0 + j);
                if (j < nv2 && Img::of(kx, xd, yj, off) > t[q]) pos[q] += step;
            }
        }
        // the counts of the four, two to a word (each sum is at most 1024)
        int c01 = 0, c23 = 0;
        if (hasx) {
            c01 = (nv2 - pos[0]) | ((nv2 - pos[1]) << 16);
            c23 = (nv2 - pos[2]) | ((nv2 - pos[3]) << 16);
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
__global__ void __launch_bounds__(256) shift_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                          const int32_t* __restrict__ g1, int n1,
                                                          const int32_t* __restrict__ g2, int n2, double zq, int ch,
                                                          ShiftOut o) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    const int m = n1 + n2;                               // 6 <= m <= P, n1 <= 61
    const bool in1 = gl < n1;
    int col = 0;
    if (gl < m) col = in1 ? g1[gl] : g2[gl - n1];
    const unsigned long long mask1 = (1ull << n1) - 1ull;
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_flags = 0, s_rank = 0;
      unsigned long long s_img[4] = {0ull, 0ull, 0ull, 0ull};
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf("");
        if (ri < rows_here && gl < m) x = __builtin_nontemporal_load(ps + (row0 + ri) * s + col);
        const bool kept = x == x;
        const unsigned long long km = (__ballot(kept) >> g0) & G::MASK;
        const int nv1 = __popcll(km & mask1), nv2 = __popcll(km >> n1);
        const PsKey pk = key_of_ps(x);
        const bool off = ((__ballot(kept && !pk.exact()) >> g0) & G::MASK) != 0ull;       // the row is off the grid
        const bool inf = ((__ballot(kept && __builtin_isinf(x)) >> g0) & G::MASK) != 0ull;
        const bool tested = nv1 >= 3 && nv2 >= 3;
        const int M = nv1 * nv2;
        const int rank = shift_rank(M, nv1 + nv2, zq);
        int k[4];
        shift_targets(M, rank, k);
        // ---- the sorted y, one per lane from the group's first lane on
        const uint32_t o2 = group_sort<P, uint32_t>(kept && !in1 ? f32_ord(x) : PAD32, gl);
        const float yf = f32_unord(o2);
        const uint32_t yv = off ? __float_as_uint(yf) : (uint32_t)key_of_ps(yf).key();
        const bool on = tested && !inf;
        unsigned long long img[4];
        if (__ballot(on && off) == 0ull)                     // wave-uniform: every bisected row of the pass is on the grid
            group_select<P, ImgGrid>(on, off, kept && in1, pk.key(), 0.0, yv, g0, nv2, k, img);
        else
            group_select<P, ImgAny>(on, off, kept && in1, pk.key(), (double)(x + 0.0f), yv, g0, nv2, k, img);
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
        if (tested) shift_finish(s_flags, s_img[0], s_img[1], s_img[2], s_img[3], shift, lo, hi);
        o.tested[row] = tested ? 1 : 0;
        o.shift[row] = shift;
        o.lo[row] = lo;
        o.hi[row] = hi;
        o.rank[row] = tested ? s_rank : 0;
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
struct ShiftRowLds {
    unsigned h1[SH_BINS], h2[SH_BINS];       // the key histograms of a grid row; h2 becomes E2[u] = #{y < u}
    int nv1, nv2, flags;
    unsigned long long res[4];
};

// D_(k) of a grid row by one wave -> its image
__device__ __forceinline__ unsigned long long shift_wave_select_grid(const ShiftRowLds& sh, int lane, int nv2, int k) {
    unsigned a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = sh.h1[lane + 64 * q];
    int lo = -SH_GRID_OFS, hi = SH_GRID_OFS;
    while (lo < hi) {                                    // wave-uniform, 11 trips
        const int t = (lo + hi) >> 1;                    // (floor, also below zero)
        unsigned cnt = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int u = min(max(lane + 64 * q - t, 0), SH_BINS - 1);       // the bins from 1001 on are empty: E2 = n2' there
            cnt += a[q] * ((unsigned)nv2 - sh.h2[u]);
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) cnt += __shfl_xor(cnt, ofs);
        if (cnt >= (unsigned)k) hi = t;
        else lo = t + 1;
    }
    return (unsigned long long)(lo + SH_GRID_OFS);
}

// D_(k) of any row without an infinity by one wave: X[0..nv1) and Y[0..nv2) sorted keys, the low 32 bits order bits
__device__ __forceinline__ unsigned long long shift_wave_select_any(const unsigned long long* X, int nv1,
                                                                    const unsigned long long* Y, int nv2, int lane, int k) {
    const auto val = [](unsigned long long key) { return (double)f32_unord((uint32_t)key); };
    unsigned long long lo = f64_ord(val(X[0]) - val(Y[nv2 - 1])), hi = f64_ord(val(X[nv1 - 1]) - val(Y[0]));
    while (lo < hi) {                                    // wave-uniform
        const unsigned long long t = lo + ((hi - lo) >> 1);
        unsigned cnt = 0u;
        for (int i = lane; i < nv1; i += 64) {
            const double xd = val(X[i]);
            int a = 0, b = nv2;                          // first j with x - y_j <= t
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (f64_ord(xd - val(Y[mid])) > t) a = mid + 1;
                else b = mid;
            }
            cnt += (unsigned)(nv2 - a);
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) cnt += __shfl_xor(cnt, ofs);
        if (cnt >= (unsigned)k) hi = t;
        else lo = t + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(RB_THREADS) shift_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                 const int32_t* __restrict__ g1, int n1,
                                                                 const int32_t* __restrict__ g2, int n2, double zq, int P,
                                                                 ShiftOut o) {
    extern __shared__ __align__(16) unsigned char smemsh[];
    unsigned long long* A = reinterpret_cast<unsigned long long*>(smemsh);      // [P] group << 32 | order bits
    __shared__ __align__(16) ShiftRowLds sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = n1 + n2;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        for (int i = tid; i < SH_BINS; i += RB_THREADS) { sh.h1[i] = 0u; sh.h2[i] = 0u; }
        if (tid == 0) { sh.nv1 = 0; sh.nv2 = 0; sh.flags = 0; }
        __syncthreads();
        // ---- one pass over the selected columns: the counts, the histograms of the values on the grid, what the row
        // holds beside them, and the sort key of every column (NaNs and padding last)
        int c1 = 0, c2 = 0, bad = 0;
        for (int j = tid; j < P; j += RB_THREADS) {
            unsigned long long a = ~0ull;
            if (j < m) {
                const bool in1 = j < n1;
                const float v = __builtin_nontemporal_load(prow + (in1 ? g1[j] : g2[j - n1]));
                if (v == v) {
                    const PsKey pk = key_of_ps(v);
                    if (pk.exact()) atomicAdd(in1 ? &sh.h1[pk.key()] : &sh.h2[pk.key()], 1u);
                    else bad |= SH_OFF;
                    if (__builtin_isinf(v)) bad |= SH_INF;
                    c1 += in1 ? 1 : 0;
                    c2 += in1 ? 0 : 1;
                }
                a = two_group_median_key(v, in1);
            }
            A[j] = a;
        }
        int c12 = c1 | (c2 << 16);                          // (a wave sees at most 32 x 64 columns)
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            c12 += __shfl_xor(c12, ofs);
            bad |= __shfl_xor(bad, ofs);
        }
        if (lane == 0) {
            atomicAdd(&sh.nv1, c12 & 0xffff);
            atomicAdd(&sh.nv2, c12 >> 16);
            if (bad) atomicOr(&sh.flags, bad);
        }
        __syncthreads();
        const int nv1 = sh.nv1, nv2 = sh.nv2;
        const bool tested = nv1 >= 3 && nv2 >= 3;           // block-uniform, as everything up to the stores
        const int M = nv1 * nv2;
        const int rank = shift_rank(M, nv1 + nv2, zq);
        const int flags = (tested ? SH_TESTED : 0) | sh.flags | ((M & 1) ? SH_ODD : 0);
        int k[4];
        shift_targets(M, rank, k);
        const int kw = wave == 0 ? k[0] : (wave == 1 ? k[1] : (wave == 2 ? k[2] : k[3]));
        const bool skip = wave == 1 && (M & 1);             // the one middle difference is wave 0's
        if (tested && !(flags & SH_INF)) {
            if (!(flags & SH_OFF)) {
                // ---- a grid row: E2[u] = #{y < u} in place, by wave 0 (lane owns bins [16 lane, 16 lane + 16))
                if (wave == 0) {
                    unsigned w[16];
                    kw_load_bins(sh.h2, lane, w);
                    int tot;
                    unsigned run = (unsigned)(kw_scan_bins(w, lane, tot) - tot);
#pragma unroll
                    for (int q = 0; q < 16; ++q) { const unsigned here = w[q]; w[q] = run; run += here; }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        reinterpret_cast<uint4*>(sh.h2)[lane * 4 + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
                }
                __syncthreads();
                if (!skip) {
                    const unsigned long long r = shift_wave_select_grid(sh, lane, nv2, kw);
                    if (lane == 0) sh.res[wave] = r;
                }
            } else {
                block_bitonic(P, [=](int i, int l, int desc) {
                    const bool asc = desc == 0;
                    const unsigned long long ax = A[i], ay = A[l];
                    if ((ax > ay) == asc) { A[i] = ay; A[l] = ax; }
                });
                if (!skip) {
                    const unsigned long long r = shift_wave_select_any(A, nv1, A + nv1, nv2, lane, kw);
                    if (lane == 0) sh.res[wave] = r;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            double shift = 0.0, lo = 0.0, hi = 0.0;
            if (tested) shift_finish(flags, sh.res[0], sh.res[1], sh.res[2], sh.res[3], shift, lo, hi);
            o.tested[row] = tested ? 1 : 0;
            o.shift[row] = shift;
            o.lo[row] = lo;
            o.hi[row] = hi;
            o.rank[row] = tested ? rank : 0;
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

int shift_check(const char* fn, const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2, int32_t s, double zq) {
    SD_TRY(check_two_groups(fn, g1, n1, g2, n2, s, SH_MAX_GROUP));
    SD_ARG_AS(fn, zq == zq && zq > 0.0 && zq <= 1.7976931348623157e308, "zq must be finite and above 0");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_shift_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_g1, int32_t n1,
                               const int32_t* d_g2, int32_t n2, double zq, uint8_t* d_tested, double* d_shift, double* d_lo,
                               double* d_hi, int32_t* d_rank) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(shift_check("sdice_shift", nullptr, n1, nullptr, n2, s, zq));        // (device lists: the counts)
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_shift && d_lo && d_hi && d_rank, "NULL output");
    SD_ARG(d_ps && d_g1 && d_g2, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const ShiftOut o{d_tested, d_shift, d_lo, d_hi, d_rank};
    const int m = n1 + n2;
    if (n1 < 3 || n2 < 3) {                                    // no row can be tested
        SD_HIP(hipMemsetAsync(d_tested, 0, (size_t)n, ctx->stream));
        for (double* q : {d_shift, d_lo, d_hi}) SD_HIP(hipMemsetAsync(q, 0, (size_t)n * 8, ctx->stream));
        SD_HIP(hipMemsetAsync(d_rank, 0, (size_t)n * 4, ctx->stream));
        return SDICE_OK;
    }
    if (m <= SH_GROUP_MAX)
        return with_group_launch(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "shift_group_kernel", (shift_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_g1, (int)n1, d_g2, (int)n2, zq, ch, o);
            return SDICE_OK;
        });
    const int P = next_pow2(m, 128);
    const size_t lds = (size_t)P * 8;
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH_LDS(ctx, "shift_block_kernel", shift_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n, (int)s,
                  d_g1, (int)n1, d_g2, (int)n2, zq, P, o);
    return SDICE_OK;
}

extern "C" int sdice_shift(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* g1, int32_t n1,
                           const int32_t* g2, int32_t n2, double zq, uint8_t* tested, double* shift, double* lo, double* hi,
                           int32_t* rank) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(g1 && g2, "index list is NULL");
    SD_TRY(shift_check(__func__, g1, n1, g2, n2, s, zq));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && shift && lo && hi && rank, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t *dg1, *dg2;
    ShiftOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dg1, g1, n1));
    SD_TRY(st.upload(&dg2, g2, n2));
    st.result(&d.tested, tested, n);
    st.result(&d.shift, shift, n);
    st.result(&d.lo, lo, n);
    st.result(&d.hi, hi, n);
    st.result(&d.rank, rank, n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_shift_dev(ctx, n, s, d_ps, dg1, n1, dg2, n2, zq, d.tested, d.shift, d.lo, d.hi, d.rank));
    return st.download_results();
}
