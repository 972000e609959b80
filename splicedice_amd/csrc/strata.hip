// K17: stratified Wilcoxon rank-sum test per junction row (van Elteren) over two column groups whose columns carry a
// stratum id (batch, centre, sex, ...) + median / mean of each group.
//
// Per row and stratum h: the row's values at the group-1 and at the group-2 columns of h with NaNs dropped, n1h and n2h
// kept, N_h = n1h + n2h; a stratum is informative when n1h >= 1 and n2h >= 1, the others contribute nothing.  Values are
// ranked inside their stratum only and the strata's rank-sum deviations are added with weights 1 / (N_h + 1):
//   r2(v) = 2 #{x < v} + #{x == v} + 1 over the stratum's kept values           (integer, twice the mid-rank; -0.0 == +0.0)
//   D_h   = sum of r2 over group 1 of h  -  n1h (N_h + 1)                      (integer, = 2 (W_h - E[W_h]))
//   T_h   = sum over the stratum's tie runs of t^3 - t                          (integer)
//   d_h   = D_h / (2 (N_h + 1))
//   V_h   = n1h n2h (N_h^3 - N_h - T_h) / (12 N_h (N_h - 1) (N_h + 1)^2)        (tie-corrected Var(W_h) times the squared weight)
//   z     = sum d_h / sqrt(sum V_h),   p = erfc(|z| / sqrt 2),   no continuity correction, z > 0: group 1 is larger
// The row is tested when the kept counts summed over the informative strata are >= 3 on both sides; a tested row whose
// informative strata are all fully tied (sum V_h = 0) has z = 0, p = 1.  Medians and means are np.median / np.mean of
// ALL kept values of a group (every stratum) in list order: sdice_ranksum's, bit for bit.
//
// One sort per row gives everything: the key of a kept value is (stratum, value, group), so after the sort the strata are
// segments, the tie runs are runs inside them, and r2 = first + last + 2 - 2 segment_start over the run [first, last].
//   a row of 3-decimal PS values float32(key / 1000):  stratum << 17 | key << 1 | group        32 bits
//   any other row:                                     stratum << 33 | f32_ord(v) << 1 | group  64 bits
// (the choice is a ballot and changes the cost alone: on 3-decimal values both keys order and tie alike).
//
// Sum over the strata.  The terms d_h and V_h are float64 quotients of integers; they are added in double-double
// arithmetic (dd.h) by a butterfly and the sum is read back as one float64.  Every d_h is a multiple of 2^-67 below 2^10
// and every non-zero V_h a multiple of 2^-68 in [2^-16, 2^8] (N_h <= 8192; N^3 - sum t^3 >= 3 N (N - 1) once two values
// differ), so any partial sum of 64 of them has at most 84 significant bits: it fits a double-double, each addition is
// exact, and the sum is THE sum of the terms -- the same for every numbering of the strata, with no rounding for the
// cancellation in sum d_h to magnify.  (A sorted butterfly of plain float64, as kruskal.hip's, is numbering-independent
// too but rounds 63 times relative to sum |d_h|, and costs two more sorting networks.)
//
// Kernels:
//   strata_group_kernel<P>: n1 + n2 <= 64.  A group of P = next_pow2(n1 + n2) lanes owns a row, one selected column per
//       lane (group 1's first), 64 / P rows per wave side by side: three bitonic networks of __shfl_xor inside the group
//       (the two groups' order bits for the medians, the rank keys), run and segment starts from ballots, the stratum
//       sums by a segmented scan, the kept values compacted through the wave's LDS for the numpy-order sums.  Lane i of
//       the wave keeps the chunk's i-th row; the double precision finish and the stores happen once per chunk.
//   strata_block_kernel: 65 <= n1 + n2 <= 8192, one workgroup per row: ordered compaction + numpy pairwise sum per
//       group, then ONE bitonic network in LDS that carries two arrays through the same barriers -- (group, value) for the
//       medians and the rank keys --, run and segment bounds by binary search, the stratum sums in LDS, one wave finishes.
//
// rowsum.h: PsKey, order bits, lane groups with group_sum, group_sort (both key widths) and group_median, the block's
// compaction, pairwise sum, bitonic network, run bounds, the median key, the stores of a row, the output pointers with
// their zeroing and staging, launch sizes and the width ladder; colcheck.h: the check of the two groups and their stratum
// ids; dd.h: the double-double sum.
#include "common.h"
#include <math.h>
#include "rowsum.h"
#include "dd.h"

namespace {

constexpr int ST_MAX_GROUP = 4096;       // columns of one group
constexpr int ST_MAX_STRATA = 64;
constexpr int ST_GROUP_MAX = 64;         // selected columns the lane-group kernel takes
constexpr int ST_LEAF_MAX = 64;          // leaves of numpy's pairwise recursion over 4096 values (PW_DEPTH levels)

// the two key widths: padding, the stratum of a key; `key >> 1` is (stratum, value) and `key & 1` group 1 in both
template <class K> struct StKey;
template <> struct StKey<uint32_t> {
    static constexpr uint32_t PAD = 0xFFFFFFFFu;
    static __device__ __forceinline__ uint32_t make(uint32_t st, float v, bool in1) {
        return (st << 17) | ((uint32_t)key_of_ps(v).key() << 1) | (in1 ? 1u : 0u);
    }
    static __device__ __forceinline__ uint32_t strat(uint32_t k) { return k >> 17; }
};
template <> struct StKey<unsigned long long> {
    static constexpr unsigned long long PAD = ~0ull;
    static __device__ __forceinline__ unsigned long long make(uint32_t st, float v, bool in1) {
        return ((unsigned long long)st << 33) | ((unsigned long long)f32_ord(v) << 1) | (in1 ? 1ull : 0ull);
    }
    static __device__ __forceinline__ uint32_t strat(unsigned long long k) { return (uint32_t)(k >> 33); }
};
struct ProjCode { template <class T> __device__ __forceinline__ T operator()(T v) const { return v >> 1; } };
template <class K> struct ProjStrat { __device__ __forceinline__ uint32_t operator()(K v) const { return StKey<K>::strat(v); } };

// d_h and V_h of one stratum from its integers; both 0 unless the stratum is informative.  -> n1h | n2h << 16 of an
// informative stratum, else 0
__device__ __forceinline__ int st_stratum_terms(int n1h, int nh, long long w, long long tie, double& d, double& v) {
    d = 0.0;
    v = 0.0;
    const int n2h = nh - n1h;
    if (n1h < 1 || n2h < 1) return 0;
    const long long N = nh;
    const long long D = w - (long long)n1h * (N + 1);
    d = (double)D / (double)(2 * (N + 1));
    const unsigned long long num = (unsigned long long)((long long)n1h * n2h) * (unsigned long long)(N * N * N - N - tie);
    const unsigned long long den = 12ull * (unsigned long long)(N * (N - 1)) * (unsigned long long)((N + 1) * (N + 1));
    v = (double)num / (double)den;
    return n1h | (n2h << 16);
}

// z and p of a tested row
__device__ __forceinline__ void st_finish(double sd, double sv, double& z, double& p) {
    if (!(sv > 0.0)) { z = 0.0; p = 1.0; return; }       // every informative stratum fully tied (sd is 0 too)
    z = sd / sqrt(sv);
    p = sd == 0.0 ? 1.0 : erfc(fabs(sd) / sqrt(2.0 * sv));
}

// the double-double sum over `width` lanes (a power of two, aligned), to every one of them; exact here (file comment)
template <int WIDTH>
__device__ __forceinline__ double st_dd_lane_sum(double term) {
    DD a = {term, 0.0};
#pragma unroll
    for (int ofs = 1; ofs < WIDTH; ofs <<= 1) a = dd_add(a, {__shfl_xor(a.hi, ofs), __shfl_xor(a.lo, ofs)});
    return a.hi + a.lo;
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
struct StSums { double sd, sv; int cnt; };       // sum d_h, sum V_h, n1' | n2' << 16 over the informative strata

// the group's keys -> its sums, to every lane of the group
template <int P, class K>
__device__ __forceinline__ StSums st_group_sums(K unsorted, int gl, int g0) {
    using G = LaneGroup<P>;
    const K key = group_sort<P, K>(unsorted, gl);
    const bool valid = key != StKey<K>::PAD;                             // the valid keys are positions 0 .. N
    const int N = __popcll((__ballot(valid) >> g0) & G::MASK);
    const K prev = __shfl_up(key, 1);
    const bool rstart = valid && (gl == 0 || (prev >> 1) != (key >> 1));
    const bool sstart = valid && (gl == 0 || StKey<K>::strat(prev) != StKey<K>::strat(key));
    const unsigned long long rm = (__ballot(rstart) >> g0) & G::MASK;    // bit i: a tie run starts at position i
    const unsigned long long sm = (__ballot(sstart) >> g0) & G::MASK;    // bit i: a stratum starts at position i
    const unsigned long long m1 = (__ballot(valid && (key & 1)) >> g0) & G::MASK;      // bit i: position i is of group 1
    const unsigned long long upto = (2ull << gl) - 1ull;                 // positions 0..gl
    int s0 = 0, s1 = -1;
    unsigned pack = 0;                                                   // r2 of a group-1 value | (t^3 - t of a run start) << 13
    if (valid) {
        const int first = 63 - __clzll((long long)(rm & upto));
        const unsigned long long above = rm & ~upto;
        const int last = above ? (__ffsll((long long)above) - 2) : N - 1;
        s0 = 63 - __clzll((long long)(sm & upto));
        const unsigned long long sabove = sm & ~upto;
        s1 = sabove ? (__ffsll((long long)sabove) - 2) : N - 1;
        const int t = last - first + 1;
        if (key & 1) pack = (unsigned)(first + last + 2 - 2 * s0);       // sums to at most 64 * 65 < 2^13
        if (rstart) pack |= (unsigned)(t * t * t - t) << 13;             // sums to less than 64^3 = 2^18
    }
    // inclusive scan inside the stratum's segment: its last position gets the stratum's two sums
#pragma unroll
    for (int ofs = 1; ofs < P; ofs <<= 1) {
        const unsigned up = __shfl_up(pack, ofs);
        if (valid && gl - ofs >= s0) pack += up;
    }
    double d = 0.0, v = 0.0;
    int cnt = 0;
    if (valid && gl == s1) {
        const unsigned long long seg = ((2ull << s1) - 1ull) & ~((1ull << s0) - 1ull);
        cnt = st_stratum_terms(__popcll(m1 & seg), s1 - s0 + 1, (long long)(pack & 0x1fffu), (long long)(pack >> 13), d, v);
    }
    StSums r;
    r.sd = st_dd_lane_sum<P>(d);
    r.sv = st_dd_lane_sum<P>(v);
    r.cnt = group_add<P>(cnt);
    return r;
}

template <int P>
__global__ void __launch_bounds__(256) strata_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                           const int32_t* __restrict__ g1, int n1,
                                                           const int32_t* __restrict__ g2, int n2,
                                                           const int32_t* __restrict__ st1, const int32_t* __restrict__ st2,
                                                           int ch, TwoSampleOut o) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    __shared__ float cx[4][64], cy[4][64];               // the kept values of the wave's rows, compacted, in list order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    float* X = cx[wave] + g0;
    float* Y = cy[wave] + g0;
    const int m = n1 + n2;                               // 6 <= m <= P, n1 <= 61
    const bool in1 = gl < n1;
    int col = 0;
    uint32_t st = 0;
    if (gl < m) {
        col = in1 ? g1[gl] : g2[gl - n1];
        st = (uint32_t)(in1 ? st1[gl] : st2[gl - n1]) & 63u;
    }
    const unsigned long long mask1 = (1ull << n1) - 1ull;
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_tested = 0;
      double s_sd = 0.0, s_sv = 0.0;
      float s_med1 = 0.f, s_med2 = 0.f, s_mean1 = 0.f, s_mean2 = 0.f;
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf("");
        if (ri < rows_here && gl < m) x = __builtin_nontemporal_load(ps + (row0 + ri) * s + col);
        // (this front is ks.hip's, written out in both: as a helper it changed the kernels and strata's timed slower, A.17)
        const bool kept = x == x;
        const unsigned long long km = (__ballot(kept) >> g0) & G::MASK;
        const unsigned long long k1 = km & mask1, k2 = km >> n1;
        const int nv1 = __popcll(k1), nv2 = __popcll(k2);
        const bool offgrid = kept && !key_of_ps(x).exact();
        // ---- the numpy-order sums over the compacted values
        SD_WAVE_SYNC();          // the previous pass's readers are done with the wave's LDS
        if (kept) {
            if (in1) X[__popcll(k1 & ((1ull << gl) - 1ull))] = x;
            else Y[__popcll(k2 & ((1ull << (gl - n1)) - 1ull))] = x;
        }
        SD_WAVE_SYNC();
        const float sum1 = 0.0f + group_sum(X, nv1, gl);     // np.sum starts from the identity 0: -0.0 values sum to +0.0
        const float sum2 = 0.0f + group_sum(Y, nv2, gl);
        // ---- the medians
        const uint32_t o1 = group_sort<P, uint32_t>(kept && in1 ? f32_ord(x) : PAD32, gl);
        const uint32_t o2 = group_sort<P, uint32_t>(kept && !in1 ? f32_ord(x) : PAD32, gl);
        const float med1 = group_median(o1, g0, nv1), med2 = group_median(o2, g0, nv2);
        // ---- the ranks inside the strata; the narrow key when every row of the pass is on the 3-decimal grid
        StSums sums;
        if (__ballot(offgrid) == 0ull)                       // wave-uniform
            sums = st_group_sums<P, uint32_t>(kept ? StKey<uint32_t>::make(st, x, in1) : StKey<uint32_t>::PAD, gl, g0);
        else
            sums = st_group_sums<P, unsigned long long>(
                kept ? StKey<unsigned long long>::make(st, x, in1) : StKey<unsigned long long>::PAD, gl, g0);
        const int tested = ((sums.cnt & 0xffff) >= 3 && (sums.cnt >> 16) >= 3) ? 1 : 0;
        // ---- to the lanes that keep the rows of this pass: lane r0 + q takes group q's
        const int src = G::src(lane, r0);
        const bool mine = G::mine(lane, r0);
        const int t_tested = __shfl(tested, src);
        const double t_sd = __shfl(sums.sd, src), t_sv = __shfl(sums.sv, src);
        const float t_med1 = __shfl(med1, src), t_med2 = __shfl(med2, src);
        const float t_mean1 = __shfl(sum1 / (float)nv1, src), t_mean2 = __shfl(sum2 / (float)nv2, src);
        if (mine) {
            s_tested = t_tested; s_sd = t_sd; s_sv = t_sv;
            s_med1 = t_med1; s_med2 = t_med2; s_mean1 = t_mean1; s_mean2 = t_mean2;
        }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = s_tested != 0;
        double z = 0.0, p = 0.0;
        if (tested) st_finish(s_sd, s_sv, z, p);
        store_two_sample(o, row, tested, p, z, s_med1, s_med2, s_mean1, s_mean2);
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
struct StAcc {                                   // per stratum, in LDS
    unsigned long long w[ST_MAX_STRATA];         // sum of r2 over group 1
    unsigned long long tie[ST_MAX_STRATA];       // sum of t^3 - t
    int n1h[ST_MAX_STRATA];
    int nh[ST_MAX_STRATA];
};

// the sorted rank keys B[0..N) -> the stratum sums in acc (cleared by the caller), by the whole block; no barrier inside
template <class K>
__device__ __forceinline__ void st_block_ranks(const K* B, int N, StAcc* acc) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int q0 = tid - lane; q0 < N; q0 += RB_THREADS) {            // wave-uniform: 64 consecutive positions a wave
        const int q = q0 + lane;
        const bool valid = q < N;
        long long w = 0, tie = 0;
        int c1 = 0, h = -1, seg_n = 0;
        bool seg_first = false;
        if (valid) {
            const K key = B[q];
            h = (int)(StKey<K>::strat(key) & 63u);
            const RunBounds run = run_bounds(B, N, (K)(key >> 1), ProjCode{}, q);
            const RunBounds seg = run_bounds(B, N, StKey<K>::strat(key), ProjStrat<K>{}, q);
            if (key & 1) { w = run.first + run.past + 1 - 2 * seg.first; c1 = 1; }
            if (q == run.first) {
                const long long t = run.past - run.first;
                tie = t * t * t - t;
            }
            seg_first = q == seg.first;
            seg_n = seg.past - seg.first;
        }
        if (seg_first) acc->nh[h] = seg_n;
        const int h0 = __shfl(h, 0);                                 // position q0 is valid
        if (__all(!valid || h == h0)) {                              // one stratum under the wave: one atomic each
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) {
                w += __shfl_xor(w, ofs);
                tie += __shfl_xor(tie, ofs);
                c1 += __shfl_xor(c1, ofs);
            }
            if (lane == 0) {
                if (w) atomicAdd(&acc->w[h0], (unsigned long long)w);
                if (tie) atomicAdd(&acc->tie[h0], (unsigned long long)tie);
                if (c1) atomicAdd(&acc->n1h[h0], c1);
            }
        } else if (valid) {
            if (w) atomicAdd(&acc->w[h], (unsigned long long)w);
            if (tie) atomicAdd(&acc->tie[h], (unsigned long long)tie);
            if (c1) atomicAdd(&acc->n1h[h], c1);
        }
    }
}

// the bitonic network over A[0..P) and B[0..P), each on its own, through the same barriers
template <class K>
__device__ __forceinline__ void st_block_sort(unsigned long long* A, K* B, int P) {
    block_bitonic(P, [=](int i, int l, int desc) {
        const bool asc = desc == 0;
        const unsigned long long ax = A[i], ay = A[l];
        if ((ax > ay) == asc) { A[i] = ay; A[l] = ax; }
        const K bx = B[i], by = B[l];
        if ((bx > by) == asc) { B[i] = by; B[l] = bx; }
    });
}

__global__ void __launch_bounds__(RB_THREADS) strata_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                  const int32_t* __restrict__ g1, int n1,
                                                                  const int32_t* __restrict__ g2, int n2,
                                                                  const int32_t* __restrict__ st1,
                                                                  const int32_t* __restrict__ st2, int P, TwoSampleOut o) {
    extern __shared__ __align__(16) unsigned char smemst[];
    unsigned long long* A = reinterpret_cast<unsigned long long*>(smemst);      // [P] group << 32 | order bits: the medians
    unsigned long long* B64 = A + P;                                            // [P] the rank keys, wide ...
    uint32_t* B32 = reinterpret_cast<uint32_t*>(B64);                           // ... or narrow
    float* F = reinterpret_cast<float*>(B64);                                   // first the compaction buffer of the means
    __shared__ float leaf_sum[ST_LEAF_MAX];
    __shared__ float scratch8[ST_LEAF_MAX * 8];
    __shared__ int leaf_off[ST_LEAF_MAX + 1];
    __shared__ int wcnt[RB_THREADS / 64 + 1];
    __shared__ StAcc acc;
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = n1 + n2;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        // ---- per group: ordered compaction + numpy pairwise sum (np.sum: the identity 0 plus the tree)
        // (written out in strata.hip and ks.hip: as a struct + helper of rowsum.h the LDS layout and the kernel changed, A.17)
        const int nv1 = block_compact(prow, g1, n1, F, wcnt);
        const float sum1 = 0.0f + block_pairwise_sum<PW_DEPTH>(F, nv1, leaf_off, leaf_sum, scratch8, ST_LEAF_MAX);
        const int nv2 = block_compact(prow, g2, n2, F, wcnt);
        const float sum2 = 0.0f + block_pairwise_sum<PW_DEPTH>(F, nv2, leaf_off, leaf_sum, scratch8, ST_LEAF_MAX);
        bool tested = nv1 >= 3 && nv2 >= 3;                     // block-uniform; the informative strata may keep fewer
        double sd = 0.0, sv = 0.0;
        if (tested) {
            // ---- grid row or not; the two keys of every selected column, NaNs and padding last
            int off = 0;
            for (int j = tid; j < m; j += RB_THREADS) {
                const float v = prow[j < n1 ? g1[j] : g2[j - n1]];
                off |= (v == v && !key_of_ps(v).exact()) ? 1 : 0;
            }
            const bool grid = __syncthreads_or(off) == 0;       // (a barrier: the sums are done with F)
            for (int j = tid; j < P; j += RB_THREADS) {
                unsigned long long a = ~0ull, b64 = ~0ull;
                uint32_t b32 = PAD32;
                if (j < m) {
                    const bool in1 = j < n1;
                    const float v = prow[in1 ? g1[j] : g2[j - n1]];
                    if (v == v) {
                        const uint32_t st = (uint32_t)(in1 ? st1[j] : st2[j - n1]) & 63u;
                        a = two_group_median_key(v, in1);
                        if (grid) b32 = StKey<uint32_t>::make(st, v, in1);
                        else b64 = StKey<unsigned long long>::make(st, v, in1);
                    }
                }
                A[j] = a;
                if (grid) B32[j] = b32;
                else B64[j] = b64;
            }
            for (int h = tid; h < ST_MAX_STRATA; h += RB_THREADS) { acc.w[h] = 0ull; acc.tie[h] = 0ull; acc.n1h[h] = 0; acc.nh[h] = 0; }
            __syncthreads();
            const int N = nv1 + nv2;
            if (grid) {                                         // block-uniform
                st_block_sort<uint32_t>(A, B32, P);
                st_block_ranks<uint32_t>(B32, N, &acc);
            } else {
                st_block_sort<unsigned long long>(A, B64, P);
                st_block_ranks<unsigned long long>(B64, N, &acc);
            }
            __syncthreads();
            // ---- the strata, one per lane of every wave (each wave computes the same; thread 0 stores)
            double d, v;
            const int cnt = group_add<64>(st_stratum_terms(acc.n1h[lane], acc.nh[lane], (long long)acc.w[lane],
                                                           (long long)acc.tie[lane], d, v));
            sd = st_dd_lane_sum<64>(d);
            sv = st_dd_lane_sum<64>(v);
            tested = (cnt & 0xffff) >= 3 && (cnt >> 16) >= 3;
        }
        if (tid == 0) {
            double z = 0.0, p = 0.0;
            float med1 = 0.f, med2 = 0.f;
            if (tested) {
                st_finish(sd, sv, z, p);
                med1 = median_of_ord(A, nv1);                   // np.median on float32
                med2 = median_of_ord(A + nv1, nv2);
            }
            // (written out: through store_two_sample the two divisions leave the `tested` branch, and the kernel so changed
            // timed 0.2 - 0.5 % above the range of the one before it: EXPERIMENTS A.12)
            o.tested[row] = tested ? 1 : 0;
            o.p[row] = p;
            if (o.z) o.z[row] = z;
            o.med1[row] = med1;
            o.med2[row] = med2;
            o.mean1[row] = tested ? sum1 / (float)nv1 : 0.f;
            o.mean2[row] = tested ? sum2 / (float)nv2 : 0.f;
            o.delta[row] = med1 - med2;
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

}  // namespace

extern "C" int sdice_ranksum_strata_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_g1,
                                        int32_t n1, const int32_t* d_g2, int32_t n2, const int32_t* d_strat1,
                                        const int32_t* d_strat2, int32_t n_strata, uint8_t* d_tested, double* d_p,
                                        double* d_z, float* d_med1, float* d_med2, float* d_mean1, float* d_mean2,
                                        float* d_delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(check_two_groups("sdice_ranksum_strata", nullptr, n1, nullptr, n2, s, ST_MAX_GROUP, nullptr, nullptr, n_strata,
                            ST_MAX_STRATA));                   // (device lists: the counts)
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med1 && d_med2 && d_mean1 && d_mean2 && d_delta, "NULL output");
    SD_ARG(d_ps && d_g1 && d_g2 && d_strat1 && d_strat2, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    TwoSampleOut o{d_tested, d_p, d_z, d_med1, d_med2, d_mean1, d_mean2, d_delta};
    const int m = n1 + n2;
    if (n1 < 3 || n2 < 3) return zero_two_sample(ctx, n, o);         // no row can be tested
    if (m <= ST_GROUP_MAX)
        return with_group_launch(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "strata_group_kernel", (strata_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_g1, (int)n1, d_g2, (int)n2, d_strat1, d_strat2, ch, o);
            return SDICE_OK;
        });
    const int P = next_pow2(m, 128);
    const size_t lds = (size_t)P * 16;
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH_LDS(ctx, "strata_block_kernel", strata_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n,
                  (int)s, d_g1, (int)n1, d_g2, (int)n2, d_strat1, d_strat2, P, o);
    return SDICE_OK;
}

extern "C" int sdice_ranksum_strata(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* g1, int32_t n1,
                                    const int32_t* g2, int32_t n2, const int32_t* strat1, const int32_t* strat2,
                                    int32_t n_strata, uint8_t* tested, double* p, double* z, float* med1, float* med2,
                                    float* mean1, float* mean2, float* delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(g1 && g2 && strat1 && strat2, "index or stratum list is NULL");
    SD_TRY(check_two_groups(__func__, g1, n1, g2, n2, s, ST_MAX_GROUP, strat1, strat2, n_strata, ST_MAX_STRATA));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med1 && med2 && mean1 && mean2 && delta, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    TwoSampleOut o;
    float* d_ps;
    int32_t *dg1, *dg2, *ds1, *ds2;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dg1, g1, n1));
    SD_TRY(st.upload(&dg2, g2, n2));
    SD_TRY(st.upload(&ds1, strat1, n1));
    SD_TRY(st.upload(&ds2, strat2, n2));
    SD_TRY(stage_two_sample(st, n, {tested, p, z, med1, med2, mean1, mean2, delta}, &o));
    SD_TRY(sdice_ranksum_strata_dev(ctx, n, s, d_ps, dg1, n1, dg2, n2, ds1, ds2, n_strata, o.tested, o.p, o.z, o.med1, o.med2,
                                    o.mean1, o.mean2, o.delta));
    return st.download_results();
}
