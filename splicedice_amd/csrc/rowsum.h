// Per-row helpers that the rank tests share.  Device: numpy's float32 pairwise summation reproduced operation for
// operation (by a block, by a wave and by a lane group), the ordered NaN-dropping compaction of a row's selected columns,
// np.median of a sorted run, the 3-decimal PS key of a float and its float back, the order-preserving bits of a float, the
// lane groups with their sums, bitonic sort and median, the key of a signed-rank difference, the workgroup's bitonic
// network, the tie-run bounds of a sorted array, the median search in the 16-bins-per-lane histograms of the counting
// kernels, the stores of a two-sample row.  Host: the eight output pointers of the two-sample tests, their "no row can be
// tested" block and their registration as the result fields of a host entry point (stage_two_sample, over common.h's
// HostStaging), the launch sizes of the wave-per-chunk and row-per-workgroup kernels, the width ladder of the lane-group
// kernels and their launch (with_group_width, with_group_launch), the launch pair of the k-set tests (kw_launch_pair); the
// checks of the column lists and the k-set limits are colcheck.h's (host only, no HIP), included here.  What each file
// takes:
//   ranksum.hip (K5)      PsKey, median_sorted, block_compact, the pairwise sums, find_bin, lanes_below; TwoSampleOut (as
//                         RsOut), zero_two_sample, stage_two_sample, the launch sizes, next_pow2, with_group_width
//   kruskal.hip (K12)     as ranksum.hip's kernels + f32_ord, median_of_ord, block_bitonic
//                         + the k-set section: the limits, KwSets, kw_stage_row / kw_walk_set (the first walk of the grid
//                         kernel), kw_block_sort_sets (the block kernel up to its medians), kw_plan, kw_launch_pair,
//                         kw_check_sets, check_columns, kw_chi2_sf
//   jonckheere.hip (K18)  as kruskal.hip's k-set section + kw_load_bins / kw_scan_bins, the launch sizes
//   friedman.hip (K21)    lanes_below, wave_pairwise_sum (FloatAt), f32_ord, median_of_ord, PAD32, kw_wave_max / kw_wave_min,
//                         kw_chi2_sf, the launch sizes; fr_check_sets (colcheck.h)
//   signedrank.hip (K13)  PsKey, f32_ord, LaneGroup, group_add / group_sum / group_sort / group_median, pair_diff_key,
//                         block_compact_by, block_pairwise_sum, block_bitonic, run_bounds, median_of_ord, store_two_sample,
//                         with_group_launch; TwoSampleOut, zero_two_sample, stage_two_sample, check_columns
//   spearman.hip (K14)    PsKey, f32_ord, LaneGroup and its sums, the block's compaction, sum, network and run bounds, the
//                         launch sizes, with_group_launch, check_columns
//   gram.hip              check_columns
//   exactrank.hip (K16)   PsKey, pair_diff_key, SD_WAVE_SYNC, row_launch_blocks; stage_two_sample, check_columns
//   strata.hip (K17)      PsKey, f32_ord, LaneGroup, group_add / group_sum / group_sort / group_median, block_compact,
//                         block_pairwise_sum, block_bitonic, run_bounds, two_group_median_key, median_of_ord,
//                         store_two_sample, the launch sizes, with_group_launch; TwoSampleOut, zero_two_sample,
//                         stage_two_sample, check_two_groups (with the stratum ids)
//   ks.hip (K19)          PsKey, f32_ord, LaneGroup, group_sum / group_sort / group_median, block_compact,
//                         block_pairwise_sum, block_bitonic, two_group_median_key, median_of_ord, store_two_sample, the
//                         launch sizes, with_group_launch; TwoSampleOut (D in the z slot), zero_two_sample,
//                         stage_two_sample (with `exact`), check_two_groups
//   shift.hip (K20)       PsKey, f32_ord / f32_unord, LaneGroup, group_add / group_sort, block_bitonic,
//                         two_group_median_key, kw_load_bins / kw_scan_bins, the launch sizes, with_group_launch;
//                         ShiftOut, the SH_ marks, f64_ord / f64_unord, shift_targets; check_two_groups
//   walsh.hip (K22)       PsKey, f32_ord / f32_unord, LaneGroup, group_add / group_sort, block_bitonic, kw_load_bins /
//                         kw_scan_bins, the launch sizes, with_group_launch, ShiftOut, the SH_ marks, f64_ord / f64_unord,
//                         shift_targets; check_columns
// (strata.hip and ks.hip: the pass front of the group kernels and the LDS + sums of the block kernels stay written out, A.17)
// Every helper is inlined into the kernels that call it and the kernels themselves stay in their .hip files, so a change
// to a helper here is a change to each kernel that uses it -- ranksum.hip's pairq and count kernels among them, whose
// committed counter pass is stamped with the hash of ranksum.hip alone and will not notice.
#pragma once
#include "common.h"
#include "colcheck.h"
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#define SD_WAVE_SYNC()                                        \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

namespace {

// The outputs of a two-sample test (ranksum.hip, signedrank.hip, strata.hip and, with `exact` beside them, exactrank.hip):
// [n] each, device pointers in a kernel's argument, host or device pointers on the host
struct TwoSampleOut {
    uint8_t* tested;
    double* p;
    double* z;       // may be NULL
    float* med1;
    float* med2;
    float* mean1;
    float* mean2;
    float* delta;
};

// the stores of a row: the fields of an untested row are 0 (p and z are the caller's), delta = med1 - med2
__device__ __forceinline__ void store_two_sample(const TwoSampleOut& o, int64_t row, bool tested, double p, double z, float med1,
                                                 float med2, float mean1, float mean2) {
    o.tested[row] = tested ? 1 : 0;
    o.p[row] = p;
    if (o.z) o.z[row] = z;
    o.med1[row] = tested ? med1 : 0.f;
    o.med2[row] = tested ? med2 : 0.f;
    o.mean1[row] = tested ? mean1 : 0.f;
    o.mean2[row] = tested ? mean2 : 0.f;
    o.delta[row] = tested ? med1 - med2 : 0.f;
}

__device__ __forceinline__ float median_sorted(const float* a, int nv) {
    // np.median: odd -> middle; even -> np.mean of the two middle values in float32
    const int h = nv >> 1;
    if (nv & 1) return a[h];
    return (a[h - 1] + a[h]) / 2.0f;
}

// float32(k / 1000.0) for k = 0..1000 without the table: the product with float32(0.001) plus one residual step is
// the correctly rounded quotient for every one of the 1001 values (checked exhaustively against the table's
// definition, tests/test_abi_and_host.py) -- three VALU instructions instead of an LDS look-up, which is what this
// kernel is short of
__device__ __forceinline__ float ps_of_key(float kf) {
    const float q = kf * 0.001f;
    return __builtin_fmaf(__builtin_fmaf(-q, 1000.0f, kf), 0.001f, q);
}

constexpr int RB_THREADS = 256;

// ordered compaction of the non-NaN values of ps[row, idx[0..cnt)] into dst; returns count
__device__ int block_compact(const float* __restrict__ prow, const int32_t* __restrict__ idx, int cnt,
                             float* dst, int* wcnt /* [RB_THREADS/64 + 1] shared */) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < cnt; c0 += RB_THREADS) {
        const int k = c0 + tid;
        float x = __builtin_nanf("");
        if (k < cnt) x = prow[idx[k]];
        const bool valid = x == x;
        const unsigned long long m = __ballot(valid);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int q = 0; q < RB_THREADS / 64; ++q) {
            if (q < w) woff += wcnt[q];
            tot += wcnt[q];
        }
        if (valid) dst[base + woff + pre] = x;
        base += tot;
        __syncthreads();
    }
    return base;
}

// numpy's pairwise_sum recursion  `n <= 128 ? leaf : sum(a, n2) + sum(a + n2, n - n2)`,
// n2 = n/2 - (n/2) % 8, unrolled at compile time to PW_DEPTH levels.  The larger half is up to
// len/2 + 7.5, so 4096 values can need SIX levels (4095 -> 2055 -> 1031 -> 519 -> 263 -> 135 -> 71)
// and up to 64 leaves.  Every thread walks it redundantly with block-uniform arguments: no stacks,
// no single-lane section.
constexpr int PW_DEPTH = 6;

template <int DEPTH>
__device__ __forceinline__ void pw_leaves(int off, int len, int* leaf_off, int& nl, bool writer) {
    if (DEPTH == 0 || len <= 128) {
        if (writer) leaf_off[nl] = off;
        ++nl;
    } else {
        int n2 = len / 2;
        n2 -= n2 % 8;
        pw_leaves<(DEPTH > 0 ? DEPTH - 1 : 0)>(off, n2, leaf_off, nl, writer);
        pw_leaves<(DEPTH > 0 ? DEPTH - 1 : 0)>(off + n2, len - n2, leaf_off, nl, writer);
    }
}

template <int DEPTH>
__device__ __forceinline__ float pw_combine(int len, const float* leaf_sum, int& next) {
    if (DEPTH == 0 || len <= 128) return leaf_sum[next++];
    int n2 = len / 2;
    n2 -= n2 % 8;
    const float l = pw_combine<(DEPTH > 0 ? DEPTH - 1 : 0)>(n2, leaf_sum, next);
    const float r = pw_combine<(DEPTH > 0 ? DEPTH - 1 : 0)>(len - n2, leaf_sum, next);
    return l + r;
}

// numpy pairwise_sum over a[0..n) in float32 by the whole block; result to all threads
template <int DEPTH>
__device__ float block_pairwise_sum(const float* a, int n, int* leaf_off /*[LEAF_MAX+1]*/, float* leaf_sum,
                                    float* scratch8 /* [LEAF_MAX*8] */, int leaf_max) {
    const int tid = threadIdx.x;
    (void)leaf_max;
    int nl = 0;
    pw_leaves<DEPTH>(0, n, leaf_off, nl, tid == 0);
    if (tid == 0) leaf_off[nl] = n;
    __syncthreads();
    for (int t = tid; t < nl * 8; t += blockDim.x) {
        const int L = t >> 3, j = t & 7;
        const int off = leaf_off[L], len = leaf_off[L + 1] - off;
        float r = 0.f;
        if (len >= 8) {
            r = a[off + j];
            for (int i = 8; i < len - (len % 8); i += 8) r += a[off + i + j];
        }
        scratch8[t] = r;
    }
    __syncthreads();
    for (int L = tid; L < nl; L += blockDim.x) {
        const int off = leaf_off[L], len = leaf_off[L + 1] - off;
        float res;
        if (len < 8) {
            res = 0.f;
            for (int i = 0; i < len; ++i) res += a[off + i];
        } else {
            const float* r = scratch8 + L * 8;
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int i = len - (len % 8); i < len; ++i) res += a[off + i];
        }
        leaf_sum[L] = res;
    }
    __syncthreads();
    int next = 0;
    const float out = pw_combine<DEPTH>(n, leaf_sum, next);
    __syncthreads();      // leaf_sum / leaf_off are reused by the next call
    return out;
}

// number of set bits of a wave mask below this lane (v_mbcnt_lo + v_mbcnt_hi: two instructions, no 64-bit mask per lane)
__device__ __forceinline__ int lanes_below(unsigned long long m, int base = 0) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, (uint32_t)base));
}

// key of a PS value v: rint(1000 v) clamped to 0..1000 (a value outside [0, 1] clamps to a key whose float it is not: no
// separate range check), and whether v is exactly float32(key / 1000).  A NaN is not exact and its key is never used.
// exact() is evaluated where it is asked for, so a caller's `a || b.exact()` skips it as the written-out test did.
struct PsKey {
    float v, kf;
    __device__ __forceinline__ int key() const { return (int)kf; }
    __device__ __forceinline__ bool exact() const { return ps_of_key(kf) == v; }
};
__device__ __forceinline__ PsKey key_of_ps(float v) {
    return {v, __builtin_amdgcn_fmed3f(__builtin_rintf(v * 1000.0f), 0.0f, 1000.0f)};
}

// element loaders of wave_pairwise_sum: floats as they are, 16-bit keys as float32(key / 1000)
struct FloatAt { const float* a; __device__ __forceinline__ float operator()(int i) const { return a[i]; } };
struct KeyAt { const unsigned short* k; __device__ __forceinline__ float operator()(int i) const { return ps_of_key((float)k[i]); } };

// numpy pairwise_sum of at(0..nv) by one wave, nv needing at most DEPTH halvings: lane = leaf*8 + j owns accumulator j
// of its leaf, 8 leaves per round; the 8 accumulators are folded with three xor-exchanges, which reproduces
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) because float addition is commutative.  leaf_off [2^DEPTH + 1] and leaf_sum
// [2^DEPTH] are the wave's own LDS.
template <int DEPTH, class At>
__device__ __forceinline__ float wave_pairwise_sum(At at, int nv, int lane, int* leaf_off, float* leaf_sum) {
    int nl = 0;
    pw_leaves<DEPTH>(0, nv, leaf_off, nl, lane == 0);
    if (lane == 0) leaf_off[nl] = nv;
    SD_WAVE_SYNC();
    const int j = lane & 7;
    for (int base = 0; base < nl; base += 8) {          // wave-uniform trip count
        const int L = base + (lane >> 3);
        int off = 0, len = 0;
        if (L < nl) { off = leaf_off[L]; len = leaf_off[L + 1] - off; }
        const int main_n = len - (len & 7);
        float r = 0.f;
        if (len >= 8) {
            r = at(off + j);
            for (int i = 8; i < main_n; i += 8) r += at(off + i + j);
        }
        r = r + __shfl_xor(r, 1);
        r = r + __shfl_xor(r, 2);
        r = r + __shfl_xor(r, 4);
        for (int i = (len >= 8 ? main_n : 0); i < len; ++i) r += at(off + i);
        if (j == 0 && L < nl) leaf_sum[L] = r;
    }
    SD_WAVE_SYNC();
    int next = 0;
    const float out = pw_combine<DEPTH>(nv, leaf_sum, next);
    SD_WAVE_SYNC();
    return out;
}

// Histogram of 1024 bins scanned by one wave, lane owns bins [16 lane, 16 lane + 16): the bin where the cumulative
// count crosses position `target`.  cum0 / tot are this lane's count below its 16 bins and inside them, a bin's count is
// (H[bin] >> SHIFT) & MASK.  The lane whose 16 bins contain the position is found with a ballot; its 16 counters are
// then examined by lanes 0..15 together (prefix by shuffles, crossing by a second ballot) -- uniform, no divergent walk.
// (The caller's values by reference: with by-value parameters the counting and the grid kernel are allocated a register
// or two fewer and come out up to 26 instructions longer or shorter; this way their code is what it was with the
// search written out in each.)
template <int SHIFT, unsigned MASK>
__device__ __forceinline__ int find_bin(const unsigned* const& H, const int& lane, int target, const int& cum0, const int& tot) {
    const int L = __ffsll((long long)__ballot(target >= cum0 && target < cum0 + tot)) - 1;
    const int base = __shfl(cum0, L);
    const unsigned wq = lane < 16 ? H[L * 16 + lane] : 0u;
    int inc = (int)((wq >> SHIFT) & MASK);
#pragma unroll
    for (int ofs = 1; ofs < 16; ofs <<= 1) {
        const int up = __shfl_up(inc, ofs);
        if (lane >= ofs) inc += up;
    }
    return L * 16 + (__ffsll((long long)__ballot(lane < 16 && target < base + inc)) - 1);
}

// order-preserving bits of a non-NaN float (-0.0 == +0.0), below 0xFFFFFFFF, and the float back (+0.0 for either zero):
// what the block kernels of kruskal.hip, signedrank.hip and spearman.hip sort and the others count on
__device__ __forceinline__ uint32_t f32_ord(float v) {
    const uint32_t b = __float_as_uint(v + 0.0f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float f32_unord(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// np.median of the nv smallest of K[0..), sorted ascending, whose low 32 bits are order-preserving bits
template <class T>
__device__ __forceinline__ float median_of_ord(const T* K, int nv) {
    const int h = nv >> 1;
    const float v1 = f32_unord((uint32_t)K[h]);
    return (nv & 1) ? v1 : (f32_unord((uint32_t)K[h - 1]) + v1) / 2.0f;
}

// what pads a sort of 32-bit keys: above every f32_ord and every key below
constexpr uint32_t PAD32 = 0xFFFFFFFFu;

// Sort key of a kept pair (x, y) of the signed-rank test (signedrank.hip's file comment): (code << 1) | (d > 0), code =
// |key_x - key_y| on a row of 3-decimal PS values (`grid`), else the bits of |x - y|; PAD32 for a zero difference.
// signedrank.hip ranks by it for z and exactrank.hip for the exact p: one function, so both see the same ranks.
__device__ __forceinline__ uint32_t pair_diff_key(float x, float y, bool grid) {
    if (grid) {
        const int d = key_of_ps(x).key() - key_of_ps(y).key();
        return d == 0 ? PAD32 : (((uint32_t)(d < 0 ? -d : d) << 1) | (d > 0 ? 1u : 0u));
    }
    const float d = x - y;
    return d == 0.0f ? PAD32 : ((__float_as_uint(fabsf(d)) << 1) | (d > 0.0f ? 1u : 0u));
}

// ---- lane groups: P lanes (a power of two) own a row, 64 / P rows side by side in a wave, a pass of the chunk loop takes
// the rows r0 .. r0 + R of the chunk and lane i of the wave keeps what the chunk's i-th row came to
template <int P>
struct LaneGroup {
    static constexpr int R = 64 / P;
    static constexpr unsigned long long MASK = P == 64 ? ~0ull : ((1ull << (P & 63)) - 1ull);      // of a ballot shifted down to the group
    // the lane that holds group q's value for lane r0 + q, and whether this lane keeps a row of the pass
    static __device__ __forceinline__ int src(int lane, int r0) { return ((lane - r0) * P) & 63; }
    static __device__ __forceinline__ bool mine(int lane, int r0) { return lane >= r0 && lane < r0 + R; }
};

// sum over the group, to every lane of it
template <int P>
__device__ __forceinline__ int group_add(int v) {
#pragma unroll
    for (int ofs = 1; ofs < P; ofs <<= 1) v += __shfl_xor(v, ofs);
    return v;
}

// ascending bitonic sort of one value per lane (gl = lane in the group) inside aligned groups of P lanes
template <int P, class T>
__device__ __forceinline__ T group_sort(T v, int gl) {
#pragma unroll
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const T other = __shfl_xor(v, j);
            const bool upper = (gl & j) != 0;
            const bool asc = (gl & k) == 0;              // k == P: ascending everywhere
            const T lo = v < other ? v : other, hi = v < other ? other : v;
            v = (asc != upper) ? lo : hi;
        }
    }
    return v;
}

// np.median of the group's nv sorted order-preserving values (lane g0 + i holds the i-th smallest)
__device__ __forceinline__ float group_median(uint32_t sorted, int g0, int nv) {
    const int h = nv >> 1;
    const float v1 = f32_unord(__shfl(sorted, g0 + h));
    const float v0 = f32_unord(__shfl(sorted, g0 + (h > 0 ? h - 1 : 0)));
    return (nv & 1) ? v1 : (v0 + v1) / 2.0f;
}

// numpy pairwise_sum of A[0..nv), nv <= 64 (one leaf), by a group of P >= 8 lanes, every lane of the group gets it: for
// nv >= 8 lane j (mod 8) owns accumulator j, folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) by three xor exchanges as
// in wave_pairwise_sum; then the tail (or, below 8 values, all of them) one after another
__device__ __forceinline__ float group_sum(const float* A, int nv, int gl) {
    const int main_n = nv & ~7, j = gl & 7;
    float r = 0.f;
    if (nv >= 8) {
        r = A[j];
        for (int i = 8; i < main_n; i += 8) r += A[i + j];
    }
    r = r + __shfl_xor(r, 1);
    r = r + __shfl_xor(r, 2);
    r = r + __shfl_xor(r, 4);
    if (nv < 8) r = 0.f;
    for (int i = (nv >= 8 ? main_n : 0); i < nv; ++i) r += A[i];
    return r;
}

// ---- a row per workgroup
// Ordered NaN-dropping compaction by the whole block, the general form: load(q) gives position q's value, a float or a
// pair of them (NaN past the list: q runs to cnt rounded up to the block), kept when it holds no NaN; sink(q, pos,
// kept, v) follows with pos = the number of kept positions below q.  Returns the count; ends with a barrier.
// (block_compact above is the one-list case with the prefix from a 64-bit mask, as ranksum.hip's and kruskal.hip's
// kernels were built with.)
__device__ __forceinline__ bool holds_no_nan(float v) { return v == v; }
__device__ __forceinline__ bool holds_no_nan(float2 v) { return v.x == v.x && v.y == v.y; }
template <class Load, class Sink>
__device__ int block_compact_by(int cnt, int* wcnt /* [RB_THREADS/64] shared */, Load load, Sink sink) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < cnt; c0 += RB_THREADS) {
        const int q = c0 + tid;
        const auto v = load(q);
        const bool valid = holds_no_nan(v);
        const unsigned long long mk = __ballot(valid);
        if (lane == 0) wcnt[w] = __popcll(mk);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int i = 0; i < RB_THREADS / 64; ++i) {
            if (i < w) woff += wcnt[i];
            tot += wcnt[i];
        }
        sink(q, base + woff + lanes_below(mk), valid, v);
        base += tot;
        __syncthreads();
    }
    return base;
}

// The bitonic sorting network over positions 0..P) (a power of two) by the whole block: cx(i, l, desc) compare-exchanges
// positions i < l, ascending when desc == 0; ends with a barrier
template <class CX>
__device__ void block_bitonic(int P, CX cx) {
    const int tid = threadIdx.x;
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += RB_THREADS) {
                const int l = i ^ j;
                if (l > i) cx(i, l, i & kk);
            }
            __syncthreads();
        }
    }
}

// Bounds [first, past) of the run of `code` in K[0..n), ascending under proj, by two binary searches.  With a position
// `at` of the run given the searches stay on its two sides; without, the second starts where the first ended.
struct RunBounds { int first, past; };
struct ProjSelf { template <class T> __device__ __forceinline__ T operator()(T v) const { return v; } };
struct ProjAbove1 { __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return v >> 1; } };
template <class T, class C, class Proj>
__device__ __forceinline__ RunBounds run_bounds(const T* K, int n, C code, Proj proj, int at = -1) {
    int lo = 0, hi = at < 0 ? n : at;                   // first position with a code >= this one
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (proj(K[mid]) < code) lo = mid + 1; else hi = mid; }
    const int first = lo;
    if (at >= 0) lo = at + 1;
    hi = n;                                             // first position with a larger code
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (proj(K[mid]) <= code) lo = mid + 1; else hi = mid; }
    return {first, lo};
}

// Two column groups by the workgroup (strata.hip, ks.hip): the key the medians are sorted by -- (group << 32 | order
// bits) of a selected value, a NaN last with the padding
__device__ __forceinline__ unsigned long long two_group_median_key(float v, bool in1) {
    return v == v ? ((unsigned long long)(in1 ? 0u : 1u) << 32) | f32_ord(v) : ~0ull;
}

// ---- the estimates with an interval (shift.hip, walsh.hip): the five outputs, what a lane keeps of its row beside the
// images of its order statistics, the order-preserving bits of a float64 and which order statistics are wanted
struct ShiftOut {
    uint8_t* tested;
    double* shift;
    double* lo;
    double* hi;
    int32_t* rank;
};

constexpr int SH_TESTED = 1, SH_OFF = 2, SH_INF = 4, SH_ODD = 8;

// order-preserving bits of a non-NaN float64 that is not -0.0, and the float64 back
__device__ __forceinline__ unsigned long long f64_ord(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double f64_unord(unsigned long long o) {
    return __longlong_as_double((long long)((o & 0x8000000000000000ull) ? (o ^ 0x8000000000000000ull) : ~o));
}

// the four order statistics wanted of M differences (or Walsh averages): the middle ones (twice the same for odd M), c and
// its mirror
__device__ __forceinline__ void shift_targets(int M, int c, int (&k)[4]) {
    k[0] = (M + 1) >> 1;
    k[1] = (M >> 1) + 1;
    k[2] = c;
    k[3] = M + 1 - c;
}

// ---- k sample sets (kruskal.hip, jonckheere.hip): the limits, the sets as a kernel argument, the first walk of a wave
// over a row of 3-decimal values and the (set, value) sort of a workgroup over any row
constexpr int KW_BINS = 1024;            // 1001 used
constexpr int KW_SUM_PIECE = 8192;       // np.add.reduce hands the pairwise loop at most np.getbufsize() = 8192 values at a time
constexpr int KW_PW_DEPTH = 7;           // levels of numpy's pairwise recursion inside a piece (7689 values are the first to need 7)
constexpr int KW_LEAF_MAX = 128;         // a part after 7 halvings is at most 8192 / 128 + 15 values long
constexpr unsigned char KW_REDO = 0xFF;  // `tested` mark: row left to the block kernel by the grid kernel

struct KwSets { int32_t ptr[KW_MAX_SETS + 1]; };

__device__ __forceinline__ float kw_wave_max(float v) {
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v = fmaxf(v, __shfl_xor(v, ofs));
    return v;
}
__device__ __forceinline__ float kw_wave_min(float v) {
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v = fminf(v, __shfl_xor(v, ofs));
    return v;
}

// chi2.sf(h, df), integer df >= 1 (kruskal.hip, friedman.hip): the closed series with positive terms only (x = h / 2)
//   even df: e^-x sum_{j < df/2} x^j / j!      odd df: erfc(sqrt x) + e^-x sum_{j=1..(df-1)/2} x^(j-1/2) / Gamma(j+1/2)
__device__ double kw_chi2_sf(double h, int df) {
    const double x = 0.5 * h;
    double sum = 0.0;
    const double e = exp(-0.5 * x);      // e^-x in two factors: e^-x alone is subnormal from x = 709, where the sum can still lift p above 1e-280
    if (df & 1) {
        const double r = sqrt(x);
        double term = r * 1.12837916709551257390;        // x^(1/2) / Gamma(3/2) = 2 sqrt(x / pi)
        const int m = (df - 1) >> 1;
        for (int j = 1; j <= m; ++j) {
            sum += term;
            term *= x / ((double)j + 0.5);
        }
        return erfc(r) + (sum * e) * e;
    }
    double term = 1.0;
    const int m = df >> 1;
    for (int j = 0; j < m; ++j) {
        sum += term;
        term *= x / (double)(j + 1);
    }
    return (sum * e) * e;
}

// np.sum of the contiguous float32 array float32(K[0..nv) / 1000): the identity 0 plus the pairwise tree of every piece
// of KW_SUM_PIECE values, the pieces added left to right (at most two: nv <= KW_MAX_N).  The whole-array tree is a
// different sum above one piece.
__device__ __forceinline__ float kw_wave_sum_keys(const unsigned short* K, int nv, int lane, int* leaf_off, float* leaf_sum) {
    float sum = 0.0f + wave_pairwise_sum<KW_PW_DEPTH>(KeyAt{K}, min(nv, KW_SUM_PIECE), lane, leaf_off, leaf_sum);
    if (nv > KW_SUM_PIECE)               // wave-uniform
        sum += wave_pairwise_sum<KW_PW_DEPTH>(KeyAt{K + KW_SUM_PIECE}, nv - KW_SUM_PIECE, lane, leaf_off, leaf_sum);
    return sum;
}

// The wave's LDS in the grid kernels: Htot[1024] | Hset[1024] | leaf_sum[leaf_cap] | leaf_off[leaf_cap + 1] | keys[nsel] u16
struct KwWaveLds {
    unsigned* Htot;
    unsigned* Hset;
    float* leaf_sum;
    int* leaf_off;
    unsigned short* keys;
    __device__ __forceinline__ KwWaveLds(unsigned char* base, int leaf_cap) {
        Htot = reinterpret_cast<unsigned*>(base);
        Hset = Htot + KW_BINS;
        leaf_sum = reinterpret_cast<float*>(Hset + KW_BINS);
        leaf_off = reinterpret_cast<int*>(leaf_sum + leaf_cap);
        keys = reinterpret_cast<unsigned short*>(leaf_off + leaf_cap + 1);
    }
};

// A row's selected columns staged as keys (0xFFFF = NaN); false when a value is not its key's float (wave-uniform).  On
// true both histograms are cleared and the wave is in step.
__device__ __forceinline__ bool kw_stage_row(const float* __restrict__ prow, const int32_t* __restrict__ cols, int nsel,
                                             const KwWaveLds& L, int lane) {
    bool ok = true;
    for (int j = lane; j < nsel; j += 64) {
        const float v = __builtin_nontemporal_load(prow + cols[j]);
        const PsKey pk = key_of_ps(v);
        ok = ok && (v != v || pk.exact());
        L.keys[j] = (v != v) ? (unsigned short)0xFFFF : (unsigned short)pk.key();
    }
    if (__ballot(!ok) != 0ull) return false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        reinterpret_cast<uint4*>(L.Htot)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4*>(L.Hset)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
    }
    SD_WAVE_SYNC();
    return true;
}

// this lane's 16 bins of a histogram
__device__ __forceinline__ void kw_load_bins(const unsigned* H, int lane, unsigned (&w)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 t4 = reinterpret_cast<const uint4*>(H)[lane * 4 + q];
        w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w;
    }
}

// this lane's count inside its 16 bins (tot) and the inclusive scan of that over the lanes
__device__ __forceinline__ int kw_scan_bins(const unsigned (&w)[16], int lane, int& tot) {
    tot = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += (int)w[q];
    int pre = tot;
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) {
        const int up = __shfl_up(pre, ofs);
        if (lane >= ofs) pre += up;
    }
    return pre;
}

// One set of the first walk: K[0..cnt) are the set's staged keys.  Ordered compaction in place (a key moves to a slot at
// or below its own; every lane reads its key of the round before any lane writes) + the set's histogram; with fewer
// than 3 kept values the count is returned at once (wave-uniform, the histogram is left as it is).  Then the numpy-order
// mean, the median from the histogram's scan, before_join(w, t) with this lane's 16 bins of the set and of the total
// of the sets BEFORE it, and the set joins the total, its own bins cleared.
template <class BeforeJoin>
__device__ __forceinline__ int kw_walk_set(unsigned short* K, int cnt, const KwWaveLds& L, int lane, float& med, float& mean,
                                           BeforeJoin before_join) {
    int nv = 0;
    for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int j = c0 + lane;
        const unsigned key = j < cnt ? (unsigned)K[j] : 0xFFFFu;
        const bool valid = key != 0xFFFFu;
        const unsigned long long m = __ballot(valid);
        SD_WAVE_SYNC();
        if (valid) {
            K[lanes_below(m, nv)] = (unsigned short)key;
            atomicAdd(&L.Hset[key], 1u);
        }
        nv += __popcll(m);
    }
    SD_WAVE_SYNC();
    if (nv < 3) return nv;
    const float sum = kw_wave_sum_keys(K, nv, lane, L.leaf_off, L.leaf_sum);
    // scan of the set's histogram, lane owns bins [16 lane, 16 lane + 16)
    unsigned w[16];
    kw_load_bins(L.Hset, lane, w);
    int tot;
    const int cum0 = kw_scan_bins(w, lane, tot) - tot;
    // the median: the bins where the cumulative count crosses the middle positions
    const int hh = nv >> 1;
    const int bin1 = find_bin<0, ~0u>(L.Hset, lane, hh, cum0, tot);
    const int bin0 = (nv & 1) ? bin1 : find_bin<0, ~0u>(L.Hset, lane, hh - 1, cum0, tot);      // wave-uniform branch
    const float v0 = ps_of_key((float)bin0), v1 = ps_of_key((float)bin1);
    med = (nv & 1) ? v1 : (v0 + v1) / 2.0f;      // np.median on float32
    mean = sum / (float)nv;
    SD_WAVE_SYNC();          // find_bin's readers are done with Hset
    unsigned t[16];
    kw_load_bins(L.Htot, lane, t);
    before_join(w, t);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        reinterpret_cast<uint4*>(L.Htot)[lane * 4 + q] =
            make_uint4(t[4 * q] + w[4 * q], t[4 * q + 1] + w[4 * q + 1], t[4 * q + 2] + w[4 * q + 2], t[4 * q + 3] + w[4 * q + 3]);
        reinterpret_cast<uint4*>(L.Hset)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
    }
    SD_WAVE_SYNC();
    return nv;
}

// The workgroup's named LDS in the block kernels (the sort area K[P] is dynamic)
struct KwBlockLds {
    float leaf_sum[KW_LEAF_MAX];
    float scratch8[KW_LEAF_MAX * 8];
    int leaf_off[KW_LEAF_MAX + 1];
    int wcnt[RB_THREADS / 64 + 1];
    int sptr[KW_MAX_SETS + 1];
    int nvs[KW_MAX_SETS];
    int starts[KW_MAX_SETS + 1];
    float meanS[KW_MAX_SETS], medS[KW_MAX_SETS];
};

// One row by the workgroup.  Per set: ordered compaction + numpy pairwise sum (the key area is the float buffer); false
// (block-uniform) when a set keeps fewer than 3 values.  Otherwise sh.nvs / sh.meanS hold the sets' counts and means,
// K[0..P) the 64-bit keys (set << 32 | order bits of the value) sorted ascending, NaNs and padding last, so set i is the
// sorted run K[sh.starts[i] .. sh.starts[i + 1]), and sh.medS its np.median; ends with a barrier.
__device__ __forceinline__ bool kw_block_sort_sets(const float* __restrict__ prow, const int32_t* __restrict__ cols, int k, int P,
                                                   unsigned long long* K, KwBlockLds& sh) {
    const int tid = threadIdx.x;
    float* F = reinterpret_cast<float*>(K);
    const int nsel = sh.sptr[k];
    for (int i = 0; i < k; ++i) {
        const int a = sh.sptr[i];
        const int nv = block_compact(prow, cols + a, sh.sptr[i + 1] - a, F, sh.wcnt);
        if (nv < 3) return false;                // block-uniform
        // np.sum: 0 + the tree of the first KW_SUM_PIECE values (+ the tree of the rest), see kw_wave_sum_keys; the
        // leading 0 makes a sum of -0.0 values +0.0 as numpy's is
        float sum = 0.0f + block_pairwise_sum<KW_PW_DEPTH>(F, min(nv, KW_SUM_PIECE), sh.leaf_off, sh.leaf_sum, sh.scratch8, KW_LEAF_MAX);
        if (nv > KW_SUM_PIECE)                   // block-uniform
            sum += block_pairwise_sum<KW_PW_DEPTH>(F + KW_SUM_PIECE, nv - KW_SUM_PIECE, sh.leaf_off, sh.leaf_sum, sh.scratch8, KW_LEAF_MAX);
        if (tid == 0) { sh.nvs[i] = nv; sh.meanS[i] = sum / (float)nv; }
    }
    // ---- keys (set, value), NaNs and padding last; sort; medians
    for (int j = tid; j < P; j += RB_THREADS) {
        unsigned long long key = ~0ull;
        if (j < nsel) {
            const float v = prow[cols[j]];
            if (v == v) {
                int lo = 0, hi = k;              // the set of selection j: last i with sptr[i] <= j
                while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (sh.sptr[m] <= j) lo = m; else hi = m; }
                key = ((unsigned long long)lo << 32) | f32_ord(v);
            }
        }
        K[j] = key;
    }
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < k; ++i) { sh.starts[i] = acc; acc += sh.nvs[i]; }
        sh.starts[k] = acc;
    }
    __syncthreads();
    block_bitonic(P, [K](int i, int l, int desc) {
        const bool asc = desc == 0;
        const unsigned long long x = K[i], y = K[l];
        if ((x > y) == asc) { K[i] = y; K[l] = x; }
    });
    if (tid < k) sh.medS[tid] = median_of_ord(K + sh.starts[tid], sh.nvs[tid]);        // np.median on float32
    __syncthreads();
    return true;
}

// Host: rows of one wave's chunk in the wave-per-row kernels -- as many (64 at most) as keeps every wave slot of the
// chip (32 per CU) busy twice over
inline int rows_per_chunk(int n_cu, int64_t n) {
    const int64_t slots = (int64_t)n_cu * 32;
    int ch = 64;
    while (ch > 1 && sd_ceil_div(n, ch) < 2 * slots) ch >>= 1;
    return ch;
}

// Host: workgroups of `waves` waves for a kernel whose waves walk chunks of ch rows, every wave slot of the chip filled
// at most once; and of a kernel whose workgroups walk n rows (or n blocks of rows), 8 a CU at most
inline int64_t wave_launch_blocks(const sdice_ctx* ctx, int64_t n, int ch, int waves) {
    return std::min(sd_ceil_div(sd_ceil_div(n, ch), waves), (int64_t)ctx->n_cu * 32 / waves);
}
inline int64_t row_launch_blocks(const sdice_ctx* ctx, int64_t n) { return std::min(n, (int64_t)ctx->n_cu * 8); }

// Host: the power of two from `from` (one itself) up that is not below v
inline int next_pow2(int v, int from) {
    while (from < v) from <<= 1;
    return from;
}

// Host: the lane-group width of m <= 64 selected columns -- 8, 16, 32 or 64, none below FROM -- handed to launch as a
// std::integral_constant, so that a generic lambda picks its kernel<P> and keeps its own argument list
template <int FROM = 8, class Launch>
inline int with_group_width(int m, Launch launch) {
    if constexpr (FROM <= 8)
        if (m <= 8) return launch(std::integral_constant<int, 8>{});
    if constexpr (FROM <= 16)
        if (m <= 16) return launch(std::integral_constant<int, 16>{});
    if (m <= 32) return launch(std::integral_constant<int, 32>{});
    return launch(std::integral_constant<int, 64>{});
}

// Host: the launch of a lane-group kernel over n rows of m <= 64 selected columns -- workgroups of GROUP_WAVES waves
// that walk chunks of ch rows, no dynamic LDS; launch(width, ch, blocks) names the kernel<width> and its arguments
constexpr int GROUP_WAVES = 4;
template <int FROM = 8, class Launch>
inline int with_group_launch(const sdice_ctx* ctx, int64_t n, int m, Launch launch) {
    const int ch = rows_per_chunk(ctx->n_cu, n);
    const int64_t blocks = wave_launch_blocks(ctx, n, ch, GROUP_WAVES);
    return with_group_width<FROM>(m, [&](auto width) -> int { return launch(width, ch, blocks); });
}

// Host: the sets as the kernels take them, the launch shape of a grid kernel over KwWaveLds and the sort length of a
// block kernel
struct KwPlan {
    KwSets sets;
    int leaf_cap, wstride, waves, P;
    size_t grid_lds, block_lds;
};
inline KwPlan kw_plan(const int32_t* set_ptr, int k) {
    KwPlan pl;
    int maxset = 0;
    for (int i = 0; i <= KW_MAX_SETS; ++i) pl.sets.ptr[i] = i <= k ? set_ptr[i] : set_ptr[k];
    for (int i = 0; i < k; ++i) maxset = std::max(maxset, (int)(set_ptr[i + 1] - set_ptr[i]));
    const int nsel = set_ptr[k];
    // Leaves of the pairwise recursion over a piece of at most KW_SUM_PIECE values: after d halvings a part is at most
    // piece / 2^d + 15 long, a leaf from 128 down
    const int piece = std::min(maxset, KW_SUM_PIECE);
    pl.leaf_cap = 1;
    while (pl.leaf_cap < KW_LEAF_MAX && piece > 113 * pl.leaf_cap) pl.leaf_cap <<= 1;
    pl.wstride = (int)((2 * KW_BINS * 4 + (2 * pl.leaf_cap + 1) * 4 + 2 * nsel + 15) & ~15);
    const int waves = 64 * 1024 / pl.wstride;        // the workgroup is sized from the LDS a wave needs
    pl.waves = waves > 4 ? 4 : (waves < 1 ? 1 : waves);
    pl.grid_lds = (size_t)pl.waves * pl.wstride;
    pl.P = next_pow2(nsel, 2);
    pl.block_lds = (size_t)pl.P * 8;
    return pl;
}

// Host: the two launches of a k-set test -- the grid kernel over every row, then the block kernel over the rows it marked
// KW_REDO
template <auto GridKernel, auto BlockKernel, class Out>
inline int kw_launch_pair(sdice_ctx* ctx, const char* grid_name, const char* block_name, const KwPlan& pl, const float* d_ps,
                          int64_t n, int s, const int32_t* d_cols, int k, const Out& o) {
    const int ch = rows_per_chunk(ctx->n_cu, n);
    SD_LAUNCH_LDS(ctx, grid_name, GridKernel, dim3((unsigned)wave_launch_blocks(ctx, n, ch, pl.waves)), dim3(pl.waves * 64),
                  pl.grid_lds, d_ps, n, s, d_cols, pl.sets, k, ch, pl.wstride, pl.leaf_cap, o);
    SD_LAUNCH_LDS(ctx, block_name, BlockKernel, dim3((unsigned)row_launch_blocks(ctx, sd_ceil_div(n, RB_THREADS))),
                  dim3(RB_THREADS), pl.block_lds, d_ps, n, s, d_cols, pl.sets, k, pl.P, 1, o);
    return SDICE_OK;
}

// Host: "no row can be tested" -- every field of the n rows is 0, queued on the context's stream
inline int zero_two_sample(sdice_ctx* ctx, int64_t n, const TwoSampleOut& o) {
    SD_HIP(hipMemsetAsync(o.tested, 0, (size_t)n, ctx->stream));
    SD_HIP(hipMemsetAsync(o.p, 0, (size_t)n * 8, ctx->stream));
    if (o.z) SD_HIP(hipMemsetAsync(o.z, 0, (size_t)n * 8, ctx->stream));
    for (float* q : {o.med1, o.med2, o.mean1, o.mean2, o.delta}) SD_HIP(hipMemsetAsync(q, 0, (size_t)n * 4, ctx->stream));
    return SDICE_OK;
}

// Host: the two-sample results of a host entry point (h: the caller's arrays, h.z and h_exact may be NULL) as one block
// of its HostStaging; *d gets the device pointers the _dev call writes, *d_exact that of `exact` where the test has one
inline int stage_two_sample(HostStaging& st, int64_t n, TwoSampleOut h, TwoSampleOut* d, uint8_t* h_exact = nullptr,
                            uint8_t** d_exact = nullptr) {
    st.result(&d->tested, h.tested, n);
    if (d_exact) st.result(d_exact, h_exact, n);
    st.result(&d->p, h.p, n);
    st.result(&d->z, h.z, n);
    st.result(&d->med1, h.med1, n);
    st.result(&d->med2, h.med2, n);
    st.result(&d->mean1, h.mean1, n);
    st.result(&d->mean2, h.mean2, n);
    st.result(&d->delta, h.delta, n);
    return st.alloc_results();
}
}  // namespace
