// Per-row device helpers of the rank tests, lifted from ranksum.hip word for word for kruskal.hip: numpy's float32
// pairwise summation reproduced operation for operation, the ordered NaN-dropping compaction of a row's selected columns,
// np.median of a sorted run, and the float of a 3-decimal PS key.  ranksum.hip still carries its own copies: its source
// file stamps the committed counter pass that bench.py quotes (kernel_source_sha16), so it is left byte for byte as it
// was; when that pass is next retaken, ranksum.hip should include this header instead (the device code of its kernels
// came out identical with the include in place).
#pragma once
#include "common.h"

#define SD_WAVE_SYNC()                                        \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

namespace {

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
}  // namespace
