// K12: Kruskal-Wallis H test per junction row across k >= 2 sample sets + per-set median / mean.
//
// scipy.stats.kruskal per row under the row rules of the two-set path (compareSampleSets.py:216-224): per set the row's
// values at the set's columns with NaNs dropped, the row is tested when every set keeps >= 3 values; average ranks over
// all N kept values; p = chi2.sf(H, k - 1).  A row whose N values are all equal stays tested with H = 0, p = 1.
//
// Arithmetic.  The textbook H = 12/(N(N+1)) sum R_i^2/n_i - 3(N+1) subtracts two numbers near 3(N+1); here the centred
// form is used, in integers up to the last step:
//   r2(v) = 2 * average rank of value v = 2 #{x < v} + #{x == v} + 1          (integer)
//   D_i   = sum of r2 over set i  -  n_i (N + 1)                               (integer, = 2 R_i - n_i (N + 1))
//   H     = 3/(N(N+1)) * sum_i D_i^2/n_i / T,   T = 1 - sum(t^3 - t)/(N^3 - N)
//         = 3 (N - 1) * S / (N^3 - N - sum(t^3 - t)),   S = sum_i D_i^2 / n_i  (float64; the divisor is an integer)
// S is summed over the SORTED terms with a fixed tree, so H does not depend on the order the sets are given in.
// chi2.sf for integer df is the finite series with positive terms only (x = H/2):
//   even df: e^-x sum_{j < df/2} x^j / j!      odd df: erfc(sqrt x) + e^-x sum_{j=1..(df-1)/2} x^(j-1/2) / Gamma(j+1/2)
//
// Kernels:
//   kruskal_grid_kernel: rows whose selected values all are 3-decimal PS values float32(key / 1000), key = 0..1000 (all
//       that compare_sample_sets ever reads).  One WAVE per row, nothing is sorted: the row's selected columns are
//       staged in LDS as 16-bit keys; the sets are walked one after another -- compaction (NaNs dropped, order kept),
//       1001-bin histogram of the set, numpy-order mean, median from the histogram's scan, histogram added into the
//       row's total; the total is scanned into r2 per bin and sum(t^3 - t); a second walk sums r2 per set.  Set i's
//       scalars live in lane i (k <= 64).  Any other row is marked KW_REDO in `tested` and left to
//   kruskal_block_kernel: any finite float32 values, one workgroup per row.  Means as ranksum_block_kernel (ordered
//       compaction + numpy pairwise sum), then two bitonic sorts of 64-bit keys in LDS: by (set, value) for the
//       medians, by (value, set) for the ranks (run bounds by binary search, r2 summed per set with LDS atomics).
//
// rowsum.h: the compaction, the pairwise sums, find_bin, the order bits of a float, np.median of sorted order bits, the
// block's bitonic network, the launch sizes and the column check.
#include "common.h"
#include <math.h>
#include <algorithm>
#include "rowsum.h"

namespace {

constexpr int KW_MAX_SETS = 64;
constexpr int KW_MAX_N = 16384;          // selected columns per row, both kernels (block kernel: 8 B of LDS per column)
constexpr int KW_BINS = 1024;            // 1001 used
constexpr int KW_SUM_PIECE = 8192;       // np.add.reduce hands the pairwise loop at most np.getbufsize() = 8192 values at a time
constexpr int KW_PW_DEPTH = 7;           // levels of numpy's pairwise recursion inside a piece (7689 values are the first to need 7)
constexpr int KW_LEAF_MAX = 128;         // a part after 7 halvings is at most 8192 / 128 + 15 values long
constexpr unsigned char KW_REDO = 0xFF;  // `tested` mark: row left to the block kernel by the grid kernel

struct KwSets { int32_t ptr[KW_MAX_SETS + 1]; };
struct KwOut {
    uint8_t* tested;
    double* p;
    double* h;       // may be NULL
    float* med;      // [k][n]
    float* mean;     // [k][n]
    float* delta;
};

// chi2.sf(h, df), integer df >= 1: the closed series (see the file comment)
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

// H and p of a tested row from the integer pieces
__device__ __forceinline__ void kw_finish(double S, long long N, long long tie, int k, double& H, double& p) {
    const long long den = N * N * N - N - tie;           // (N^3 - N) T
    if (den == 0) { H = 0.0; p = 1.0; return; }          // every value equal
    H = 3.0 * S * (double)(N - 1) / (double)den;
    p = kw_chi2_sf(H, k - 1);
}

// sum of the 64 lanes' non-negative terms, independent of which lane holds which: ascending bitonic sort across the
// wave, then a fixed butterfly (both partners of an exchange add the same two numbers)
__device__ __forceinline__ double kw_sorted_sum(double v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const double other = __shfl_xor(v, j);
            const bool upper = (lane & j) != 0;
            const bool asc = (lane & k) == 0;            // k == 64: ascending everywhere
            const double lo = fmin(v, other), hi = fmax(v, other);
            v = (asc != upper) ? lo : hi;
        }
    }
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) v += __shfl_xor(v, ofs);
    return v;
}

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

// np.sum of the contiguous float32 array float32(K[0..nv) / 1000): the identity 0 plus the pairwise tree of every piece
// of KW_SUM_PIECE values, the pieces added left to right (at most two: nv <= KW_MAX_N).  The whole-array tree is a
// different sum above one piece.
__device__ __forceinline__ float kw_wave_sum_keys(const unsigned short* K, int nv, int lane, int* leaf_off, float* leaf_sum) {
    float sum = 0.0f + wave_pairwise_sum<KW_PW_DEPTH>(KeyAt{K}, min(nv, KW_SUM_PIECE), lane, leaf_off, leaf_sum);
    if (nv > KW_SUM_PIECE)               // wave-uniform
        sum += wave_pairwise_sum<KW_PW_DEPTH>(KeyAt{K + KW_SUM_PIECE}, nv - KW_SUM_PIECE, lane, leaf_off, leaf_sum);
    return sum;
}

// ------------------------------------------------------------------ grid path: one wave per row
// LDS per wave (wstride bytes): Htot[1024] | Hset[1024] | leaf_sum[leaf_cap] | leaf_off[leaf_cap + 1] | keys[nsel] u16
__global__ void __launch_bounds__(256) kruskal_grid_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                           const int32_t* __restrict__ cols, KwSets sets, int k, int ch,
                                                           int wstride, int leaf_cap, KwOut o) {
    extern __shared__ __align__(16) unsigned char smemk[];
    __shared__ int sptr[KW_MAX_SETS + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = blockDim.x >> 6;
    unsigned* Htot = reinterpret_cast<unsigned*>(smemk + (size_t)wave * wstride);
    unsigned* Hset = Htot + KW_BINS;
    float* leaf_sum = reinterpret_cast<float*>(Hset + KW_BINS);
    int* leaf_off = reinterpret_cast<int*>(leaf_sum + leaf_cap);
    unsigned short* keys = reinterpret_cast<unsigned short*>(leaf_off + leaf_cap + 1);
    for (int i = threadIdx.x; i <= k; i += blockDim.x) sptr[i] = sets.ptr[i];
    __syncthreads();
    const int nsel = sptr[k];
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row: 0 untested, 1 tested, KW_REDO
      int s_flag = 0;
      double s_S = 0.0;
      long long s_tie = 0;
      int s_N = 0;
      float s_delta = 0.f;
      for (int ri = 0; ri < rows_here; ++ri) {
        const int64_t row = row0 + ri;
        const float* prow = ps + row * s;
        SD_WAVE_SYNC();          // the previous row's readers are done with the wave's LDS
        // ---- stage the selected columns as keys (0xFFFF = NaN) and check that every value IS its key's float
        bool ok = true;
        for (int j = lane; j < nsel; j += 64) {
            const float v = __builtin_nontemporal_load(prow + cols[j]);
            const PsKey pk = key_of_ps(v);
            ok = ok && (v != v || pk.exact());
            keys[j] = (v != v) ? (unsigned short)0xFFFF : (unsigned short)pk.key();
        }
        if (__ballot(!ok) != 0ull) {
            if (lane == ri) s_flag = KW_REDO;
            continue;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            reinterpret_cast<uint4*>(Htot)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
            reinterpret_cast<uint4*>(Hset)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
        }
        SD_WAVE_SYNC();
        // ---- first walk over the sets
        int my_nv = 0;
        float my_med = 0.f, my_mean = 0.f;
        bool all3 = true;
        for (int i = 0; i < k; ++i) {
            const int a = sptr[i], cnt = sptr[i + 1] - a;
            unsigned short* K = keys + a;
            // ordered compaction in place (a key moves to a slot at or below its own; every lane reads its key of the
            // round before any lane writes) + the set's histogram
            int nv = 0;
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                const int j = c0 + lane;
                const unsigned key = j < cnt ? (unsigned)K[j] : 0xFFFFu;
                const bool valid = key != 0xFFFFu;
                const unsigned long long m = __ballot(valid);
                SD_WAVE_SYNC();
                if (valid) {
                    K[lanes_below(m, nv)] = (unsigned short)key;
                    atomicAdd(&Hset[key], 1u);
                }
                nv += __popcll(m);
            }
            SD_WAVE_SYNC();
            if (nv < 3) { all3 = false; break; }        // wave-uniform
            const float sum = kw_wave_sum_keys(K, nv, lane, leaf_off, leaf_sum);
            // scan of the set's histogram, lane owns bins [16 lane, 16 lane + 16); the set joins the total, its bins are cleared
            unsigned w[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 t4 = reinterpret_cast<const uint4*>(Hset)[lane * 4 + q];
                w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w;
            }
            int tot = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) tot += (int)w[q];
            int pre = tot;
#pragma unroll
            for (int ofs = 1; ofs < 64; ofs <<= 1) {
                const int up = __shfl_up(pre, ofs);
                if (lane >= ofs) pre += up;
            }
            const int cum0 = pre - tot;
            // the median: the bins where the cumulative count crosses the middle positions
            const int hh = nv >> 1;
            const int bin1 = find_bin<0, ~0u>(Hset, lane, hh, cum0, tot);
            const int bin0 = (nv & 1) ? bin1 : find_bin<0, ~0u>(Hset, lane, hh - 1, cum0, tot);      // wave-uniform branch
            const float v0 = ps_of_key((float)bin0), v1 = ps_of_key((float)bin1);
            const float med = (nv & 1) ? v1 : (v0 + v1) / 2.0f;       // np.median on float32
            SD_WAVE_SYNC();          // find_bin's readers are done with Hset
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint4 t4 = reinterpret_cast<const uint4*>(Htot)[lane * 4 + q];
                t4.x += w[4 * q]; t4.y += w[4 * q + 1]; t4.z += w[4 * q + 2]; t4.w += w[4 * q + 3];
                reinterpret_cast<uint4*>(Htot)[lane * 4 + q] = t4;
                reinterpret_cast<uint4*>(Hset)[lane * 4 + q] = make_uint4(0, 0, 0, 0);
            }
            SD_WAVE_SYNC();
            if (lane == i) { my_nv = nv; my_med = med; my_mean = sum / (float)nv; }
        }
        if (!all3) {
            if (lane < k) {
                o.med[(int64_t)lane * n + row] = 0.f;
                o.mean[(int64_t)lane * n + row] = 0.f;
            }
            continue;
        }
        // ---- total histogram -> r2 per bin, N, sum(t^3 - t)
        int N;
        long long tie = 0;
        {
            unsigned w[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 t4 = reinterpret_cast<const uint4*>(Htot)[lane * 4 + q];
                w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w;
            }
            int tot = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) tot += (int)w[q];
            int pre = tot;
#pragma unroll
            for (int ofs = 1; ofs < 64; ofs <<= 1) {
                const int up = __shfl_up(pre, ofs);
                if (lane >= ofs) pre += up;
            }
            N = __shfl(pre, 63);
            int cum = pre - tot;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const long long t = (long long)w[q];
                tie += t * t * t - t;
                const unsigned r2 = 2u * (unsigned)cum + w[q] + 1u;
                cum += (int)w[q];
                w[q] = r2;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                reinterpret_cast<uint4*>(Htot)[lane * 4 + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) tie += __shfl_xor(tie, ofs);
        }
        SD_WAVE_SYNC();
        // ---- second walk: sum of r2 per set (at most N (N + 1) < 2^32 in all)
        unsigned my_r2 = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned short* K = keys + sptr[i];
            const int nv = __shfl(my_nv, i);
            unsigned local = 0;
            for (int j = lane; j < nv; j += 64) local += Htot[K[j]];
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) local += __shfl_xor(local, ofs);
            if (lane == i) my_r2 = local;
        }
        // ---- S over the sets, delta, the per-set outputs
        double term = 0.0;
        if (lane < k) {
            const long long D = (long long)my_r2 - (long long)my_nv * (long long)(N + 1);
            term = (double)(D * D) / (double)my_nv;
        }
        const double S = kw_sorted_sum(term, lane);
        const float inf = __builtin_inff();
        const float dl = kw_wave_max(lane < k ? my_med : -inf) - kw_wave_min(lane < k ? my_med : inf);
        if (lane < k) {
            o.med[(int64_t)lane * n + row] = my_med;
            o.mean[(int64_t)lane * n + row] = my_mean;
        }
        if (lane == ri) { s_flag = 1; s_S = S; s_tie = tie; s_N = N; s_delta = dl; }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        if (s_flag == KW_REDO) {
            o.tested[row] = KW_REDO;
        } else {
            double H = 0.0, p = 0.0;
            if (s_flag) kw_finish(s_S, (long long)s_N, s_tie, k, H, p);
            o.tested[row] = (uint8_t)s_flag;
            o.p[row] = p;
            if (o.h) o.h[row] = H;
            o.delta[row] = s_delta;
        }
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
__global__ void __launch_bounds__(RB_THREADS) kruskal_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                   const int32_t* __restrict__ cols, KwSets sets, int k, int P,
                                                                   int redo_only, KwOut o) {
    extern __shared__ __align__(16) unsigned char smemb[];
    unsigned long long* K = reinterpret_cast<unsigned long long*>(smemb);       // [P]; first the compaction buffer of the means
    float* F = reinterpret_cast<float*>(smemb);
    __shared__ float leaf_sum[KW_LEAF_MAX];
    __shared__ float scratch8[KW_LEAF_MAX * 8];
    __shared__ int leaf_off[KW_LEAF_MAX + 1];
    __shared__ int wcnt[RB_THREADS / 64 + 1];
    __shared__ int sptr[KW_MAX_SETS + 1];
    __shared__ int nvs[KW_MAX_SETS];
    __shared__ int starts[KW_MAX_SETS + 1];
    __shared__ float meanS[KW_MAX_SETS], medS[KW_MAX_SETS];
    __shared__ unsigned long long r2S[KW_MAX_SETS];
    __shared__ unsigned long long tieS;
    __shared__ unsigned char flags[RB_THREADS];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i <= k; i += RB_THREADS) sptr[i] = sets.ptr[i];
    __syncthreads();
    const int nsel = sptr[k];
    const int64_t n_chunks = (n + RB_THREADS - 1) / RB_THREADS;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
      {
        const int64_t row = c * RB_THREADS + tid;
        flags[tid] = (row < n && (!redo_only || o.tested[row] == KW_REDO)) ? 1 : 0;
      }
      __syncthreads();
      for (int ri = 0; ri < RB_THREADS; ++ri) {
        if (!flags[ri]) continue;                    // block-uniform
        const int64_t row = c * RB_THREADS + ri;
        const float* prow = ps + row * s;
        // ---- per set: ordered compaction + numpy pairwise sum (the key area is the float buffer)
        bool all3 = true;
        for (int i = 0; i < k; ++i) {
            const int a = sptr[i];
            const int nv = block_compact(prow, cols + a, sptr[i + 1] - a, F, wcnt);
            if (nv < 3) { all3 = false; break; }     // block-uniform
            // np.sum: 0 + the tree of the first KW_SUM_PIECE values (+ the tree of the rest), see kw_wave_sum_keys; the
            // leading 0 makes a sum of -0.0 values +0.0 as numpy's is
            float sum = 0.0f + block_pairwise_sum<KW_PW_DEPTH>(F, min(nv, KW_SUM_PIECE), leaf_off, leaf_sum, scratch8, KW_LEAF_MAX);
            if (nv > KW_SUM_PIECE)                   // block-uniform
                sum += block_pairwise_sum<KW_PW_DEPTH>(F + KW_SUM_PIECE, nv - KW_SUM_PIECE, leaf_off, leaf_sum, scratch8, KW_LEAF_MAX);
            if (tid == 0) { nvs[i] = nv; meanS[i] = sum / (float)nv; }
        }
        if (!all3) {
            if (tid < k) {
                o.med[(int64_t)tid * n + row] = 0.f;
                o.mean[(int64_t)tid * n + row] = 0.f;
            }
            if (tid == 0) {
                o.tested[row] = 0; o.p[row] = 0.0;
                if (o.h) o.h[row] = 0.0;
                o.delta[row] = 0.f;
            }
            __syncthreads();
            continue;
        }
        // ---- keys (set, value), NaNs and padding last; sort; medians
        for (int j = tid; j < P; j += RB_THREADS) {
            unsigned long long key = ~0ull;
            if (j < nsel) {
                const float v = prow[cols[j]];
                if (v == v) {
                    int lo = 0, hi = k;              // the set of selection j: last i with sptr[i] <= j
                    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (sptr[m] <= j) lo = m; else hi = m; }
                    key = ((unsigned long long)lo << 32) | f32_ord(v);
                }
            }
            K[j] = key;
        }
        if (tid == 0) {
            int acc = 0;
            for (int i = 0; i < k; ++i) { starts[i] = acc; acc += nvs[i]; }
            starts[k] = acc;
            tieS = 0ull;
        }
        if (tid < k) r2S[tid] = 0ull;
        __syncthreads();
        const auto by_key = [K](int i, int l, int desc) {
            const bool asc = desc == 0;
            const unsigned long long x = K[i], y = K[l];
            if ((x > y) == asc) { K[i] = y; K[l] = x; }
        };
        block_bitonic(P, by_key);
        const int N = starts[k];
        if (tid < k) {
            const int nv = nvs[tid];
            medS[tid] = median_of_ord(K + starts[tid], nv);        // np.median on float32
        }
        __syncthreads();
        // ---- keys (value, set); sort; ranks
        for (int q = tid; q < N; q += RB_THREADS) {
            const unsigned long long key = K[q];
            K[q] = (key << 32) | (key >> 32);
        }
        __syncthreads();
        block_bitonic(P, by_key);
        long long tie = 0;
        for (int q = tid; q < N; q += RB_THREADS) {
            const unsigned long long key = K[q];
            const uint32_t vb = (uint32_t)(key >> 32);
            // (written out: through run_bounds of rowsum.h the two selects of a search step change places and the rank
            // loses its zero extension, and no timing tool runs this kernel's rank loop: their tables are 3-decimal)
            int lo = 0, hi = N;                      // first position with value >= vb
            while (lo < hi) { const int m = (lo + hi) >> 1; if ((uint32_t)(K[m] >> 32) < vb) lo = m + 1; else hi = m; }
            const int first = lo;
            hi = N;                                  // first position with value > vb
            while (lo < hi) { const int m = (lo + hi) >> 1; if ((uint32_t)(K[m] >> 32) <= vb) lo = m + 1; else hi = m; }
            atomicAdd(&r2S[(int)(key & 0xffu)], (unsigned long long)(first + lo + 1));
            if (q == first) {
                const long long t = lo - first;
                tie += t * t * t - t;
            }
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) tie += __shfl_xor(tie, ofs);
        if (lane == 0 && tie) atomicAdd(&tieS, (unsigned long long)tie);
        __syncthreads();
        if (tid < 64) {                              // the first wave
            double term = 0.0;
            float my_med = 0.f;
            if (tid < k) {
                const long long D = (long long)r2S[tid] - (long long)nvs[tid] * (long long)(N + 1);
                term = (double)(D * D) / (double)nvs[tid];
                my_med = medS[tid];
                o.med[(int64_t)tid * n + row] = my_med;
                o.mean[(int64_t)tid * n + row] = meanS[tid];
            }
            const double S = kw_sorted_sum(term, lane);
            const float inf = __builtin_inff();
            const float dl = kw_wave_max(tid < k ? my_med : -inf) - kw_wave_min(tid < k ? my_med : inf);
            if (tid == 0) {
                double H, p;
                kw_finish(S, (long long)N, (long long)tieS, k, H, p);
                o.tested[row] = 1; o.p[row] = p;
                if (o.h) o.h[row] = H;
                o.delta[row] = dl;
            }
        }
        __syncthreads();
      }
      __syncthreads();           // every thread has read the chunk's flags
    }
}

// the checks both entry points share; set_ptr is a HOST array
int kw_check_sets(const int32_t* set_ptr, int32_t k, int32_t s) {
    SD_ARG(set_ptr, "set_ptr is NULL");
    SD_ARG(k >= 2 && k <= KW_MAX_SETS, "the number of sets must be 2..64");
    SD_ARG(set_ptr[0] == 0, "set_ptr[0] must be 0");
    for (int i = 0; i < k; ++i) SD_ARG(set_ptr[i + 1] > set_ptr[i], "empty set (set_ptr must increase)");
    if (set_ptr[k] > KW_MAX_N) {
        sdice_set_error("sdice_kruskal: %d selected columns, at most %d are supported", (int)set_ptr[k], KW_MAX_N);
        return SDICE_ERR_ARG;
    }
    SD_ARG(set_ptr[k] <= s, "more selected columns than the table has (a column belongs to one set only)");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_kruskal_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                                 const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_h,
                                 float* d_med, float* d_mean, float* d_delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets(set_ptr, k, s));
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med && d_mean && d_delta, "NULL output");
    SD_ARG(d_ps && d_cols, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    KwSets sets;
    int maxset = 0;
    for (int i = 0; i <= KW_MAX_SETS; ++i) sets.ptr[i] = i <= k ? set_ptr[i] : set_ptr[k];
    for (int i = 0; i < k; ++i) maxset = std::max(maxset, (int)(set_ptr[i + 1] - set_ptr[i]));
    const int nsel = set_ptr[k];
    KwOut o{d_tested, d_p, d_h, d_med, d_mean, d_delta};
    {   // grid path.  Leaves of the pairwise recursion over a piece of at most KW_SUM_PIECE values: after d halvings a
        // part is at most piece / 2^d + 15 long, a leaf from 128 down
        const int piece = std::min(maxset, KW_SUM_PIECE);
        int leaf_cap = 1;
        while (leaf_cap < KW_LEAF_MAX && piece > 113 * leaf_cap) leaf_cap <<= 1;
        const int wstride = (int)((2 * KW_BINS * 4 + (2 * leaf_cap + 1) * 4 + 2 * nsel + 15) & ~15);
        int waves = 64 * 1024 / wstride;             // the workgroup is sized from the LDS a wave needs
        waves = waves > 4 ? 4 : (waves < 1 ? 1 : waves);
        const size_t lds = (size_t)waves * wstride;
        const int ch = rows_per_chunk(ctx->n_cu, n);
        const int64_t blocks = wave_launch_blocks(ctx, n, ch, waves);
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kruskal_grid_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        SD_LAUNCH(ctx, "kruskal_grid_kernel", kruskal_grid_kernel, dim3((unsigned)blocks), dim3(waves * 64), lds, d_ps, n,
                  (int)s, d_cols, sets, (int)k, ch, wstride, leaf_cap, o);
    }
    {   // the rows it marked KW_REDO
        const int P = next_pow2(nsel, 2);
        const size_t lds = (size_t)P * 8;
        const int64_t blocks = row_launch_blocks(ctx, sd_ceil_div(n, RB_THREADS));
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kruskal_block_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        SD_LAUNCH(ctx, "kruskal_block_kernel", kruskal_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n,
                  (int)s, d_cols, sets, (int)k, P, 1, o);
    }
    return SDICE_OK;
}

extern "C" int sdice_kruskal(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                             const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* h, float* med,
                             float* mean, float* delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets(set_ptr, k, s));
    SD_ARG(cols, "cols is NULL");
    const int nsel = set_ptr[k];
    SD_TRY(check_columns(__func__, {cols}, nsel, s, "column index out of range", "a column may belong to one set only"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med && mean && delta, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float *d_ps, *df;
    int32_t* dcols;
    uint8_t* dt;
    double* dd;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dcols, cols, nsel));
    SD_TRY(st.alloc(&dt, n));
    SD_TRY(st.alloc(&dd, n * 2));                    // p, h
    SD_TRY(st.alloc(&df, n * (2 * (int64_t)k + 1))); // med[k][n], mean[k][n], delta
    SD_TRY(sdice_kruskal_dev(ctx, n, s, d_ps, dcols, set_ptr, k, dt, dd, dd + n, df, df + (int64_t)k * n,
                             df + 2 * (int64_t)k * n));
    SD_TRY(st.download(tested, dt, n));
    SD_TRY(st.download(p, dd, n));
    if (h) SD_TRY(st.download(h, dd + n, n));
    SD_TRY(st.download(med, df, (int64_t)k * n));
    SD_TRY(st.download(mean, df + (int64_t)k * n, (int64_t)k * n));
    return st.download(delta, df + 2 * (int64_t)k * n, n);
}
