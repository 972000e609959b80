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
// Dunn's test (sdice_kruskal_dunn): both kernels carry a pair epilogue behind `template <bool DUNN>`; the DUNN = false
// instantiations are sdice_kruskal's kernels as they were.  For every pair of sets i < j, in the order (0,1), (0,2), ..,
// (k-2,k-1), pair index q of m = k (k - 1) / 2, from the row's integers alone (den = N^3 - N - sum(t^3 - t)):
//   num = D_i n_j - D_j n_i                      (64-bit integer, |num| <= N^3 / 2 < 2^41: exact as a float64)
//   z^2 = 3 (N - 1) num^2 / (n_i n_j (n_i + n_j) den)        (R_i-bar - R_j-bar over its standard error, no continuity term)
//   z   = num / sqrt(den * (n_i n_j (n_i + n_j)) / (3 (N - 1)))
// The exact floating-point form: den < 2^42, n_i n_j (n_i + n_j) < 2^41 and 3 (N - 1) are exact float64; their product is
// an exact double-double (one fma), the quotient, the root and num / root run in double-double arithmetic (dd.h, each
// good to about 2^-100) and z = hi + lo is the ONE rounding of the chain: rounding count 1, so z is within 1 ulp of the
// correctly rounded value (equal to it but for a value within 2^-100 of a rounding boundary).  num == 0 gives z = +0.0 by
// a test on the integer.  z > 0: set i ranks above set j.  Swapping or renumbering sets negates num and nothing else, so
// z negates bit for bit.
//   p    = erfc(|z| / sqrt 2): the library erfc of the rounded z, |z| * 0.7071.. rounded once before it
//   padj = Holm's step-down inside the row: rank_q = #{t: p_t < p_q or (p_t == p_q and t < q)},
//          padj_q = min(1, max over the pairs t with rank_t <= rank_q of (m - rank_t) p_t); (m - rank) p is one float64
//          product, max and min are exact.  Equal p's get equal padj: of two equal p's the later rank has the smaller factor.
// A row with den == 0 (every kept value equal): z = 0, p = 1, padj = 1 for every pair; an untested row: 0 in every slot.
// One pair per lane of one wave (dunn_pairs): lane q fetches (D_i, n_i, D_j, n_j) from the lanes (grid kernel) or the LDS
// slots (block kernel) of its two sets; the ranks by counting over m rounds of __shfl, then (m - rank) p goes to the lane of
// its rank (ds_permute), a max scan runs up the lanes and every lane reads back its rank's -- no atomics, nothing depends
// on an order of arrival.  m <= 64 lanes: k <= SDICE_DUNN_MAX_SETS = 11 (55 pairs) for this entry point.
//
// rowsum.h: the compaction, the pairwise sums, find_bin, the order bits of a float, np.median of sorted order bits, the
// block's bitonic network, the launch sizes and the column check; and, shared with jonckheere.hip (K18), the limits, the
// staging and first walk of the grid kernel (kw_stage_row, kw_walk_set), the block kernel up to its medians
// (kw_block_sort_sets), the checks of the sets and the launch plan (kw_check_sets, kw_plan).
#include "common.h"
#include <math.h>
#include <algorithm>
#include "rowsum.h"
#include "dd.h"

namespace {

struct KwOut {
    uint8_t* tested;
    double* p;
    double* h;       // may be NULL
    float* med;      // [k][n]
    float* mean;     // [k][n]
    float* delta;
};

// sdice_kruskal_dunn: KwOut and the pair outputs, pair-major [m][n]; pair_p and pair_padj may be NULL
struct DunnOut : KwOut {
    double* pair_z;
    double* pair_p;
    double* pair_padj;
};
template <bool DUNN> using KwOutOf = std::conditional_t<DUNN, DunnOut, KwOut>;
constexpr int DUNN_MAX_SETS = SDICE_DUNN_MAX_SETS;
static_assert(DUNN_MAX_SETS * (DUNN_MAX_SETS - 1) / 2 <= 64, "one pair per lane of a wave");

// the sets (i, j), i < j, of pair q in the order (0,1), (0,2), .., (k-2,k-1); (0, 0) from q = k (k - 1) / 2 on
__device__ __forceinline__ int2 dunn_pair_of(int q, int k) {
    int i = 0;
    while (i < k - 1 && q >= k - 1 - i) { q -= k - 1 - i; ++i; }
    return i < k - 1 ? make_int2(i, i + 1 + q) : make_int2(0, 0);
}

// 0 in every pair slot of a row that is not tested; called by the lanes of one wave
__device__ __forceinline__ void dunn_zero(const DunnOut& o, int lane, int m, int64_t n, int64_t row) {
    if (lane < m) {
        o.pair_z[(int64_t)lane * n + row] = 0.0;
        if (o.pair_p) o.pair_p[(int64_t)lane * n + row] = 0.0;
        if (o.pair_padj) o.pair_padj[(int64_t)lane * n + row] = 0.0;
    }
}

// The pair epilogue of a tested row, one pair per lane of ONE whole wave (file comment): pr = dunn_pair_of(lane, k);
// fetch(i, D, nv) hands every lane D_i and n_i of the set i it names (all 64 lanes call it together).
template <class Fetch>
__device__ __forceinline__ void dunn_pairs(const DunnOut& o, int lane, int m, int2 pr, long long N, long long den, int64_t n,
                                           int64_t row, Fetch fetch) {
    long long Di, Dj;
    int ni, nj;
    fetch(pr.x, Di, ni);
    fetch(pr.y, Dj, nj);
    double z = 0.0, p = 1.0;
    const long long num = Di * nj - Dj * ni;
    if (den != 0 && num != 0) {                      // (den: wave-uniform)
        const double a = (double)den, b = (double)((long long)ni * nj * (ni + nj));
        const double ab = a * b;
        const DD v = dd_div_d(dd_fast2sum(ab, __builtin_fma(a, b, -ab)), (double)(3 * (N - 1)));
        const DD zz = dd_div({(double)num, 0.0}, dd_sqrt(v));
        z = zz.hi + zz.lo;
        if (o.pair_p || o.pair_padj) p = erfc(fabs(z) * 0.70710678118654752440);       // (uniform)
    }
    const bool mine = lane < m;
    if (mine) {
        o.pair_z[(int64_t)lane * n + row] = z;
        if (o.pair_p) o.pair_p[(int64_t)lane * n + row] = p;
    }
    if (!o.pair_padj) return;                        // (uniform)
    int rank = 0;
    for (int t = 0; t < m; ++t) {
        const double pt = __shfl(p, t);
        rank += (pt < p || (pt == p && t < lane)) ? 1 : 0;
    }
    // the ranks of the m pairs are a permutation of 0..m-1; with rank = lane on the idle lanes, of 0..63: every lane
    // sends (m - rank) p to the lane of its rank, an inclusive max scan runs up the lanes, every lane reads its rank's
    if (!mine) rank = lane;
    const double mine_v = mine ? (double)(m - rank) * p : 0.0;
    const long long bits = __double_as_longlong(mine_v);
    const int lo = __builtin_amdgcn_ds_permute(rank << 2, (int)bits);
    const int hi = __builtin_amdgcn_ds_permute(rank << 2, (int)(bits >> 32));
    double run = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) {
        const double up = __shfl_up(run, ofs);
        if (lane >= ofs) run = fmax(run, up);
    }
    const double best = __shfl(run, rank);
    if (mine) o.pair_padj[(int64_t)lane * n + row] = fmin(1.0, best);
}

// H and p (kw_chi2_sf: rowsum.h, shared with friedman.hip) of a tested row from the integer pieces
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

// ------------------------------------------------------------------ grid path: one wave per row
// LDS per wave (wstride bytes): Htot[1024] | Hset[1024] | leaf_sum[leaf_cap] | leaf_off[leaf_cap + 1] | keys[nsel] u16
// (DUNN: 3 waves per SIMD asked for -- with the epilogue the kernel came out at 178 VGPRs and 2 waves, which cost more than
// the epilogue's instructions; it now takes 168 and 20 bytes of scratch per lane.  The bound leaves DUNN = false as it was.)
template <bool DUNN>
__global__ void __launch_bounds__(256, DUNN ? 3 : 1) kruskal_grid_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                           const int32_t* __restrict__ cols, KwSets sets, int k, int ch,
                                                           int wstride, int leaf_cap, KwOutOf<DUNN> o) {
    extern __shared__ __align__(16) unsigned char smemk[];
    __shared__ int sptr[KW_MAX_SETS + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = blockDim.x >> 6;
    const KwWaveLds L(smemk + (size_t)wave * wstride, leaf_cap);
    unsigned* const Htot = L.Htot;
    unsigned short* const keys = L.keys;
    for (int i = threadIdx.x; i <= k; i += blockDim.x) sptr[i] = sets.ptr[i];
    __syncthreads();
    const int nsel = sptr[k];
    const int64_t n_chunks = (n + ch - 1) / ch;
    [[maybe_unused]] const int m = k * (k - 1) / 2;
    [[maybe_unused]] int2 pr = make_int2(0, 0);
    if constexpr (DUNN) pr = dunn_pair_of(lane, k);
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
        if (!kw_stage_row(prow, cols, nsel, L, lane)) {
            if (lane == ri) s_flag = KW_REDO;
            continue;
        }
        // ---- first walk over the sets
        int my_nv = 0;
        float my_med = 0.f, my_mean = 0.f;
        bool all3 = true;
        for (int i = 0; i < k; ++i) {
            const int a = sptr[i];
            float med, mean;
            const int nv = kw_walk_set(keys + a, sptr[i + 1] - a, L, lane, med, mean, [](const unsigned (&)[16], const unsigned (&)[16]) {});
            if (nv < 3) { all3 = false; break; }        // wave-uniform
            if (lane == i) { my_nv = nv; my_med = med; my_mean = mean; }
        }
        if (!all3) {
            if (lane < k) {
                o.med[(int64_t)lane * n + row] = 0.f;
                o.mean[(int64_t)lane * n + row] = 0.f;
            }
            if constexpr (DUNN) dunn_zero(o, lane, m, n, row);
            continue;
        }
        // ---- total histogram -> r2 per bin, N, sum(t^3 - t)
        int N;
        long long tie = 0;
        {
            unsigned w[16];
            kw_load_bins(Htot, lane, w);
            int tot;
            const int pre = kw_scan_bins(w, lane, tot);
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
        if constexpr (DUNN) {
            const long long NN = N;
            const long long myD = (long long)my_r2 - (long long)my_nv * (NN + 1);
            dunn_pairs(o, lane, m, pr, NN, NN * NN * NN - NN - tie, n, row, [myD, my_nv](int i, long long& D, int& nv) {
                D = __shfl(myD, i);
                nv = __shfl(my_nv, i);
            });
        }
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
template <bool DUNN>
__global__ void __launch_bounds__(RB_THREADS) kruskal_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                   const int32_t* __restrict__ cols, KwSets sets, int k, int P,
                                                                   int redo_only, KwOutOf<DUNN> o) {
    extern __shared__ __align__(16) unsigned char smemb[];
    unsigned long long* K = reinterpret_cast<unsigned long long*>(smemb);       // [P]; first the compaction buffer of the means
    __shared__ KwBlockLds sh;
    __shared__ unsigned long long r2S[KW_MAX_SETS];
    __shared__ unsigned long long tieS;
    __shared__ unsigned char flags[RB_THREADS];
    const int tid = threadIdx.x, lane = tid & 63;
    [[maybe_unused]] const int m = k * (k - 1) / 2;
    [[maybe_unused]] int2 pr = make_int2(0, 0);
    if constexpr (DUNN) pr = dunn_pair_of(lane, k);
    for (int i = tid; i <= k; i += RB_THREADS) sh.sptr[i] = sets.ptr[i];
    __syncthreads();
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
        // ---- means, the (set, value) sort, medians
        const bool all3 = kw_block_sort_sets(prow, cols, k, P, K, sh);
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
            if constexpr (DUNN)
                if (tid < 64) dunn_zero(o, tid, m, n, row);
            __syncthreads();
            continue;
        }
        const auto by_key = [K](int i, int l, int desc) {
            const bool asc = desc == 0;
            const unsigned long long x = K[i], y = K[l];
            if ((x > y) == asc) { K[i] = y; K[l] = x; }
        };
        const int N = sh.starts[k];
        if (tid == 0) tieS = 0ull;
        if (tid < k) r2S[tid] = 0ull;
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
                const long long D = (long long)r2S[tid] - (long long)sh.nvs[tid] * (long long)(N + 1);
                term = (double)(D * D) / (double)sh.nvs[tid];
                my_med = sh.medS[tid];
                o.med[(int64_t)tid * n + row] = my_med;
                o.mean[(int64_t)tid * n + row] = sh.meanS[tid];
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
            if constexpr (DUNN) {
                const long long NN = N;
                dunn_pairs(o, lane, m, pr, NN, NN * NN * NN - NN - (long long)tieS, n, row, [&](int i, long long& D, int& nv) {
                    nv = sh.nvs[i];
                    D = (long long)r2S[i] - (long long)nv * (NN + 1);
                });
            }
        }
        __syncthreads();
      }
      __syncthreads();           // every thread has read the chunk's flags
    }
}

}  // namespace

extern "C" int sdice_kruskal_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                                 const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_h,
                                 float* d_med, float* d_mean, float* d_delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_kruskal", set_ptr, k, s));
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med && d_mean && d_delta, "NULL output");
    SD_ARG(d_ps && d_cols, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const KwPlan pl = kw_plan(set_ptr, k);
    KwOut o{d_tested, d_p, d_h, d_med, d_mean, d_delta};
    return kw_launch_pair<kruskal_grid_kernel<false>, kruskal_block_kernel<false>>(ctx, "kruskal_grid_kernel", "kruskal_block_kernel",
                                                                                   pl, d_ps, n, s, d_cols, k, o);
}

extern "C" int sdice_kruskal(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                             const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* h, float* med,
                             float* mean, float* delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_kruskal", set_ptr, k, s));
    SD_ARG(cols, "cols is NULL");
    const int nsel = set_ptr[k];
    SD_TRY(check_columns(__func__, {cols}, nsel, s, "column index out of range", "a column may belong to one set only"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med && mean && delta, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t* dcols;
    KwOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dcols, cols, nsel));
    st.result(&d.tested, tested, n);
    st.result(&d.p, p, n);
    st.result(&d.h, h, n);
    st.result(&d.med, med, (int64_t)k * n);          // [k][n]
    st.result(&d.mean, mean, (int64_t)k * n);
    st.result(&d.delta, delta, n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_kruskal_dev(ctx, n, s, d_ps, dcols, set_ptr, k, d.tested, d.p, d.h, d.med, d.mean, d.delta));
    return st.download_results();
}

extern "C" int sdice_kruskal_dunn_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                                      const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_h,
                                      float* d_med, float* d_mean, float* d_delta, double* d_pair_z, double* d_pair_p,
                                      double* d_pair_padj) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_kruskal_dunn", set_ptr, k, s));
    SD_ARG(k <= DUNN_MAX_SETS, "the number of sets must be 2..11 (one pair of sets per lane of a wave)");
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med && d_mean && d_delta && d_pair_z, "NULL output");
    SD_ARG(d_ps && d_cols, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const KwPlan pl = kw_plan(set_ptr, k);
    DunnOut o{{d_tested, d_p, d_h, d_med, d_mean, d_delta}, d_pair_z, d_pair_p, d_pair_padj};
    return kw_launch_pair<kruskal_grid_kernel<true>, kruskal_block_kernel<true>>(ctx, "kruskal_dunn_grid_kernel",
                                                                                 "kruskal_dunn_block_kernel", pl, d_ps, n, s, d_cols, k, o);
}

extern "C" int sdice_kruskal_dunn(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                                  const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* h, float* med,
                                  float* mean, float* delta, double* pair_z, double* pair_p, double* pair_padj) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_kruskal_dunn", set_ptr, k, s));
    SD_ARG(k <= DUNN_MAX_SETS, "the number of sets must be 2..11 (one pair of sets per lane of a wave)");
    SD_ARG(cols, "cols is NULL");
    const int nsel = set_ptr[k];
    SD_TRY(check_columns(__func__, {cols}, nsel, s, "column index out of range", "a column may belong to one set only"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med && mean && delta && pair_z, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t* dcols;
    DunnOut d;
    const int64_t m = (int64_t)k * (k - 1) / 2;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dcols, cols, nsel));
    st.result(&d.tested, tested, n);
    st.result(&d.p, p, n);
    st.result(&d.h, h, n);
    st.result(&d.med, med, (int64_t)k * n);          // [k][n]
    st.result(&d.mean, mean, (int64_t)k * n);
    st.result(&d.delta, delta, n);
    st.result(&d.pair_z, pair_z, m * n);             // [m][n]
    st.result(&d.pair_p, pair_p, m * n);
    st.result(&d.pair_padj, pair_padj, m * n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_kruskal_dunn_dev(ctx, n, s, d_ps, dcols, set_ptr, k, d.tested, d.p, d.h, d.med, d.mean, d.delta, d.pair_z,
                                  d.pair_p, d.pair_padj));
    return st.download_results();
}
