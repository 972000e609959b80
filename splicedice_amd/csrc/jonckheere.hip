// K18: Jonckheere-Terpstra trend test per junction row across k >= 2 ORDERED sample sets + per-set median / mean.
//
// The row rules and the per-set outputs are kruskal.hip's (K12): per set the row's values at the set's columns with NaNs
// dropped, the row is tested when every set keeps >= 3 values; med / mean / delta are bit for bit those of sdice_kruskal.
// The sets are ordered as given, set 0 < set 1 < ... < set k-1.
//
// Arithmetic, in integers up to the last step (n_i kept values in set i, N their sum, t the sizes of the tie groups of
// the N values):
//   J2  = sum_{i<j} sum_{x in set i, y in set j} (2 [x < y] + [x == y])        (= 2 J)
//   M2  = sum_{i<j} n_i n_j = (N^2 - sum n_i^2) / 2                              (= 2 E[J])
//   A   = N(N-1)(2N+5) - sum n_i(n_i-1)(2n_i+5) - sum t(t-1)(2t+5)
//   B1  = sum n_i(n_i-1)(n_i-2), B2 = sum t(t-1)(t-2), C1 = sum n_i(n_i-1), C2 = sum t(t-1)
//   num = A N(N-1)(N-2) + 2 B1 B2 + 9 (N-2) C1 C2                                (128-bit: up to 4e25 at N = 16384)
//   Var(J) = num / (72 N(N-1)(N-2)),  z = (J2 - M2) / (2 sqrt Var) = (J2 - M2) / sqrt(num / (18 N(N-1)(N-2)))
//   p = erfc(|z| / sqrt 2), no continuity correction; z > 0: the values rise along the set order.
// The last step (num / (18 den), its root, the two quotients, erfc up to x^2 = 9) runs in double-double arithmetic (dd.h,
// erfc_dd.h), in which num is exact; nothing is divided in 128 bits.  num == 0 (every kept value equal) is decided on the
// integers: the row stays tested with z = 0, p = 1.
//
// Kernels:
//   jonckheere_grid_kernel: rows of 3-decimal PS values, one WAVE per row, nothing is sorted: the first walk of
//       kruskal_grid_kernel (rowsum.h: kw_walk_set); before set j's histogram joins the total of the sets before it the
//       total is scanned (lane owns 16 bins) and sum_v Hset[v] (2 cum_excl(Htot)[v] + Htot[v]) goes to J2.  After the last
//       set the total gives the tie sums.  Set i's count lives in lane i.  Any other row is marked KW_REDO and left to
//   jonckheere_block_kernel: any finite float32 values, one workgroup per row: means, the (set, value) sort and the
//       medians of kruskal_block_kernel (rowsum.h: kw_block_sort_sets); then every element binary-searches its value's
//       lower and upper bound in each set's sorted run: the bounds summed over the earlier sets are its share of J2,
//       upper - lower summed over all sets is its tie-group size t, and sum over groups of t g(t) = sum over elements of
//       g(t).  No second sort, no pair loop.
#include "common.h"
#include <math.h>
#include <algorithm>
#include "rowsum.h"
#include "dd.h"
#include "erfc_dd.h"

namespace {

struct JtOut {
    uint8_t* tested;
    double* p;
    double* z;
    double* j;       // may be NULL
    float* med;      // [k][n]
    float* mean;     // [k][n]
    float* delta;
};

// the integer pieces of a tested row (file comment); a holds the set and tie terms of A, the N term joins in jt_finish
struct JtSums {
    long long j2, m2, a, b1, b2, c1, c2;
    int N;
};

// the set terms of one set's count and the tie terms of one tie group's size: the same three polynomials
__device__ __forceinline__ void jt_terms(long long t, long long& a, long long& b, long long& c) {
    const long long tt = t * (t - 1);
    a += tt * (2 * t + 5);
    b += tt * (t - 2);
    c += tt;
}

__device__ __forceinline__ long long jt_wave_sum(long long v) {
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs);
    return v;
}

// z, p and J of a tested row
__device__ __forceinline__ void jt_finish(const JtSums& q, double& z, double& p, double& j) {
    const long long N = q.N;
    const long long den = N * (N - 1) * (N - 2);                     // N >= 6
    const long long A = N * (N - 1) * (2 * N + 5) - q.a;             // negative on heavily tied rows
    // num = A den + 2 B1 B2 + 9 (N - 2) C1 C2 >= 0 from unsigned 64 x 64 -> 128 products only (C1 C2 < 2^57); the signed
    // 128-bit product of a negative A came out of the device compiler as the unsigned one, 2^64 den too large
    typedef unsigned __int128 u128;
    const u128 bc = 2 * ((u128)(unsigned long long)q.b1 * (unsigned long long)q.b2) +
                    (u128)(unsigned long long)(9 * (N - 2)) * (unsigned long long)(q.c1 * q.c2);
    const u128 ad = (u128)(unsigned long long)(A < 0 ? -A : A) * (unsigned long long)den;
    const u128 num = A < 0 ? bc - ad : bc + ad;
    j = 0.5 * (double)q.j2;                                          // exact: J2 < 2^29
    if (num == 0) { z = 0.0; p = 1.0; return; }                      // every value equal
    // 4 Var = num / (18 den) in double-double arithmetic (num < 2^86 is exact there): z and erfc's argument keep about
    // 100 bits to their single last rounding, so the printed z is the correctly rounded quotient
    const DD v4 = dd_div_d(dd_u128(num), (double)(18 * den));
    const long long D = q.j2 - q.m2;
    const DD zz = dd_div({(double)D, 0.0}, dd_sqrt(v4));
    z = zz.hi + zz.lo;
    if (D == 0) { p = 1.0; return; }
    // p = erfc(|z| / sqrt 2) from x^2 = D^2 / (2 * 4 Var): erfc_dd.h where most rows are, the library erfc down the tail
    const DD x2 = dd_div(dd_mul({(double)D, 0.0}, {(double)D, 0.0}), dd_mul_d(v4, 2.0));
    p = x2.hi <= SR_DD_X2_MAX ? erfc_dd_x2(x2) : erfc(sqrt(x2.hi + x2.lo));
}

// ------------------------------------------------------------------ grid path: one wave per row
__global__ void __launch_bounds__(256) jonckheere_grid_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                              const int32_t* __restrict__ cols, KwSets sets, int k, int ch,
                                                              int wstride, int leaf_cap, JtOut o) {
    extern __shared__ __align__(16) unsigned char smemj[];
    __shared__ int sptr[KW_MAX_SETS + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = blockDim.x >> 6;
    const KwWaveLds L(smemj + (size_t)wave * wstride, leaf_cap);
    for (int i = threadIdx.x; i <= k; i += blockDim.x) sptr[i] = sets.ptr[i];
    __syncthreads();
    const int nsel = sptr[k];
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row: 0 untested, 1 tested, KW_REDO
      int s_flag = 0;
      JtSums s_q = {0, 0, 0, 0, 0, 0, 0, 0};
      float s_delta = 0.f;
      for (int ri = 0; ri < rows_here; ++ri) {
        const int64_t row = row0 + ri;
        const float* prow = ps + row * s;
        SD_WAVE_SYNC();          // the previous row's readers are done with the wave's LDS
        if (!kw_stage_row(prow, cols, nsel, L, lane)) {
            if (lane == ri) s_flag = KW_REDO;
            continue;
        }
        // ---- the walk over the sets in their order
        int my_nv = 0;
        float my_med = 0.f, my_mean = 0.f;
        unsigned j2 = 0;         // this lane's bins' share of J2 (J2 < N^2 < 2^32 in all)
        bool all3 = true;
        for (int i = 0; i < k; ++i) {
            const int a = sptr[i];
            float med, mean;
            const int nv = kw_walk_set(L.keys + a, sptr[i + 1] - a, L, lane, med, mean,
                                       [&j2, i, lane](const unsigned (&w)[16], const unsigned (&t)[16]) {
                if (i == 0) return;                      // wave-uniform: nothing before the first set
                int tot;
                unsigned cum = (unsigned)(kw_scan_bins(t, lane, tot) - tot);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    j2 += w[q] * (2u * cum + t[q]);
                    cum += t[q];
                }
            });
            if (nv < 3) { all3 = false; break; }        // wave-uniform
            if (lane == i) { my_nv = nv; my_med = med; my_mean = mean; }
        }
        if (!all3) {
            if (lane < k) {
                o.med[(int64_t)lane * n + row] = 0.f;
                o.mean[(int64_t)lane * n + row] = 0.f;
            }
            continue;
        }
        // ---- the tie sums from the total histogram, the set sums from the lanes' counts
        JtSums q = {0, 0, 0, 0, 0, 0, 0, 0};
        {
            unsigned w[16];
            kw_load_bins(L.Htot, lane, w);
            long long ta = 0, tb = 0, tc = 0;
#pragma unroll
            for (int b = 0; b < 16; ++b) jt_terms((long long)w[b], ta, tb, tc);
            long long na = 0;
            jt_terms((long long)my_nv, na, q.b1, q.c1);  // (a lane at or past k holds 0)
            q.a = jt_wave_sum(ta + na);
            q.b1 = jt_wave_sum(q.b1);
            q.c1 = jt_wave_sum(q.c1);
            q.b2 = jt_wave_sum(tb);
            q.c2 = jt_wave_sum(tc);
            const long long N = jt_wave_sum((long long)my_nv);
            q.N = (int)N;
            q.m2 = (N * N - jt_wave_sum((long long)my_nv * my_nv)) / 2;
            q.j2 = jt_wave_sum((long long)j2);
        }
        const float inf = __builtin_inff();
        const float dl = kw_wave_max(lane < k ? my_med : -inf) - kw_wave_min(lane < k ? my_med : inf);
        if (lane < k) {
            o.med[(int64_t)lane * n + row] = my_med;
            o.mean[(int64_t)lane * n + row] = my_mean;
        }
        if (lane == ri) { s_flag = 1; s_q = q; s_delta = dl; }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        if (s_flag == KW_REDO) {
            o.tested[row] = KW_REDO;
        } else {
            double z = 0.0, p = 0.0, j = 0.0;
            if (s_flag) jt_finish(s_q, z, p, j);
            o.tested[row] = (uint8_t)s_flag;
            o.p[row] = p;
            o.z[row] = z;
            if (o.j) o.j[row] = j;
            o.delta[row] = s_delta;
        }
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
__global__ void __launch_bounds__(RB_THREADS) jonckheere_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                      const int32_t* __restrict__ cols, KwSets sets, int k, int P,
                                                                      int redo_only, JtOut o) {
    extern __shared__ __align__(16) unsigned char smemjb[];
    unsigned long long* K = reinterpret_cast<unsigned long long*>(smemjb);      // [P]; first the compaction buffer of the means
    __shared__ KwBlockLds sh;
    __shared__ unsigned long long accS[4];           // J2 and the three tie sums
    __shared__ unsigned char flags[RB_THREADS];
    const int tid = threadIdx.x, lane = tid & 63;
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
        if (!kw_block_sort_sets(prow, cols, k, P, K, sh)) {
            if (tid < k) {
                o.med[(int64_t)tid * n + row] = 0.f;
                o.mean[(int64_t)tid * n + row] = 0.f;
            }
            if (tid == 0) {
                o.tested[row] = 0; o.p[row] = 0.0; o.z[row] = 0.0;
                if (o.j) o.j[row] = 0.0;
                o.delta[row] = 0.f;
            }
            __syncthreads();
            continue;
        }
        const int N = sh.starts[k];
        if (tid < 4) accS[tid] = 0ull;
        __syncthreads();
        // ---- every element against every set's sorted run
        long long j2 = 0, ta = 0, tb = 0, tc = 0;
        for (int q = tid; q < N; q += RB_THREADS) {
            const unsigned long long key = K[q];
            const uint32_t vb = (uint32_t)key;
            const int mine = (int)(key >> 32);
            int t = 0;
            for (int i = 0; i < k; ++i) {
                const unsigned long long* R = K + sh.starts[i];
                const int len = sh.starts[i + 1] - sh.starts[i];
                int lo = 0, hi = len;                // first position with a value >= vb
                while (lo < hi) { const int m = (lo + hi) >> 1; if ((uint32_t)R[m] < vb) lo = m + 1; else hi = m; }
                const int first = lo;
                hi = len;                            // first position with a value > vb
                while (lo < hi) { const int m = (lo + hi) >> 1; if ((uint32_t)R[m] <= vb) lo = m + 1; else hi = m; }
                if (i < mine) j2 += first + lo;
                t += lo - first;
            }
            // sum over the tie groups of t g(t) = sum over the elements of g(t)
            const long long t1 = t - 1;
            ta += t1 * (2 * t + 5);
            tb += t1 * (t - 2);
            tc += t1;
        }
        j2 = jt_wave_sum(j2); ta = jt_wave_sum(ta); tb = jt_wave_sum(tb); tc = jt_wave_sum(tc);
        if (lane == 0) {
            atomicAdd(&accS[0], (unsigned long long)j2);
            atomicAdd(&accS[1], (unsigned long long)ta);
            atomicAdd(&accS[2], (unsigned long long)tb);
            atomicAdd(&accS[3], (unsigned long long)tc);
        }
        __syncthreads();
        if (tid < 64) {                              // the first wave
            float my_med = 0.f;
            long long nv = 0;
            if (tid < k) {
                nv = sh.nvs[tid];
                my_med = sh.medS[tid];
                o.med[(int64_t)tid * n + row] = my_med;
                o.mean[(int64_t)tid * n + row] = sh.meanS[tid];
            }
            JtSums q = {0, 0, 0, 0, 0, 0, 0, 0};
            long long na = 0;
            jt_terms(nv, na, q.b1, q.c1);
            q.a = jt_wave_sum(na) + (long long)accS[1];
            q.b1 = jt_wave_sum(q.b1);
            q.c1 = jt_wave_sum(q.c1);
            q.b2 = (long long)accS[2];
            q.c2 = (long long)accS[3];
            q.N = N;
            q.m2 = ((long long)N * N - jt_wave_sum(nv * nv)) / 2;
            q.j2 = (long long)accS[0];
            const float inf = __builtin_inff();
            const float dl = kw_wave_max(tid < k ? my_med : -inf) - kw_wave_min(tid < k ? my_med : inf);
            if (tid == 0) {
                double z, p, j;
                jt_finish(q, z, p, j);
                o.tested[row] = 1; o.p[row] = p; o.z[row] = z;
                if (o.j) o.j[row] = j;
                o.delta[row] = dl;
            }
        }
        __syncthreads();
      }
      __syncthreads();           // every thread has read the chunk's flags
    }
}

}  // namespace

extern "C" int sdice_jonckheere_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                                    const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_z,
                                    double* d_j, float* d_med, float* d_mean, float* d_delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_jonckheere", set_ptr, k, s));
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_z && d_med && d_mean && d_delta, "NULL output");
    SD_ARG(d_ps && d_cols, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    const KwPlan pl = kw_plan(set_ptr, k);
    JtOut o{d_tested, d_p, d_z, d_j, d_med, d_mean, d_delta};
    return kw_launch_pair<jonckheere_grid_kernel, jonckheere_block_kernel>(ctx, "jonckheere_grid_kernel", "jonckheere_block_kernel",
                                                                           pl, d_ps, n, s, d_cols, k, o);
}

extern "C" int sdice_jonckheere(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                                const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* z, double* j,
                                float* med, float* mean, float* delta) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(kw_check_sets("sdice_jonckheere", set_ptr, k, s));
    SD_ARG(cols, "cols is NULL");
    const int nsel = set_ptr[k];
    SD_TRY(check_columns(__func__, {cols}, nsel, s, "column index out of range", "a column may belong to one set only"));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && z && med && mean && delta, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t* dcols;
    JtOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dcols, cols, nsel));
    st.result(&d.tested, tested, n);
    st.result(&d.p, p, n);
    st.result(&d.z, z, n);
    st.result(&d.j, j, n);
    st.result(&d.med, med, (int64_t)k * n);          // [k][n]
    st.result(&d.mean, mean, (int64_t)k * n);
    st.result(&d.delta, delta, n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_jonckheere_dev(ctx, n, s, d_ps, dcols, set_ptr, k, d.tested, d.p, d.z, d.j, d.med, d.mean, d.delta));
    return st.download_results();
}
