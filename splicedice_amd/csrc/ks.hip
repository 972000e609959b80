// K19: two-sample Kolmogorov-Smirnov test per junction row over two column groups + median / mean of each group.
//
// Per row: the row's values at the group-1 and at the group-2 columns with NaNs dropped, n1' and n2' kept, N = n1' + n2';
// the row is tested when n1' >= 3 and n2' >= 3.  With c1(v) = #{x in group 1 : x <= v} and c2(v) likewise (float32
// comparison, -0.0 == +0.0)
//   M    = max over the distinct kept values v of |c1(v) n2' - c2(v) n1'|          (integer, <= 2^24)
//   D    = M / (n1' n2')                                                           (one float64 division)
//   lam2 = M^2 / (n1' n2' N)                                                       (exact integers, one division)
//   p    = min(1, 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lam2))                        (Kolmogorov's limiting distribution)
// The two empirical distribution functions are compared at the END of a tie run only, so a run that holds values of both
// groups gives one deviation whatever order the sort left the group bit in.  No Stephens or continuity correction and no
// finite-n form: the p-value of a row too large for the exact form is the plain limit.
//
// The series.  For lam2 >= KS_SWITCH the alternating series as 2 exp(-2 lam2) (1 - exp(-6 lam2) + exp(-16 lam2) - ...):
// the leading factor carries the whole range down to the smallest float64 and the bracket is 1 minus at most eight small
// terms.  Below, Jacobi's dual  1 - sqrt(2 pi / lam2) sum_{k>=1} exp(-(2k - 1)^2 pi^2 / (8 lam2)),  three terms at most.
// At KS_SWITCH = 1/2 (p = 0.711) neither form cancels.  Both are summed in double-double arithmetic (dd.h) with an
// exponential written out in it: a relative error of about 2^-95 before the one rounding to float64 (a subnormal result
// is rounded once more by ldexp).  No proof of correct rounding, but the stored p equals the 50-digit referee's rounded
// value on every row of the test tables, which is what makes the command's table the referee's byte for byte.
//
// Exact p (want_exact, N <= 32): the conditional permutation probability given the row's ties.  With T the tie-run ends
// of the merged order as cumulative counts t,
//   inside = #{lattice paths (0,0) -> (n1', n2') : |i n2' - (t - i) n1'| < M at every t in T, i = group-1 values among the first t}
//   p      = (C(N, n1') - inside) / C(N, n1')
// by the recurrence cnt_t[i] = cnt_{t-1}[i] + cnt_{t-1}[i-1] with cnt[i] zeroed at a checkpoint t in T where the bound
// fails: lane i holds cnt[i] and, beside it, the same count without the bound (C(N, n1') at the end); both stay below
// C(32, 16) < 2^32.  What R >= 4.2 ks.test(exact = TRUE) computes with ties, scipy's ks_2samp(method="exact") without.
//
// Kernels:
//   ks_group_kernel<P>: n1 + n2 <= 64.  A group of P = next_pow2(n1 + n2) lanes owns a row, one selected column per lane
//       (group 1's first), 64 / P rows per wave side by side: the kept values compacted through the wave's LDS for the
//       numpy-order sums, the two median sorts, and one more sort of the key (value << 1 | group) -- 32 bits when every
//       row of the pass holds 3-decimal values, 64 bits with f32_ord otherwise (a ballot; both order and tie alike).
//       Run ends from a ballot, c1 from a popcount of the group-1 mask, M by a max over the group; the exact recurrence
//       by __shfl_up inside the group, as many steps as the largest eligible row of the pass has values.  Lane i of the
//       wave keeps the chunk's i-th row; the double precision finish and the stores happen once per chunk.
//   ks_block_kernel: 65 <= n1 + n2 <= 8192, one workgroup per row: ordered compaction + numpy pairwise sum per group,
//       ONE bitonic network in LDS over (group << 32 | f32_ord(v)), NaNs and padding last, after which the two groups
//       are two sorted segments; every thread takes positions q < N and counts both segments at the value of q by two
//       upper-bound searches, so ties need no special case; M is a block max.  A row left with N <= 32 collects its
//       checkpoints (t = c1 + c2 is a run end) with an LDS atomicOr and every wave runs the recurrence.
//
// rowsum.h: PsKey, order bits, lane groups with group_sum, group_sort (both key widths) and group_median, the block's
// compaction, pairwise sum and bitonic network, the median key, the stores of a row, the output pointers with their
// zeroing and staging (D rides in the z slot), launch sizes and the width ladder; colcheck.h: the check of the two groups.
#include "common.h"
#include <math.h>
#include "rowsum.h"
#include "dd.h"

namespace {

constexpr int KS_MAX_GROUP = 4096;       // columns of one group
constexpr int KS_GROUP_MAX = 64;         // selected columns the lane-group kernel takes
constexpr int KS_LEAF_MAX = 64;          // leaves of numpy's pairwise recursion over 4096 values (PW_DEPTH levels)
constexpr int KS_EXACT_MAX = 32;         // kept values of a row the exact form takes: C(32, 16) < 2^32
constexpr double KS_SWITCH = 0.5;        // lam2 from which the alternating series is summed, below it the dual one
constexpr double KS_DROP = 80.0;         // a term exp(-80) < 2^-115 of the leading one is left out

// exp(-a) = m 2^e for a double-double a >= 0, m a double-double in [0.7, 1.42]: a = k ln 2 + r with |r| <= 0.35, exp(-r)
// as the ninth repeated square of the Taylor polynomial of degree 10 at -r / 512 (its remainder is below 2^-140, the
// squarings double a relative error of 2^-104 nine times).  Only +, *, /, fma and sqrt: the host and the device agree.
struct KsExp { DD m; int e; };
__host__ __device__ inline KsExp ks_exp_neg(DD a) {
    const DD ln2 = {0x1.62e42fefa39efp-1, 0x1.abc9e3b39803fp-56};
    const double k = __builtin_rint(a.hi * 0x1.71547652b82fep+0);
    const DD r = dd_add(dd_mul_d(ln2, k), {-a.hi, -a.lo});           // -(a - k ln 2)
    const DD x = {r.hi * 0x1p-9, r.lo * 0x1p-9};
    DD s = {1.0, 0.0};
    for (int n = 10; n >= 1; --n) s = dd_add({1.0, 0.0}, dd_div_d(dd_mul(s, x), (double)n));
    for (int i = 0; i < 9; ++i) s = dd_mul(s, s);
    return {s, -(int)k};
}

// the asymptotic p of a tested row in double-double arithmetic, about 95 bits before the rounding to float64 (the
// printed table is then the referee's to the last digit on every row tested, as the other rank tests' are)
__host__ __device__ inline double ks_asymptotic_p(int M, int nv1, int nv2) {
    if (M == 0) return 1.0;
    const DD lam2 = dd_div_d({(double)((long long)M * M), 0.0}, (double)((long long)nv1 * nv2 * (nv1 + nv2)));
    if (lam2.hi >= KS_SWITCH) {
        DD s = {1.0, 0.0};
        for (int k = 2; k <= 9; ++k) {
            const DD a = dd_mul_d(lam2, 2.0 * (double)(k * k - 1));
            if (a.hi > KS_DROP) break;
            const KsExp t = ks_exp_neg(a);
            const double sc = __builtin_ldexp((k & 1) ? 1.0 : -1.0, t.e);       // (a power of two: the products are exact)
            s = dd_add(s, {t.m.hi * sc, t.m.lo * sc});
        }
        const KsExp lead = ks_exp_neg(dd_mul_d(lam2, 2.0));
        const DD p = dd_mul(lead.m, s);
        return __builtin_ldexp(p.hi + p.lo, lead.e + 1);
    }
    const DD pi2 = {0x1.3bd3cc9be45dep+3, 0x1.692b71366cc04p-51}, two_pi = {0x1.921fb54442d18p+2, 0x1.1a62633145c07p-52};
    const DD c = dd_div(pi2, dd_mul_d(lam2, 8.0));
    DD s = {0.0, 0.0};
    for (int k = 1; k <= 3; ++k) {
        const DD a = dd_mul_d(c, (double)((2 * k - 1) * (2 * k - 1)));
        if (a.hi > KS_DROP) break;
        const KsExp t = ks_exp_neg(a);
        const double sc = __builtin_ldexp(1.0, t.e);
        s = dd_add(s, {t.m.hi * sc, t.m.lo * sc});
    }
    const DD q = dd_mul(dd_sqrt(dd_div(two_pi, lam2)), s);
    const DD p = dd_add({1.0, 0.0}, {-q.hi, -q.lo});
    return fmin(1.0, p.hi + p.lo);
}

// D and p of a tested row: exact (inside, total paths) when total != 0
__device__ __forceinline__ void ks_finish(int M, int nv1, int nv2, uint32_t inside, uint32_t total, double& d, double& p) {
    d = (double)M / (double)(nv1 * nv2);
    p = total ? (double)(total - inside) / (double)total : ks_asymptotic_p(M, nv1, nv2);
}

// The path counts of an eligible row by a (sub)group of lanes, lane i = gl holding cnt[i]: `steps` >= N is wave-uniform,
// `on` uniform in the group; ends: bit t - 1 set when t is a checkpoint.  first: the wave lane of the group's lane 0.
// -> inside and total at (nv1, nv2), to every lane of the group (0, 0 when !on)
__device__ __forceinline__ void ks_path_counts(int gl, int first, bool on, int nv1, int nv2, int M, uint32_t ends, int steps,
                                               uint32_t& inside, uint32_t& total) {
    const int N = nv1 + nv2;
    uint32_t cnt = (on && gl == 0) ? 1u : 0u, tot = cnt;
    for (int t = 1; t <= steps; ++t) {                       // wave-uniform
        uint32_t uc = __shfl_up(cnt, 1), ut = __shfl_up(tot, 1);
        if (gl == 0) { uc = 0u; ut = 0u; }
        if (on && t <= N) {
            cnt += uc;
            tot += ut;
            const int j = t - gl;                            // group-2 values among the first t
            if (gl > nv1 || j < 0 || j > nv2) { cnt = 0u; tot = 0u; }
            else if ((ends >> (t - 1)) & 1u) {
                const int dev = gl * nv2 - j * nv1;
                if ((dev < 0 ? -dev : dev) >= M) cnt = 0u;
            }
        }
    }
    inside = __shfl(cnt, first + (on ? nv1 : 0));
    total = __shfl(tot, first + (on ? nv1 : 0));
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
// the two key widths: padding and the key of a kept value; `key >> 1` is the value and `key & 1` group 1 in both
template <class K> struct KsKey;
template <> struct KsKey<uint32_t> {
    static constexpr uint32_t PAD = PAD32;
    static __device__ __forceinline__ uint32_t make(float v, bool in1) {
        return ((uint32_t)key_of_ps(v).key() << 1) | (in1 ? 1u : 0u);
    }
};
template <> struct KsKey<unsigned long long> {
    static constexpr unsigned long long PAD = ~0ull;
    static __device__ __forceinline__ unsigned long long make(float v, bool in1) {
        return ((unsigned long long)f32_ord(v) << 1) | (in1 ? 1ull : 0ull);
    }
};

// the group's keys -> M, to every lane of the group; ends: bit i set when sorted position i ends a tie run
template <int P, class K>
__device__ __forceinline__ int ks_group_m(K unsorted, int gl, int g0, int nv1, int nv2, unsigned long long& ends) {
    using G = LaneGroup<P>;
    const K key = group_sort<P, K>(unsorted, gl);
    const int N = nv1 + nv2;                                              // the kept keys are positions 0 .. N
    const bool valid = gl < N;
    const K next = __shfl_down(key, 1);
    const bool rend = valid && (gl == N - 1 || (next >> 1) != (key >> 1));
    const unsigned long long m1 = (__ballot(valid && (key & 1)) >> g0) & G::MASK;      // bit i: position i is of group 1
    ends = (__ballot(rend) >> g0) & G::MASK;
    int dev = 0;
    if (rend) {
        const int c1 = __popcll(m1 & ((2ull << gl) - 1ull));              // group-1 values at positions 0..gl
        const int c2 = gl + 1 - c1;
        dev = c1 * nv2 - c2 * nv1;
        dev = dev < 0 ? -dev : dev;
    }
#pragma unroll
    for (int ofs = 1; ofs < P; ofs <<= 1) dev = max(dev, __shfl_xor(dev, ofs));
    return dev;
}

template <int P>
__global__ void __launch_bounds__(256) ks_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                       const int32_t* __restrict__ g1, int n1,
                                                       const int32_t* __restrict__ g2, int n2, int want_exact, int ch,
                                                       TwoSampleOut o, uint8_t* __restrict__ exact) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    __shared__ float cx[4][64], cy[4][64];               // the kept values of the wave's rows, compacted, in list order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    float* X = cx[wave] + g0;
    float* Y = cy[wave] + g0;
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
      int s_tested = 0, s_M = 0, s_nv = 0;
      uint32_t s_inside = 0u, s_total = 0u;
      float s_med1 = 0.f, s_med2 = 0.f, s_mean1 = 0.f, s_mean2 = 0.f;
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf("");
        if (ri < rows_here && gl < m) x = __builtin_nontemporal_load(ps + (row0 + ri) * s + col);
        // (this front is strata.hip's, written out in both: as a helper it changed the kernels and strata's timed slower, A.17)
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
        // ---- the merged order; the narrow key when every row of the pass is on the 3-decimal grid
        unsigned long long ends;
        int M;
        if (__ballot(offgrid) == 0ull)                       // wave-uniform
            M = ks_group_m<P, uint32_t>(kept ? KsKey<uint32_t>::make(x, in1) : KsKey<uint32_t>::PAD, gl, g0, nv1, nv2, ends);
        else
            M = ks_group_m<P, unsigned long long>(kept ? KsKey<unsigned long long>::make(x, in1) : KsKey<unsigned long long>::PAD,
                                                  gl, g0, nv1, nv2, ends);
        const int tested = (nv1 >= 3 && nv2 >= 3) ? 1 : 0;
        // ---- the exact path counts of the rows small enough
        uint32_t inside = 0u, total = 0u;
        if (want_exact) {                                    // uniform over the launch
            const bool on = tested && nv1 + nv2 <= KS_EXACT_MAX;
            int steps = on ? nv1 + nv2 : 0;
#pragma unroll
            for (int ofs = P; ofs < 64; ofs <<= 1) steps = max(steps, __shfl_xor(steps, ofs));
            ks_path_counts(gl, g0, on, nv1, nv2, M, (uint32_t)ends, steps, inside, total);
        }
        // ---- to the lanes that keep the rows of this pass: lane r0 + q takes group q's
        const int src = G::src(lane, r0);
        const bool mine = G::mine(lane, r0);
        const int t_tested = __shfl(tested, src), t_M = __shfl(M, src), t_nv = __shfl(nv1 | (nv2 << 16), src);
        const uint32_t t_inside = __shfl(inside, src), t_total = __shfl(total, src);
        const float t_med1 = __shfl(med1, src), t_med2 = __shfl(med2, src);
        const float t_mean1 = __shfl(sum1 / (float)nv1, src), t_mean2 = __shfl(sum2 / (float)nv2, src);
        if (mine) {
            s_tested = t_tested; s_M = t_M; s_nv = t_nv; s_inside = t_inside; s_total = t_total;
            s_med1 = t_med1; s_med2 = t_med2; s_mean1 = t_mean1; s_mean2 = t_mean2;
        }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = s_tested != 0;
        double d = 0.0, p = 0.0;
        if (tested) ks_finish(s_M, s_nv & 0xffff, s_nv >> 16, s_inside, s_total, d, p);
        store_two_sample(o, row, tested, p, d, s_med1, s_med2, s_mean1, s_mean2);
        if (exact) exact[row] = (tested && s_total != 0u) ? 1 : 0;
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
__global__ void __launch_bounds__(RB_THREADS) ks_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                              const int32_t* __restrict__ g1, int n1,
                                                              const int32_t* __restrict__ g2, int n2, int want_exact, int P,
                                                              TwoSampleOut o, uint8_t* __restrict__ exact) {
    extern __shared__ __align__(16) unsigned char smemks[];
    unsigned long long* A = reinterpret_cast<unsigned long long*>(smemks);      // [P] group << 32 | order bits
    float* F = reinterpret_cast<float*>(A);                                     // first the compaction buffer of the means
    __shared__ float leaf_sum[KS_LEAF_MAX];
    __shared__ float scratch8[KS_LEAF_MAX * 8];
    __shared__ int leaf_off[KS_LEAF_MAX + 1];
    __shared__ int wcnt[RB_THREADS / 64 + 1];
    __shared__ int sh_M;
    __shared__ unsigned sh_ends;
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = n1 + n2;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        // ---- per group: ordered compaction + numpy pairwise sum (np.sum: the identity 0 plus the tree)
        // (written out in strata.hip and ks.hip: as a struct + helper of rowsum.h the LDS layout and the kernel changed, A.17)
        const int nv1 = block_compact(prow, g1, n1, F, wcnt);
        const float sum1 = 0.0f + block_pairwise_sum<PW_DEPTH>(F, nv1, leaf_off, leaf_sum, scratch8, KS_LEAF_MAX);
        const int nv2 = block_compact(prow, g2, n2, F, wcnt);
        const float sum2 = 0.0f + block_pairwise_sum<PW_DEPTH>(F, nv2, leaf_off, leaf_sum, scratch8, KS_LEAF_MAX);
        const bool tested = nv1 >= 3 && nv2 >= 3;               // block-uniform
        const int N = nv1 + nv2;
        int M = 0;
        uint32_t inside = 0u, total = 0u;
        if (tested) {
            // ---- the key of every selected column, NaNs and padding last (the sums are done with F: they end with a barrier)
            for (int j = tid; j < P; j += RB_THREADS) {
                unsigned long long a = ~0ull;
                if (j < m) {
                    const bool in1 = j < n1;
                    a = two_group_median_key(prow[in1 ? g1[j] : g2[j - n1]], in1);
                }
                A[j] = a;
            }
            if (tid == 0) { sh_M = 0; sh_ends = 0u; }
            __syncthreads();
            block_bitonic(P, [=](int i, int l, int desc) {
                const bool asc = desc == 0;
                const unsigned long long ax = A[i], ay = A[l];
                if ((ax > ay) == asc) { A[i] = ay; A[l] = ax; }
            });
            // ---- A[0..nv1) is group 1 sorted, A[nv1..N) group 2: both counts at the value of every position
            const bool on = want_exact && N <= KS_EXACT_MAX;    // block-uniform
            int dev = 0;
            for (int q = tid; q < N; q += RB_THREADS) {
                const unsigned long long v = A[q] & 0xFFFFFFFFull;
                int lo = 0, hi = nv1;                           // first position of group 1 above v
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (A[mid] <= v) lo = mid + 1; else hi = mid; }
                const int c1 = lo;
                const unsigned long long v2 = v | (1ull << 32);
                lo = nv1; hi = N;                               // first position of group 2 above v
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (A[mid] <= v2) lo = mid + 1; else hi = mid; }
                const int c2 = lo - nv1;
                const int dq = c1 * nv2 - c2 * nv1;
                dev = max(dev, dq < 0 ? -dq : dq);
                if (on) atomicOr(&sh_ends, 1u << (c1 + c2 - 1));        // t = c1 + c2 ends a tie run, 1 <= t <= 32
            }
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) dev = max(dev, __shfl_xor(dev, ofs));
            if (lane == 0 && dev) atomicMax(&sh_M, dev);
            __syncthreads();
            M = sh_M;
            // ---- the exact path counts (each wave computes the same; thread 0 stores)
            if (on) ks_path_counts(lane, 0, true, nv1, nv2, M, sh_ends, N, inside, total);
        }
        if (tid == 0) {
            double d = 0.0, p = 0.0;
            float med1 = 0.f, med2 = 0.f;
            if (tested) {
                ks_finish(M, nv1, nv2, inside, total, d, p);
                med1 = median_of_ord(A, nv1);                   // np.median on float32
                med2 = median_of_ord(A + nv1, nv2);
            }
            store_two_sample(o, row, tested, p, d, med1, med2, sum1 / (float)nv1, sum2 / (float)nv2);
            if (exact) exact[row] = (tested && total != 0u) ? 1 : 0;
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

}  // namespace

extern "C" int sdice_ks_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_g1, int32_t n1,
                            const int32_t* d_g2, int32_t n2, int32_t want_exact, uint8_t* d_tested, double* d_p, double* d_d,
                            float* d_med1, float* d_med2, float* d_mean1, float* d_mean2, float* d_delta, uint8_t* d_exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_TRY(check_two_groups("sdice_ks", nullptr, n1, nullptr, n2, s, KS_MAX_GROUP));      // (device lists: the counts)
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_med1 && d_med2 && d_mean1 && d_mean2 && d_delta, "NULL output");
    SD_ARG(!want_exact || d_exact, "NULL output: exact is required with want_exact");
    SD_ARG(d_ps && d_g1 && d_g2, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    TwoSampleOut o{d_tested, d_p, d_d, d_med1, d_med2, d_mean1, d_mean2, d_delta};
    const int m = n1 + n2;
    const int we = want_exact ? 1 : 0;
    if (n1 < 3 || n2 < 3) {                                    // no row can be tested
        if (d_exact) SD_HIP(hipMemsetAsync(d_exact, 0, (size_t)n, ctx->stream));
        return zero_two_sample(ctx, n, o);
    }
    if (m <= KS_GROUP_MAX)
        return with_group_launch(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "ks_group_kernel", (ks_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_g1, (int)n1, d_g2, (int)n2, we, ch, o, d_exact);
            return SDICE_OK;
        });
    const int P = next_pow2(m, 128);
    const size_t lds = (size_t)P * 8;
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH_LDS(ctx, "ks_block_kernel", ks_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n, (int)s, d_g1,
                  (int)n1, d_g2, (int)n2, we, P, o, d_exact);
    return SDICE_OK;
}

extern "C" int sdice_ks(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* g1, int32_t n1,
                        const int32_t* g2, int32_t n2, int32_t want_exact, uint8_t* tested, double* p, double* d, float* med1,
                        float* med2, float* mean1, float* mean2, float* delta, uint8_t* exact) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(g1 && g2, "index list is NULL");
    SD_TRY(check_two_groups(__func__, g1, n1, g2, n2, s, KS_MAX_GROUP));
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && med1 && med2 && mean1 && mean2 && delta, "NULL output");
    SD_ARG(!want_exact || exact, "NULL output: exact is required with want_exact");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    TwoSampleOut o;
    uint8_t* d_exact = nullptr;                                // stays NULL when the caller gave no `exact`
    float* d_ps;
    int32_t *dg1, *dg2;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dg1, g1, n1));
    SD_TRY(st.upload(&dg2, g2, n2));
    SD_TRY(stage_two_sample(st, n, {tested, p, d, med1, med2, mean1, mean2, delta}, &o, exact, exact ? &d_exact : nullptr));
    SD_TRY(sdice_ks_dev(ctx, n, s, d_ps, dg1, n1, dg2, n2, want_exact, o.tested, o.p, o.z, o.med1, o.med2, o.mean1, o.mean2,
                        o.delta, d_exact));
    return st.download_results();
}
