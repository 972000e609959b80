// K14: Spearman rank correlation per junction row between the PS values of m listed columns and one covariate value per
// listed column + n / mean / median of the row's kept PS values (the `correlate` sub-command).
//
// scipy.stats.spearmanr(x_kept, ps_kept) per row: a sample is kept when its PS value is not NaN, the row is tested when
// at least 3 are kept, the covariate is ranked again among the kept samples of each row, rho is the Pearson correlation of
// the two average-rank vectors and p = 2 t.sf(|t|, nu) = I_{1 - rho^2}(nu / 2, 1 / 2), nu = n' - 2.  PS values tie by
// float32 equality (-0.0 == +0.0), covariate values by the tie-group ids the host passes.
//
// What arrives: the columns sorted by covariate (ties in table order) and a dense tie-group id per column, xg[0] = 0,
// non-decreasing in steps of 0 or 1.  The covariate itself never reaches the device: the ranks of a row's kept subset
// are a prefix count over the kept flags in that order, closed per tie group --
//   a2 = 2 * average covariate rank = (kept before the group) + (kept up to the group's end) + 1
//   b2 = 2 * average PS rank        = 2 (kept values below) + (kept values equal, itself included) + 1
// Arithmetic, in integers up to the last step: both doubled rank vectors sum to S = n'(n'+1), so with
//   N  = n' sum(a2 b2) - S^2,   Dx = n' sum(a2^2) - S^2,   Dy = n' sum(b2^2) - S^2        (below 2^47 at 4096 samples)
//   rho = N / sqrt(Dx Dy),   1 - rho^2 = (Dx Dy - N^2) / (Dx Dy)   with the products as 128-bit integers (93 bits)
// there is no rank rounding and no cancellation near |rho| = 1.  Dx = 0 or Dy = 0 (covariate or PS constant among the
// kept; scipy: NaN): rho = 0, p = 1, the row stays tested.  N = 0: p = 1.  N^2 = Dx Dy: rho = +-1, p = 0, also at 3 kept
// samples (scipy's t approximation; no exact or permutation p).  Otherwise rho is the double-double square root of
// N^2 / (Dx Dy), rounded once, and p is the regularized incomplete beta:
//   up to 64 kept samples: a power series in double-double arithmetic (sp_beta_half_dd), the correctly rounded float64 --
//       the table `correlate` prints equals the 50-digit referee's byte for byte there;
//   above: in float64 by the continued fraction (modified Lentz), taken from the side that converges: I_x(a, 1/2)
//       directly for x < (a + 1) / (a + 5/2), else 1 - I_{rho^2}(1/2, a) -- where that branch is taken p is above 0.05
//       and nothing cancels.  Within 1e-12 relative of the referee at 4096 samples.
//
// Kernels:
//   spearman_group_kernel<P>: m <= 64, P = 8, 16, 32 or 64 lanes own a row, one column per lane, 64 / P rows per wave side
//       by side (the lane groups of signedrank.hip).  The PS ranks need no sort: every lane reads the group's P values one
//       after another and counts those below and equal to its own; the median is the value of the lane whose rank interval
//       holds the middle position.  Covariate ranks: two popcounts of the kept mask.  The kept values are compacted through
//       the wave's LDS for the numpy-order sum (one leaf of numpy's pairwise recursion).  Lane i of a wave keeps the
//       results of the chunk's i-th row; the float64 finish and the stores happen once per chunk.
//   spearman_wave_kernel<E>: 65 <= m <= 256, one wave per row, E = 2 or 4 columns per lane, the same steps: every value
//       is broadcast once (v_readlane) and every lane counts against its E values; covariate ranks from 2 E popcounts of
//       the E kept masks; the sum by wave_pairwise_sum.
//   spearman_block_kernel: 257 <= m <= 4096, one workgroup per row after signedrank_block_kernel: ordered compaction that
//       also leaves the kept-prefix of every list position, block_pairwise_sum, one LDS bitonic sort of the order bits
//       that carries a2 as a 16-bit payload, run bounds by binary search.  The tie-group bounds of the list positions are
//       found once per workgroup.
// (Left out: a wave-per-row tier for 257..1024 columns -- counting is quadratic in m and stops paying there -- and the
// 1001-bin count for rows of 3-decimal values; the block kernel computes the same thing.)
//
// rowsum.h: the order bits of a float, the lane groups with their sums, wave_pairwise_sum, the block's compaction, pairwise
// sum, bitonic network and run bounds, the launch sizes and the column check; dd.h: the double-double arithmetic.
#include "common.h"
#include <math.h>
#include "rowsum.h"
#include "dd.h"

namespace {

constexpr int SP_MIN_COLS = 3;
constexpr int SP_MAX_COLS = 4096;
constexpr int SP_GROUP_MAX = 64;         // columns the lane-group kernel takes
constexpr int SP_WAVE_MAX = 256;         // columns the wave-per-row kernel takes
constexpr int SP_LEAF_MAX = 64;          // leaves of numpy's pairwise recursion over 4096 values (PW_DEPTH levels)
constexpr uint32_t SP_PAD = 0xFFFFFFFFu;

struct SpOut {
    uint8_t* tested;
    double* p;
    double* rho;     // may be NULL
    int32_t* n_kept;
    float* med;
    float* mean;
};

// ---- p: I_x(a, 1/2) in float64
// continued fraction of the incomplete beta function (modified Lentz); converges in O(sqrt(max(a, b))) rounds for
// x < (a + 1) / (a + b + 2)
__host__ __device__ inline double sp_betacf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 2.3e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int i = 1; i <= 4000; ++i) {
        const double fi = (double)i, i2 = 2.0 * fi;
        double aa = fi * (b - fi) * x / ((qam + i2) * (a + i2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + fi) * (qab + fi) * x / ((a + i2) * (qap + i2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return h;
}

// I_x(a, 1/2), a >= 31.5, with y = 1 - x given apart (both come from the integers, neither from the other).
// ln(Gamma(a + 1/2) / Gamma(a)) by its asymptotic series, not as a difference of two lgamma of size 1e4: the next term,
// 31 / (18432 a^9), is below 6e-17 from a = 31.5 up.
__host__ __device__ inline double sp_beta_half(double a, double x, double y) {
    const double ln_sqrt_pi = 0.5723649429247000870717;
    const double w = 1.0 / a, w2 = w * w;
    const double ln_ratio = 0.5 * log(a) - w * (1.0 / 8.0 - w2 * (1.0 / 192.0 - w2 * (1.0 / 640.0 - w2 * (17.0 / 14336.0))));
    const double front = exp(ln_ratio - ln_sqrt_pi + a * log(x) + 0.5 * log(y));
    double r;
    if (x < (a + 1.0) / (a + 2.5)) r = front * sp_betacf(a, 0.5, x) / a;
    else r = 1.0 - front * sp_betacf(0.5, a, y) * 2.0;
    return r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
}

// ---- in double-double arithmetic (dd.h): rho everywhere, and p of the rows with at most SP_DD_MAX_KEPT kept samples,
// where the float64 that comes out is the correctly rounded one (the continued fraction is a few 1e-15 off, which shows
// in the last printed digit of the table)
constexpr int SP_DD_MAX_KEPT = 64;
// I_x(a, 1/2), a = nu / 2 <= 31, from x = 1 - rho^2, y = rho^2 and r = |rho|: with front = r x^a / B(a, 1/2),
//   x <= 1/2:  front / a * sum_k (a + 1/2)_k / (a + 1)_k x^k            (every term positive: exact down any tail)
//   else:      1 - 2 front * sum_k (a + 1/2)_k / (3/2)_k y^k            (y < 1/2, p > 1e-10: at most 34 of the 106 bits cancel)
// B by B(a + 1, 1/2) = B(a, 1/2) a / (a + 1/2) from B(1/2, 1/2) = pi or B(1, 1/2) = 2
__host__ __device__ inline double sp_beta_half_dd(int nu, DD x, DD y, DD r) {
    const DD pi = {0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53};
    double a0 = (nu & 1) ? 0.5 : 1.0;
    DD front = (nu & 1) ? dd_div(dd_sqrt(x), pi) : dd_mul_d(x, 0.5);     // x^a0 / B(a0, 1/2)
    const double a = 0.5 * (double)nu;
    for (; a0 < a; a0 += 1.0) front = dd_div_d_recip(dd_mul_d(dd_mul(front, x), a0 + 0.5), a0);
    front = dd_mul(front, r);
    const bool direct = x.hi <= 0.5;
    const DD z = direct ? x : y;
    const double den0 = direct ? a + 1.0 : 1.5;
    DD term = {1.0, 0.0}, sum = {1.0, 0.0};
    for (int k = 0; k < 4000; ++k) {
        term = dd_div_d_recip(dd_mul_d(dd_mul(term, z), a + 0.5 + (double)k), den0 + (double)k);
        sum = dd_add(sum, term);
        if (term.hi < sum.hi * 0x1p-112 && z.hi * (a + 1.5 + (double)k) < den0 + 1.0 + (double)k) break;   // past the peak
    }
    DD p = dd_mul(front, sum);
    if (direct) p = dd_div_d_recip(p, a);
    else p = dd_add({1.0, 0.0}, {-2.0 * p.hi, -2.0 * p.lo});
    return p.hi + p.lo;
}

// rho and p of a tested row from the integer sums over its nv kept samples
__host__ __device__ inline void sp_finish(int nv, long long sab, long long saa, long long sbb, double& rho, double& p) {
    const long long S = (long long)nv * (nv + 1);
    const long long N = nv * sab - S * S, Dx = nv * saa - S * S, Dy = nv * sbb - S * S;
    rho = 0.0;
    p = 1.0;
    if (Dx == 0 || Dy == 0 || N == 0) return;            // a constant side; no monotone trend
    const unsigned long long an = (unsigned long long)(N < 0 ? -N : N);
    const unsigned __int128 DXY = (unsigned __int128)(unsigned long long)Dx * (unsigned long long)Dy;
    const unsigned __int128 NN = (unsigned __int128)an * an;
    if (NN >= DXY) {                                       // (Cauchy-Schwarz: never above)
        rho = N > 0 ? 1.0 : -1.0;
        p = 0.0;
        return;
    }
    const DD dd = dd_u128(DXY);
    const DD x = dd_div(dd_u128(DXY - NN), dd), y = dd_div(dd_u128(NN), dd);      // 1 - rho^2, rho^2
    const DD r = dd_sqrt(y);
    rho = N > 0 ? r.hi + r.lo : -(r.hi + r.lo);
    if (nv <= SP_DD_MAX_KEPT) p = sp_beta_half_dd(nv - 2, x, y, r);
    else p = sp_beta_half(0.5 * (double)(nv - 2), x.hi, y.hi);
}

// ------------------------------------------------------------------ lane-group path: P lanes per row
template <int P>
__global__ void __launch_bounds__(256) spearman_group_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                             const int32_t* __restrict__ cols, const int32_t* __restrict__ xg,
                                                             int m, int ch, SpOut o) {
    using G = LaneGroup<P>;                              // G::R rows side by side in a wave
    __shared__ float cx[4][64];                          // the kept values of the wave's rows, compacted, in list order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int g = lane / P, gl = lane % P, g0 = g * P;
    float* X = cx[wave] + g0;
    const int col = gl < m ? cols[gl] : 0;
    // the covariate tie group of this lane's list position covers the positions [glo, ghi) (a lane past the list is a
    // group of its own)
    unsigned long long below_lo, below_hi;
    {
        const int mine = gl < m ? xg[gl] : -1 - gl;
        const int prev = __shfl_up(mine, 1);
        const unsigned long long sm = (__ballot(gl == 0 || prev != mine) >> g0) & G::MASK;      // bit i: a group starts at i
        const unsigned long long upto = (2ull << gl) - 1ull;                                   // positions 0..gl
        const int glo = 63 - __clzll((long long)(sm & upto));
        const unsigned long long above = sm & ~upto;
        const int ghi = above ? (__ffsll((long long)above) - 1) : P;
        below_lo = (1ull << glo) - 1ull;
        below_hi = ghi >= 64 ? ~0ull : ((1ull << ghi) - 1ull);
    }
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_nv = 0, s_ab = 0, s_aa = 0, s_bb = 0;        // sums of products of doubled ranks <= 64 * 129^2
      float s_med = 0.f, s_mean = 0.f;
      for (int r0 = 0; r0 < rows_here; r0 += G::R) {        // wave-uniform
        const int ri = r0 + g;
        float x = __builtin_nanf("");
        if (ri < rows_here && gl < m) x = __builtin_nontemporal_load(ps + (row0 + ri) * s + col);
        const bool kept = x == x;
        const unsigned long long km = (__ballot(kept) >> g0) & G::MASK;
        const int nv = __popcll(km);
        // ---- the numpy-order sum over the compacted values
        SD_WAVE_SYNC();          // the previous pass's readers are done with the wave's LDS
        if (kept) X[__popcll(km & ((1ull << gl) - 1ull))] = x;
        SD_WAVE_SYNC();
        const float sum = 0.0f + group_sum(X, nv, gl);            // np.sum starts from the identity 0: -0.0 values sum to +0.0
        // ---- PS ranks by counting
        const uint32_t xo = kept ? f32_ord(x) : SP_PAD;
        int less = 0, eq = 0;
#pragma unroll 8
        for (int j = 0; j < P; ++j) {
            const uint32_t v = __shfl(xo, g0 + j);
            less += v < xo ? 1 : 0;
            eq += v == xo ? 1 : 0;
        }
        // ---- the median: the values whose rank intervals [less, less + eq) hold positions h and h - 1
        const int h = nv >> 1;
        const unsigned long long mh = __ballot(kept && less <= h && h < less + eq) >> g0 & G::MASK;
        const unsigned long long ml = __ballot(kept && less <= h - 1 && h - 1 < less + eq) >> g0 & G::MASK;
        const float v1 = f32_unord(__shfl(xo, g0 + (mh ? __ffsll((long long)mh) - 1 : 0)));
        const float v0 = f32_unord(__shfl(xo, g0 + (ml ? __ffsll((long long)ml) - 1 : 0)));
        const float med = (nv & 1) ? v1 : (v0 + v1) / 2.0f;
        // ---- the sums of the doubled ranks' products
        const int a2 = __popcll(km & below_lo) + __popcll(km & below_hi) + 1;
        const int b2 = 2 * less + eq + 1;
        const int ab = group_add<P>(kept ? a2 * b2 : 0);
        const int aa = group_add<P>(kept ? a2 * a2 : 0);
        const int bb = group_add<P>(kept ? b2 * b2 : 0);
        // ---- to the lanes that keep the rows of this pass: lane r0 + q takes group q's
        const int src = G::src(lane, r0);
        const bool mine = G::mine(lane, r0);
        const int t_nv = __shfl(nv, src), t_ab = __shfl(ab, src), t_aa = __shfl(aa, src), t_bb = __shfl(bb, src);
        const float t_med = __shfl(med, src), t_mean = __shfl(sum / (float)nv, src);
        if (mine) { s_nv = t_nv; s_ab = t_ab; s_aa = t_aa; s_bb = t_bb; s_med = t_med; s_mean = t_mean; }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = s_nv >= 3;
        double rho = 0.0, p = 0.0;
        if (tested) sp_finish(s_nv, (long long)s_ab, (long long)s_aa, (long long)s_bb, rho, p);
        o.tested[row] = tested ? 1 : 0;
        o.p[row] = p;
        if (o.rho) o.rho[row] = rho;
        o.n_kept[row] = tested ? s_nv : 0;
        o.med[row] = tested ? s_med : 0.f;
        o.mean[row] = tested ? s_mean : 0.f;
      }
    }
}

// ------------------------------------------------------------------ wave path: one wave per row, E columns per lane
// list position e * 64 + lane is element e of the lane, so a load and a ballot cover 64 consecutive positions
template <int E>
__global__ void __launch_bounds__(256) spearman_wave_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                            const int32_t* __restrict__ cols, const int32_t* __restrict__ xg,
                                                            int m, int ch, SpOut o) {
    constexpr int DEPTH = 2;                             // numpy's pairwise recursion over at most 256 values: 4 leaves
    __shared__ float cx[4][64 * E];                      // the kept values of the wave's row, compacted, in list order
    __shared__ int leaf_off[4][(1 << DEPTH) + 1];
    __shared__ float leaf_sum[4][1 << DEPTH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    float* X = cx[wave];
    // the column of each of the lane's list positions and the bounds [glo, ghi) of its covariate tie group (xg never
    // decreases); a position past the list has no column and an empty group
    int col[E], glo[E], ghi[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int q = e * 64 + lane;
        col[e] = 0; glo[e] = 0; ghi[e] = 0;
        if (q < m) {
            col[e] = cols[q];
            // (written out: through run_bounds of rowsum.h both instantiations change, and no timing tool lists the
            // 129..256 columns that reach E = 4)
            const int mine = xg[q];
            int lo = 0, hi = q;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (xg[mid] < mine) lo = mid + 1; else hi = mid; }
            glo[e] = lo;
            lo = q + 1; hi = m;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (xg[mid] <= mine) lo = mid + 1; else hi = mid; }
            ghi[e] = lo;
        }
    }
    const int64_t n_chunks = (n + ch - 1) / ch;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
      const int64_t row0 = c * ch;
      const int rows_here = (int)min((int64_t)ch, n - row0);
      // lane i keeps the chunk's i-th row
      int s_nv = 0, s_ab = 0, s_aa = 0, s_bb = 0;        // sums of products of doubled ranks <= 256 * 513^2
      float s_med = 0.f, s_mean = 0.f;
      for (int r = 0; r < rows_here; ++r) {              // wave-uniform
        const float* prow = ps + (row0 + r) * s;
        float x[E];
        unsigned long long km[E];
        int base[E], nv = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x[e] = __builtin_nanf("");
            if (e * 64 + lane < m) x[e] = __builtin_nontemporal_load(prow + col[e]);
            km[e] = __ballot(x[e] == x[e]);
            base[e] = nv;
            nv += __popcll(km[e]);
        }
        // ---- the numpy-order sum over the compacted values
        SD_WAVE_SYNC();          // the previous row's readers are done with the wave's LDS
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (x[e] == x[e]) X[base[e] + lanes_below(km[e])] = x[e];
        SD_WAVE_SYNC();
        const float sum = 0.0f + wave_pairwise_sum<DEPTH>(FloatAt{X}, nv, lane, leaf_off[wave], leaf_sum[wave]);
        // ---- PS ranks by counting: every position's value is broadcast once
        uint32_t xo[E];
        int less[E], eq[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xo[e] = x[e] == x[e] ? f32_ord(x[e]) : SP_PAD;
            less[e] = 0; eq[e] = 0;
        }
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            const int jn = min(64, m - e2 * 64);         // wave-uniform
            for (int j = 0; j < jn; ++j) {
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)xo[e2], j);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    less[e] += v < xo[e] ? 1 : 0;
                    eq[e] += v == xo[e] ? 1 : 0;
                }
            }
        }
        // ---- the median: the values whose rank intervals [less, less + eq) hold positions h and h - 1
        const int h = nv >> 1;
        uint32_t o1 = 0, o0 = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool kept = x[e] == x[e];
            const unsigned long long mh = __ballot(kept && less[e] <= h && h < less[e] + eq[e]);
            const unsigned long long ml = __ballot(kept && less[e] <= h - 1 && h - 1 < less[e] + eq[e]);
            if (mh) o1 = (uint32_t)__builtin_amdgcn_readlane((int)xo[e], __ffsll((long long)mh) - 1);      // (wave-uniform)
            if (ml) o0 = (uint32_t)__builtin_amdgcn_readlane((int)xo[e], __ffsll((long long)ml) - 1);
        }
        const float v1 = f32_unord(o1), v0 = f32_unord(o0);
        const float med = (nv & 1) ? v1 : (v0 + v1) / 2.0f;
        // ---- the sums of the doubled ranks' products
        int ab = 0, aa = 0, bb = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            int before = 0, upto = 0;                    // kept positions below glo, below ghi
#pragma unroll
            for (int e2 = 0; e2 < E; ++e2) {
                const int bl = glo[e] - e2 * 64, bh = ghi[e] - e2 * 64;
                before += bl >= 64 ? __popcll(km[e2]) : (bl <= 0 ? 0 : __popcll(km[e2] & ((1ull << bl) - 1ull)));
                upto += bh >= 64 ? __popcll(km[e2]) : (bh <= 0 ? 0 : __popcll(km[e2] & ((1ull << bh) - 1ull)));
            }
            if (x[e] == x[e]) {
                const int a2 = before + upto + 1, b2 = 2 * less[e] + eq[e] + 1;
                ab += a2 * b2;
                aa += a2 * a2;
                bb += b2 * b2;
            }
        }
        ab = group_add<64>(ab);
        aa = group_add<64>(aa);
        bb = group_add<64>(bb);
        if (lane == r) { s_nv = nv; s_ab = ab; s_aa = aa; s_bb = bb; s_med = med; s_mean = sum / (float)nv; }
      }
      if (lane < rows_here) {
        const int64_t row = row0 + lane;
        const bool tested = s_nv >= 3;
        double rho = 0.0, p = 0.0;
        if (tested) sp_finish(s_nv, (long long)s_ab, (long long)s_aa, (long long)s_bb, rho, p);
        o.tested[row] = tested ? 1 : 0;
        o.p[row] = p;
        if (o.rho) o.rho[row] = rho;
        o.n_kept[row] = tested ? s_nv : 0;
        o.med[row] = tested ? s_med : 0.f;
        o.mean[row] = tested ? s_mean : 0.f;
      }
    }
}

// ------------------------------------------------------------------ general path: one workgroup per row
__global__ void __launch_bounds__(RB_THREADS) spearman_block_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                                    const int32_t* __restrict__ cols,
                                                                    const int32_t* __restrict__ xg, int m, int P, SpOut o) {
    extern __shared__ __align__(16) unsigned char smems[];
    uint32_t* K = reinterpret_cast<uint32_t*>(smems);          // [P] first the compacted floats, then their order bits
    uint32_t* GB = K + P;                                       // [P] list position -> its tie group's ghi << 16 | glo
    unsigned short* A = reinterpret_cast<unsigned short*>(GB + P);   // [P] kept element -> list position, then its a2
    unsigned short* C = A + P;                                  // [P + 2] list position -> kept values before it; C[m] = all
    float* F = reinterpret_cast<float*>(K);
    __shared__ float leaf_sum[SP_LEAF_MAX];
    __shared__ float scratch8[SP_LEAF_MAX * 8];
    __shared__ int leaf_off[SP_LEAF_MAX + 1];
    __shared__ int wcnt[RB_THREADS / 64];
    __shared__ unsigned long long accS[3];                      // sum a2 b2, sum a2^2, sum b2^2
    const int tid = threadIdx.x, lane = tid & 63;
    // the tie-group bounds of every list position, once: xg never decreases
    for (int q = tid; q < m; q += RB_THREADS) {
        const RunBounds grp = run_bounds(xg, m, xg[q], ProjSelf{}, q);
        GB[q] = ((uint32_t)grp.past << 16) | (uint32_t)grp.first;
    }
    __syncthreads();
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* prow = ps + row * s;
        // ---- ordered compaction of the non-NaN values, with the list position of each and the prefix of every position
        const int nv = block_compact_by(
            m, wcnt,
            [=](int q) { return q < m ? prow[cols[q]] : __builtin_nanf(""); },
            [=](int q, int pos, bool valid, float x) {
                if (q < m) C[q] = (unsigned short)pos;
                if (valid) {
                    F[pos] = x;
                    A[pos] = (unsigned short)q;
                }
            });
        if (nv < 3) {                                           // block-uniform
            if (tid == 0) {
                o.tested[row] = 0; o.p[row] = 0.0;
                if (o.rho) o.rho[row] = 0.0;
                o.n_kept[row] = 0; o.med[row] = 0.f; o.mean[row] = 0.f;
            }
            continue;                                           // (the compaction ended with a barrier)
        }
        if (tid == 0) C[m] = (unsigned short)nv;
        if (tid < 3) accS[tid] = 0ull;
        // np.sum: the identity 0 plus the pairwise tree
        const float sum = 0.0f + block_pairwise_sum<PW_DEPTH>(F, nv, leaf_off, leaf_sum, scratch8, SP_LEAF_MAX);
        // ---- covariate ranks of the kept, order bits of their values, padding last (each index in place)
        for (int i = tid; i < P; i += RB_THREADS) {
            uint32_t k = SP_PAD;
            unsigned short a2 = 0;
            if (i < nv) {
                const uint32_t gb = GB[A[i]];
                a2 = (unsigned short)((int)C[gb & 0xffffu] + (int)C[gb >> 16] + 1);
                k = f32_ord(F[i]);
            }
            K[i] = k;
            A[i] = a2;
        }
        __syncthreads();
        block_bitonic(P, [=](int i, int l, int desc) {           // a2 carried along as the payload; equal keys stay
            const bool asc = desc == 0;
            const uint32_t x = K[i], y = K[l];
            if ((x > y) == asc && x != y) {
                K[i] = y; K[l] = x;
                const unsigned short t = A[i];
                A[i] = A[l]; A[l] = t;
            }
        });
        // ---- PS ranks from the run bounds
        long long ab = 0, aa = 0, bb = 0;
        for (int q = tid; q < nv; q += RB_THREADS) {
            const uint32_t code = K[q];
            const RunBounds run = run_bounds(K, nv, code, ProjSelf{}, q);
            const long long b2 = run.first + run.past + 1, a2 = A[q];
            ab += a2 * b2;
            aa += a2 * a2;
            bb += b2 * b2;
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            ab += __shfl_xor(ab, ofs);
            aa += __shfl_xor(aa, ofs);
            bb += __shfl_xor(bb, ofs);
        }
        if (lane == 0) {
            atomicAdd(&accS[0], (unsigned long long)ab);
            atomicAdd(&accS[1], (unsigned long long)aa);
            atomicAdd(&accS[2], (unsigned long long)bb);
        }
        __syncthreads();
        if (tid == 0) {
            const float med = median_of_ord(K, nv);             // np.median on float32
            double rho, p;
            sp_finish(nv, (long long)accS[0], (long long)accS[1], (long long)accS[2], rho, p);
            o.tested[row] = 1; o.p[row] = p;
            if (o.rho) o.rho[row] = rho;
            o.n_kept[row] = nv; o.med[row] = med; o.mean[row] = sum / (float)nv;
        }
        __syncthreads();           // thread 0 has read the row's LDS
    }
}

template <int E>
int sp_launch_wave(sdice_ctx* ctx, const float* d_ps, int64_t n, int s, const int32_t* d_cols, const int32_t* d_xg, int m,
                   SpOut o) {
    const int waves = 4;
    const int ch = rows_per_chunk(ctx->n_cu, n);
    const int64_t blocks = wave_launch_blocks(ctx, n, ch, waves);
    SD_LAUNCH(ctx, "spearman_wave_kernel", (spearman_wave_kernel<E>), dim3((unsigned)blocks), dim3(waves * 64), 0, d_ps, n,
              s, d_cols, d_xg, m, ch, o);
    return SDICE_OK;
}

int sp_check_scalars(int64_t n, int32_t s, int32_t m) {
    SD_ARG(n >= 0 && s >= 0, "negative size");
    if (m < SP_MIN_COLS || m > SP_MAX_COLS) {
        sdice_set_error("sdice_spearman: %d columns listed, %d..%d are supported", (int)m, SP_MIN_COLS, SP_MAX_COLS);
        return SDICE_ERR_ARG;
    }
    SD_ARG(m <= s, "more columns listed than the table has (a column may be listed once)");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_spearman_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                                  const int32_t* d_xg, int32_t m, uint8_t* d_tested, double* d_p, double* d_rho,
                                  int32_t* d_n_kept, float* d_med, float* d_mean) {
    SD_ARG(ctx, "ctx is NULL");
    SD_TRY(sp_check_scalars(n, s, m));
    if (n == 0) return SDICE_OK;
    SD_ARG(d_tested && d_p && d_n_kept && d_med && d_mean, "NULL output");
    SD_ARG(d_ps && d_cols && d_xg, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    SD_TRY(ctx->arena.reset(ctx->stream));
    SpOut o{d_tested, d_p, d_rho, d_n_kept, d_med, d_mean};
    if (m <= SP_GROUP_MAX)
        return with_group_launch(ctx, n, m, [&](auto width, int ch, int64_t blocks) -> int {
            SD_LAUNCH(ctx, "spearman_group_kernel", (spearman_group_kernel<decltype(width)::value>), dim3((unsigned)blocks),
                      dim3(GROUP_WAVES * 64), 0, d_ps, n, (int)s, d_cols, d_xg, (int)m, ch, o);
            return SDICE_OK;
        });
    if (m <= SP_WAVE_MAX / 2) return sp_launch_wave<2>(ctx, d_ps, n, s, d_cols, d_xg, m, o);
    if (m <= SP_WAVE_MAX) return sp_launch_wave<4>(ctx, d_ps, n, s, d_cols, d_xg, m, o);
    const int P = next_pow2(m, 512);
    const size_t lds = (size_t)P * 12 + 8;                // K, GB: 4 bytes each; A, C: 2 bytes each, C two entries longer (49160 B at most)
    const int64_t blocks = row_launch_blocks(ctx, n);
    SD_LAUNCH(ctx, "spearman_block_kernel", spearman_block_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), lds, d_ps, n,
              (int)s, d_cols, d_xg, (int)m, P, o);
    return SDICE_OK;
}

extern "C" int sdice_spearman(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                              const int32_t* xg, int32_t m, uint8_t* tested, double* p, double* rho, int32_t* n_kept,
                              float* med, float* mean) {
    SD_ARG(ctx, "ctx is NULL");
    SD_TRY(sp_check_scalars(n, s, m));
    SD_ARG(cols && xg, "column list or tie-group list is NULL");
    SD_TRY(check_columns(__func__, {cols}, m, s, "column index out of range", "a column may be listed once"));
    SD_ARG(xg[0] == 0, "xg must start at 0");
    for (int q = 1; q < m; ++q) SD_ARG(xg[q] == xg[q - 1] || xg[q] == xg[q - 1] + 1, "xg must rise in steps of 0 or 1");
    if (n == 0) return SDICE_OK;
    SD_ARG(tested && p && n_kept && med && mean, "NULL output");
    SD_ARG(ps, "ps is NULL");
    HostStaging st(ctx);
    float* d_ps;
    int32_t *dc, *dg;
    SpOut d;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dc, cols, m));
    SD_TRY(st.upload(&dg, xg, m));
    st.result(&d.tested, tested, n);
    st.result(&d.p, p, n);
    st.result(&d.rho, rho, n);
    st.result(&d.n_kept, n_kept, n);
    st.result(&d.med, med, n);
    st.result(&d.mean, mean, n);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_spearman_dev(ctx, n, s, d_ps, dc, dg, m, d.tested, d.p, d.rho, d.n_kept, d.med, d.mean));
    return st.download_results();
}
