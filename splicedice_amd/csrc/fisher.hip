// K6: two-sided Fisher exact test for every sample pair of every junction.
//
// Replaces the inner loop of pairwise (pairwise_fisher.py:164-179):
//   table = [[incl_a, incl_b], [excl_a, excl_b]];  p = scipy.stats.fisher_exact(table)[1]
// scipy (1.15.3, _stats_py.py fisher_exact): any zero margin -> 1.0; otherwise, with
// n1 = a+b, n2 = c+d, n = a+c and the hypergeometric pmf over k = table[0][0], the
// two-sided p is the sum of pmf(k) over the support with pmf(k) <= pmf(a) * (1 + 1e-14)
// (its cdf/sf + binary-search branches compute exactly that set), clipped at 1.
//
// Here: pmf(a) from a log-factorial table in HBM/L2 (the saddle-point form beyond the table), and
// the RATIOS r_k = pmf(k)/pmf(a) by the exact one-step recurrence outward from k = a in both
// directions, so the tie test r_k <= 1 + 1e-12 is decided to ~1e-14, far tighter than a
// log-gamma difference could.  p = pmf(a) * (1 + sum of the accepted r_k).  Monotone tails are
// cut once the remaining mass is below 1e-13 of the sum (the pmf is log-concave).
// The kernel is f64-VALU bound (O(support) steps per p-value), not HBM bound.
#include "pairs.h"
#include <algorithm>

namespace {

struct LfTable {
    const double* lf;   // lf[k] = lgamma(k + 1), k in [0, n)
    long long n;
};

// ---- log pmf(a) of a table whose total lies beyond the log-factorial table (fisher.table_max, 2^20 by default).
// The nine log-factorials cancel from ~M log M down to ~1e2, so their difference carries a few ulp of lgamma(M): 2e-9 at
// M = 2^20, 1e-5 at 1e9, 4e-3 at 2^40.  With log x! = x log x - x + h(x) the linear terms cancel identically (margins and
// cells both add up to 2M) and the x log x terms collect into the cells' deviances from their expectations
// e = row * col / M (Loader's saddle-point form of the hypergeometric pmf):
//   log pmf(a) = h(n1) + h(n2) + h(n) + h(m) - h(M) - h(a) - h(b) - h(c) - h(d) - sum over the cells of dev(x, e),
//   dev(x, e) = x log(x / e) + e - x >= 0.
// Every term is of the size of the result: h(x) = 0.5 log(2 pi x) + O(1/x) and the deviances sum to -log pmf(a) up to
// the h's, so the error is a few 1e-15 whatever the counts are.
// h(x): 0 at x = 0; lgamma below 16; from there the Stirling series (the first term left out, (691/360360) x^-11, is
// below 1.1e-16).
__device__ double stirling_rest(double x) {
    if (x == 0.0) return 0.0;
    if (x < 16.0) return lgamma(x + 1.0) - (x * log(x) - x);
    const double r = 1.0 / (x * x);
    const double s = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) * r) * r) * r) * r) / x;
    return 0.5 * log(6.283185307179586 * x) + s;
}
// dev(x, e) with delta = x - e given to full precision (x - e itself cancels when x is large).  Near the expectation,
// with v = delta / (x + e):  x / e = (1 + v) / (1 - v), log(x / e) = 2 atanh(v), 2 x v - delta = delta v, so
// dev = delta v + 2 x v (v^2 / 3 + v^4 / 5 + ...): |v| < 0.1, twelve terms reach 1e-26.
__device__ double deviance_term(double x, double e, double delta) {
    if (x == 0.0) return -delta;
    if (fabs(delta) < 0.1 * (x + e)) {
        const double v = delta / (x + e), w = v * v;
        double s = 0.0;
#pragma unroll
        for (int j = 23; j >= 5; j -= 2) s = (s + 1.0 / (double)j) * w;
        s = (s + 1.0 / 3.0) * w;
        return delta * v + 2.0 * x * v * s;
    }
    return x * log(x / e) - delta;
}
// All four cells are off their expectations by the same +-delta = (ad - bc) / M; the products come with their rounding
// errors (fma), so delta is good to ~3e-16 relative however close ad and bc are.  A real call: the kernels that use it
// are cold paths and keep their registers.
__device__ __noinline__ double log_pmf_beyond_table(double a, double b, double c, double d) {
    const double n1 = a + b, n2 = c + d, nn = a + c, mm = b + d, M = n1 + n2;
    const double ad = a * d, bc = b * c;
    const double det = (ad - bc) + (fma(a, d, -ad) - fma(b, c, -bc));
    const double delta = det / M;
    const double dev = deviance_term(a, n1 * nn / M, delta) + deviance_term(b, n1 * mm / M, -delta) +
                       deviance_term(c, n2 * nn / M, -delta) + deviance_term(d, n2 * mm / M, delta);
    const double rest = (stirling_rest(n1) + stirling_rest(n2) + stirling_rest(nn) + stirling_rest(mm)) - stirling_rest(M) -
                        (stirling_rest(a) + stirling_rest(b) + stirling_rest(c) + stirling_rest(d));
    return rest - dev;
}

// 1/y for y an integer-valued double in [1, 2^63): hardware seed + two Newton steps (no scaling or
// fix-up is ever needed in this range).  Accurate to ~1 ulp; the step ratios it feeds carry a
// relative error of a few 1e-16, against a tie slack of 1e-12 and a p-value tolerance of 1e-9.
// The IEEE division it replaces was ~2/3 of the instructions of a walk step.
__device__ __forceinline__ double rcp_pos(double y) {
    double x = __builtin_amdgcn_rcp(y);
    double e = fma(-y, x, 1.0);
    x = fma(x, e, x);
    e = fma(-y, x, 1.0);
    return fma(x, e, x);
}

// One-directional walk of the ratios r_k = pmf(k)/pmf(a) away from k = a.
//   up:   rho = (n1-k)(n-k) / ((k+1)(n2-n+k+1))        down: rho = k (n2-n+k) / ((n1-k+1)(n-k+1))
// Both are (u1 u2)/(v1 v2) with u falling and v rising by one per step, so one step routine serves both.
// No division per step: r_k = P_k/Q_k with P = prod(u1 u2), Q = prod(v1 v2), and the accepted ratios are
// summed over the common denominator, S_k = S_{k-1} (v1 v2) + [accepted] P_k, so the side's sum is S/Q --
// one reciprocal per p-value.  "Accepted" (pmf(k) <= pmf(a) (1 + 1e-12)) is P <= slack Q; the products carry
// a few 1e-16 of rounding per step.
// The step is BRANCH-FREE and needs no end test: N = u1 u2 and D = v1 v2 are quadratics in the step index,
// advanced by their first differences (N += dN, dN += 2).  They are DOUBLES: exact integers only while the products
// stay at or below 2^53, i.e. a d <= 2^53 and b c <= 2^53 for the table [[a, b], [c, d]] -- the host entry points
// refuse anything else (sd_check_pair_counts).  At the end of the support one of u1, u2 is zero, so N = 0 there, P = 0 from then on and further steps leave S/Q unchanged (both
// take the same factor D).  That needs N to be EXACT: a start product rounded to 53 bits drifts off the quadratic by
// up to an ulp per step and ends a few thousand off zero, with either sign; the steps past the end then add
// r_end * N_end / D and its successors to the sum -- a negative term is always "accepted" -- which for a table deep
// in a tail (r_end = pmf(end) / pmf(a) of 1e30) turns the sum into -1e30 or -inf.  (D only needs to be relatively
// accurate, and is.)  A lane may therefore run past its end, and a lane with nothing to do may step on
// stale state: the state machine issues steps for the whole wave without touching the exec mask
// (10 VALU per step -- 2 mul, 1 fma, 4 add, 1 compare, 2 select -- against 15 + ~10 scalar for the exec-masked step
// with the four factors kept separately).
// Scaling (exact powers of two), once per TRIP of at most 8 steps (a step multiplies P and Q by less than 2^62,
// a trip by less than 2^496): Q is brought back into [1, 2) with P and S; P, which outgrows Q while the walk
// crosses the mode, is kept below 2^500 by an exponent count eP (true P = P 2^(500 eP)).  eP > 0 is only left
// standing when P >= 2^-3, i.e. true P / Q > 2^496 at the start of a trip: such a lane cannot come back under
// Q within the trip, so "accepted" is (eP == 0 at the start of the trip) && P <= Q.
struct Walk {
    double N, dN, D, dD, P, Q, S, dN_end;
    int eP;
    // P carries a factor 1/slack, so that "accepted" is simply P <= Q; sum() puts it back
    static constexpr double SLACK = 1.0 + 1e-12, INV_SLACK = 1.0 / (1.0 + 1e-12);
    static constexpr int TRIP = 8;            // steps between two rescale() calls, at most
    __device__ __forceinline__ void side(double u1, double u2, double v1, double v2, double steps) {
        N = u1 * u2; dN = 1.0 - (u1 + u2);
        D = v1 * v2; dD = v1 + v2 + 1.0;
        dN_end = dN + 2.0 * steps;
    }
    __device__ __forceinline__ void start(double u1, double u2, double v1, double v2, double steps) {
        side(u1, u2, v1, v2, steps);
        P = INV_SLACK; Q = 1.0; S = 0.0; eP = 0;
    }
    // the walk on the other side of a continues on the same denominator: r = 1 again means P = Q / slack,
    // and S / Q ends as the sum over both sides
    __device__ __forceinline__ void turn(double u1, double u2, double v1, double v2, double steps) {
        side(u1, u2, v1, v2, steps);
        P = Q * INV_SLACK; eP = 0;
    }
    // ok: eP == 0 at the last rescale()
    __device__ __forceinline__ void step(bool ok) {
        P *= N; Q *= D;
        S = fma(S, D, (ok && P <= Q) ? P : 0.0);
        N += dN; dN += 2.0;
        D += dD; dD += 2.0;
    }
    __device__ __forceinline__ bool at_end() const { return dN >= dN_end; }
    // what remains of this side is below 1e-13 of the sum: the next ratio of ratios is below 1/2 and falls
    // from here on (the pmf is log-concave), so the rest is less than the last accepted term.  (1e-13 against a
    // p-value tolerance of 1e-9 -- north_star asks for 1e-6 --; the earlier 1e-18 bought nothing but ~10 % more steps:
    // a Gaussian-like tail needs ~1.4 sigma more to fall from 1e-13 to 1e-18 of the peak.)
    __device__ __forceinline__ bool tail_negligible() const {
        return eP == 0 && P <= Q && N + N < D && P < 1e-13 * (Q + S);
    }
    // may TRIP more steps be taken without rescale()?  A step multiplies P and Q by less than 2^62 (a trip: 2^496) and
    // S <= 2^31 Q: yes while Q and P are below 2^490 (2^490 * 2^496 * 2^31 < 2^1023) -- with counts in the thousands Q
    // grows by ~2^20 per step and the answer is yes; a lane with eP > 0 keeps its per-trip invariant only through
    // rescale().  Wave-uniform answer.
    __device__ __forceinline__ bool rescale_due() const {
        return __ballot(Q > 0x1p490 || P > 0x1p490 || eP != 0) != 0ull;
    }
    __device__ __forceinline__ void rescale() {
        // Q >= 1 (a normal number): back into [1, 2) by the power of two whose exponent field mirrors Q's -- three
        // full-rate multiplications (v_frexp_exp / v_ldexp_f64 are quarter-rate: the same scaling cost 20 issue slots)
        const unsigned ef = ((unsigned)__double2hiint(Q) >> 20) & 0x7ffu;
        const double sc = __hiloint2double((int)((2046u - ef) << 20), 0);
        Q *= sc; S *= sc; P *= sc;
        const bool up = P > 0x1p500, dn = eP > 0 && P < 0x1p-3;
        if (__ballot(up || dn) != 0ull) {                       // (wave-uniform: a ratio beyond 2^500 is a rare guest)
            P = __builtin_ldexp(P, up ? -500 : dn ? 500 : 0);
            eP += up ? 1 : dn ? -1 : 0;
        }
    }
    // slack S / Q, Q in [1, 2): hardware seed (~2^-23) + one Newton step -> ~1e-14, against a tolerance of 1e-9
    __device__ __forceinline__ double sum() const {
        double x = __builtin_amdgcn_rcp(Q);
        const double e = fma(-Q, x, 1.0);
        x = fma(x, e, x);
        return (S * SLACK) * x;
    }
    // walks this side to its end or until the rest is negligible
    __device__ __forceinline__ void run() {
        while (true) {
            const bool ok = eP == 0;
#pragma unroll
            for (int k = 0; k < TRIP; ++k) step(ok);
            rescale();
            if (at_end() || tail_negligible()) break;
        }
    }
};

__device__ double fisher_two_sided(long long a, long long b, long long c, long long d, const LfTable& t) {
    const long long n1 = a + b, n2 = c + d, n = a + c, m = b + d;
    if (n1 == 0 || n2 == 0 || n == 0 || m == 0) return 1.0;   // a zero margin (scipy: p = 1)
    const long long M = n1 + n2;
    const long long lo = n - n2 > 0 ? n - n2 : 0;
    const long long hi = n1 < n ? n1 : n;
    // (the same two evaluations, term for term, as pmf_block and fisher_beyond_table_kernel: the entry points agree
    // bit for bit on a table)
    const double* lf = t.lf;
    const double logp = M < t.n ? lf[n1] + lf[n2] + lf[n] + lf[m] - lf[M] - lf[a] - lf[b] - lf[c] - lf[d]
                                : log_pmf_beyond_table((double)a, (double)b, (double)c, (double)d);
    const double pexact = exp(logp);
    const double da = (double)a, dn1 = (double)n1, dn2 = (double)n2, dn = (double)n;
    Walk w;
    w.start(da, dn2 - dn + da, dn1 - da + 1.0, dn - da + 1.0, (double)(a - lo));                 // down from k = a
    if (a > lo) w.run();
    w.turn(dn1 - da, dn - da, da + 1.0, dn2 - dn + da + 1.0, (double)(hi - a));                    // up from k = a
    if (hi > a) w.run();
    const double total = 1.0 + w.sum();
    const double p = pexact * total;
    return p < 1.0 ? p : 1.0;
}

__global__ void __launch_bounds__(256) lf_table_kernel(double* __restrict__ lf, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lf[i] = lgamma((double)i + 1.0);
}

__global__ void __launch_bounds__(256) fisher_tables_kernel(const int64_t* __restrict__ abcd, int64_t m,
                                                            double* __restrict__ p, LfTable t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    p[i] = fisher_two_sided(abcd[4 * i], abcd[4 * i + 1], abcd[4 * i + 2], abcd[4 * i + 3], t);
}

// (i << 16 | j) of every pair index: the same for every junction, built once per call shape
__global__ void __launch_bounds__(256) pair_table_kernel(unsigned* __restrict__ tab, int64_t n_pairs, int s) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    int i, j;
    sd_pair_of(q, s, i, j);
    tab[q] = ((unsigned)i << 16) | (unsigned)j;
}

// p = pmf(a) * sum for the 256 pairs from q0 on, whose sums wait in the ring: the whole wave, four pairs per lane, the
// p-values leave as contiguous 512-byte pieces.  No call in here: a table whose total lies beyond the log-factorial table
// (counts above fisher.table_max, 2^20 by default) leaves MINUS its sum (sums are >= 1) and raises the junction's flag;
// fisher_beyond_table_kernel finishes those junctions.  (A call to lgamma -- even one, in a cold branch -- makes the
// register allocator keep the walk state in the 48 callee-saved VGPRs and spill the rest inside the loop; a pmf pass in
// a function of its own saved and restored 112 bytes per lane per call: 14 GB of scratch traffic per launch.)
extern __shared__ double smd[];
__device__ __forceinline__ bool pmf_block(int s, double* __restrict__ out, const unsigned* __restrict__ pair_tab, LfTable tab,
                                          int q0, int n_pairs, int lane) {
    const double* inc = smd;
    const double* exc = smd + s;
    const double* ring = smd + 2 * s;
    bool beyond = false;
#pragma nounroll
    for (int t = 0; t < 4; ++t) {
        const int q = q0 + t * 64 + lane;
        if (q < n_pairs) {
            const double total = ring[q & 511];
            const unsigned ij = pair_tab[q];
            int i, j;
            sd_pair_unpack(ij, i, j);
            const double a = inc[i], b = inc[j], c = exc[i], d = exc[j];
            const double n1 = a + b, n2 = c + d, nn = a + c, mm = b + d, M = n1 + n2;
            double pv = 1.0;                                           // a zero margin (scipy: p = 1)
            if (n1 != 0.0 && n2 != 0.0 && nn != 0.0 && mm != 0.0) {
                if (M < (double)tab.n) {                               // (the largest of the nine arguments)
                    const double* lf = tab.lf;
                    const double logp = lf[(int)n1] + lf[(int)n2] + lf[(int)nn] + lf[(int)mm] - lf[(int)M] - lf[(int)a] -
                                        lf[(int)b] - lf[(int)c] - lf[(int)d];
                    pv = exp(logp) * total;
                    pv = pv < 1.0 ? pv : 1.0;
                } else {
                    pv = -total;
                    beyond = true;
                }
            }
            out[q] = pv;
        }
    }
    return beyond;
}

// the junctions flagged by the pair kernel: p = pmf(a) * sum, pmf(a) by log_pmf_beyond_table, for the pairs that carry a
// negative sum
__global__ void __launch_bounds__(256) fisher_beyond_table_kernel(const int32_t* __restrict__ incl, const int64_t* __restrict__ excl,
                                                                  int64_t n, int s, int64_t n_pairs, double* __restrict__ p,
                                                                  const unsigned* __restrict__ pair_tab,
                                                                  const unsigned char* __restrict__ row_flag) {
    const int64_t row = blockIdx.x;
    if (row >= n || !row_flag[row]) return;
    double* out = p + row * n_pairs;
    for (int64_t q = threadIdx.x; q < n_pairs; q += 256) {
        const double v = out[q];
        if (v < 0.0) {
            const unsigned ij = pair_tab[q];
            int i, j;
            sd_pair_unpack(ij, i, j);
            const double a = (double)incl[row * s + i], b = (double)incl[row * s + j];
            const double c = (double)excl[row * s + i], d = (double)excl[row * s + j];
            const double pv = exp(log_pmf_beyond_table(a, b, c, d)) * -v;
            out[q] = pv < 1.0 ? pv : 1.0;
        }
    }
}

// One WAVE per junction.  The walk lengths of the pairs of one junction differ by an order of magnitude (they follow the
// margins), and a loop "for each pair: walk" keeps a wave at the pace of its slowest lane: 27 of 64 lanes were active on
// average.  Here every lane is a small state machine -- idle / walking down / walking up -- and the wave issues walk steps
// for all lanes (see Walk).  Pairs are handed out IN ORDER: when `refill` lanes are idle they take the next pairs q = next,
// next + 1, ... (a lane's rank among the idle lanes picks its pair; the (i, j) of the next 128 pairs wait in two registers
// across the wave and come by a lane shuffle), so the lanes finish a junction within one pair of each other and the pairs
// in flight are a window of ~100 consecutive indices.  Finished sums go to a ring of 512 slots in LDS; as soon as a block
// of 256 consecutive pairs is complete, the whole wave applies pmf(a) -- nine log-factorial look-ups and an exp, all lanes
// busy -- and writes the 256 p-values as four contiguous 512-byte pieces.  A p-value is written exactly once and nothing
// is read back (the version with a statically assigned run of 8 pairs per lane wrote the sums, read them again for the
// pmf pass and wrote the p-values: 12.9 GB of HBM traffic for 4 GB of results).
// The pairs are the n_pairs entries of pair_tab, column q of the output being the pair pair_tab[q] = i << 16 | j: every
// pair in row-major order (pair_table_kernel) or a caller's list (sdice_pair_list_pack_dev) -- any order, i > j and
// repeats included.  Window, ring and blocks are indexed by q alone.
template <int UNROLL, bool COUNT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8)))
fisher_pairs_kernel(const int32_t* __restrict__ incl, const int64_t* __restrict__ excl, int64_t n, int s, int n_pairs,
                    double* __restrict__ p, LfTable tab, const unsigned* __restrict__ pair_tab, int refill,
                    unsigned long long* __restrict__ row_counter, unsigned char* __restrict__ row_flag) {
    // counts staged as doubles (exact below 2^53): the set-up of a pair is four LDS reads and a dozen f64 operations
    double* inc = smd;
    double* exc = smd + s;
    double* ring = smd + 2 * s;                                        // [512] finished sums, slot = q mod 512
    const int lane = threadIdx.x;
    // (n_pairs: at most SD_MAX_PAIRS, fewer than 2^25)
    const int n_blk = (n_pairs + 255) >> 8;
    static_assert(UNROLL >= 1 && UNROLL <= 24, "unroll");
    // COUNT (fisher.count_steps, a measurement build): lane-steps issued and lane-steps that advanced a live walk
    // inside its support -- row_counter[1], [2]
    unsigned long long n_useful = 0, n_trips = 0;
    while (true) {
        // junctions are handed out one at a time: the grid is the set of resident waves, and a wave that
        // drew cheap junctions takes more of them
        unsigned long long row_u = 0;
        if (lane == 0) row_u = atomicAdd(row_counter, 1ull);
        const int64_t row = (int64_t)__shfl((long long)row_u, 0);
        if (row >= n) break;
        __syncthreads();
        for (int k = lane; k < s; k += 64) {
            inc[k] = (double)incl[row * s + k];
            exc[k] = (double)excl[row * s + k];
        }
        __syncthreads();
        double* out = p + row * (int64_t)n_pairs;

        int next = 0, fin_blk = 0;             // wave-uniform: next pair to hand out, next block for the pmf pass
        int done0 = 0, done1 = 0;              // wave-uniform: finished pairs of the even / odd block in the ring
        int tab_base = 0;                      // pair_tab[tab_base + lane] / [tab_base + 64 + lane] sit in tab_cur / tab_nxt
        unsigned tab_cur = lane < n_pairs ? pair_tab[lane] : 0u;
        unsigned tab_nxt = 64 + lane < n_pairs ? pair_tab[64 + lane] : 0u;
        int phase = 0, q_cur = 0;              // 0 idle, 1 walking down from a, 2 walking up from a
        Walk w;
        w.start(1.0, 1.0, 1.0, 1.0, 0.0);
        // the table [[a, b], [c, d]] of the current pair: down from k = a the ratio is a d / ((b + 1)(c + 1)) over
        // min(a, d) steps, up it is b c / ((a + 1)(d + 1)) over min(b, c) steps.  A zero margin leaves no step on
        // either side (the sum comes out as 1 and the pmf pass sets p = 1, as scipy does).
        double ta = 0.0, tb = 0.0, tc = 0.0, td = 0.0;
        while (true) {
            // ---- p = pmf(a) * sum for a complete block of 256 pairs, all lanes busy
            if (fin_blk < n_blk) {
                const int need = min(256, n_pairs - (fin_blk << 8));
                if (((fin_blk & 1) ? done1 : done0) == need) {
                    if (__ballot(pmf_block(s, out, pair_tab, tab, fin_blk << 8, n_pairs, lane)) != 0ull && lane == 0) row_flag[row] = 1;
                    if (fin_blk & 1) done1 = 0; else done0 = 0;
                    fin_blk += 1;
                }
            }
            // ---- hand out pairs (the ring holds the two blocks from fin_blk on)
            const unsigned long long idle_m = __ballot(phase == 0);
            const int lim = min(n_pairs, (fin_blk + 2) << 8);
            if (idle_m == ~0ull && next >= n_pairs && fin_blk >= n_blk) break;
            const int n_idle = __popcll(idle_m);
            if ((n_idle >= refill || idle_m == ~0ull) && next < lim) {
                const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(idle_m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle_m, 0u));
                const int q = next + r;
                const int dq = q - tab_base;                              // < 128 for a lane that takes a pair
                const unsigned e0 = (unsigned)__shfl((int)tab_cur, dq & 63), e1 = (unsigned)__shfl((int)tab_nxt, dq & 63);
                if (phase == 0 && q < lim) {
                    const unsigned ij = dq < 64 ? e0 : e1;
                    int i, j;
                    sd_pair_unpack(ij, i, j);
                    ta = inc[i]; tb = inc[j]; tc = exc[i]; td = exc[j];
                    q_cur = q;
                    w.start(ta, td, tb + 1.0, tc + 1.0, ta < td ? ta : td);   // down from k = a (possibly no step at all)
                    phase = 1;
                }
                next = min(next + n_idle, lim);
                if (next >= tab_base + 64) {
                    tab_base += 64;
                    tab_cur = tab_nxt;
                    tab_nxt = tab_base + 64 + lane < n_pairs ? pair_tab[tab_base + 64 + lane] : 0u;
                }
            }
            // ---- one trip: every lane steps, whatever its phase (see Walk); the exec mask is not touched
            if (COUNT) {
                const double left = (w.dN_end - w.dN) * 0.5;
                if (phase != 0 && left > 0.0) n_useful += (unsigned long long)(left < (double)UNROLL ? left : (double)UNROLL);
                n_trips += 1;
            }
            bool ok = w.eP == 0;
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                w.step(ok);
                // between the halves of a long trip the scaling is only due when some lane's products have left the first
                // half of the exponent range (wave-uniform test: 3 instructions instead of ~14)
                if (k % Walk::TRIP == Walk::TRIP - 1 && k + 1 < UNROLL && w.rescale_due()) { w.rescale(); ok = w.eP == 0; }
            }
            w.rescale();
            const bool fin = phase != 0 && (w.at_end() || w.tail_negligible());
            const double up_steps = tb < tc ? tb : tc;
            const bool dep = fin && !(phase == 1 && up_steps > 0.0);
            const unsigned long long dep1 = __ballot(dep && (q_cur & 256) != 0), dep_m = __ballot(dep);
            done1 += __popcll(dep1);
            done0 += __popcll(dep_m) - __popcll(dep1);
            if (fin) {
                if (!dep) {
                    w.turn(tb, tc, ta + 1.0, td + 1.0, up_steps);                                   // up from k = a
                    phase = 2;
                } else {
                    ring[q_cur & 511] = 1.0 + w.sum();
                    phase = 0;
                }
            }
        }
    }
    if (COUNT) {
        atomicAdd(row_counter + 1, n_useful);
        if (lane == 0) atomicAdd(row_counter + 2, n_trips * (unsigned long long)(UNROLL * 64));
    }
}

}  // namespace

// log-factorial table owned by the context (built on first use)
static int get_lf_table(sdice_ctx* ctx, LfTable* out) {
    long long want = ctx->param(SD_P_FISHER_TABLE_MAX);
    if (want < 2) want = 2;
    if (ctx->d_lf && ctx->lf_n == want) {
        out->lf = ctx->d_lf;
        out->n = want;
        return SDICE_OK;
    }
    if (ctx->d_lf) {
        SD_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->d_lf);
        ctx->d_lf = nullptr;
        ctx->lf_n = 0;
    }
    double* lf = nullptr;
    hipError_t e = hipMalloc((void**)&lf, (size_t)want * 8);
    if (e != hipSuccess) {
        sdice_set_error("fisher: hipMalloc of log-factorial table failed: %s", hipGetErrorString(e));
        return SDICE_ERR_NOMEM;
    }
    SD_LAUNCH(ctx, "lf_table_kernel", lf_table_kernel, dim3((unsigned)sd_ceil_div(want, 256)), dim3(256), 0, lf, want);
    ctx->d_lf = lf;
    ctx->lf_n = want;
    out->lf = lf;
    out->n = want;
    return SDICE_OK;
}

// The pair kernel and its second pass over n junctions and the n_pairs columns of a pair table: d_list, a caller's
// packed list, or (d_list == NULL) every pair in row-major order, built here.
static int fisher_launch(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                         int64_t n_pairs, const uint32_t* d_list, double* d_p) {
    SD_HIP(hipSetDevice(ctx->device));
    LfTable t;
    SD_TRY(get_lf_table(ctx, &t));
    int refill = (int)ctx->param(SD_P_FISHER_REFILL);
    if (refill < 1) refill = 1;
    if (refill > 64) refill = 64;
    // steps per trip: 16 (153 VGPRs, three waves per SIMD, nothing spilled) 16.0 ms per 25 000 x 19 900; 8 (114 VGPRs, four
    // waves) 16.6 ms; 16 under a 128-VGPR cap spills 100 bytes inside the loop: 18.5 ms; under 96 (five waves): 34-43 ms
    const int unroll = (int)ctx->param(SD_P_FISHER_UNROLL);
    SD_TRY(ctx->arena.reserve((d_list ? 0 : (size_t)n_pairs * 4) + (size_t)n + 8192, ctx->stream));
    const unsigned* pair_tab = d_list;
    if (!d_list) {
        unsigned* built = (unsigned*)ctx->arena.alloc((size_t)n_pairs * 4);
        if (!built) return SDICE_ERR_NOMEM;
        pair_tab = built;
    }
    unsigned long long* row_counter = (unsigned long long*)ctx->arena.alloc(24);     // + the two step counters
    unsigned char* row_flag = (unsigned char*)ctx->arena.alloc((size_t)n);
    if (!row_counter || !row_flag) return SDICE_ERR_NOMEM;
    SD_HIP(hipMemsetAsync(row_counter, 0, 24, ctx->stream));
    SD_HIP(hipMemsetAsync(row_flag, 0, (size_t)n, ctx->stream));
    if (!d_list)
        SD_LAUNCH(ctx, "pair_table_kernel", pair_table_kernel, dim3((unsigned)sd_ceil_div(n_pairs, (int64_t)256)), dim3(256), 0,
                  const_cast<unsigned*>(pair_tab), n_pairs, (int)s);
    const size_t lds = (size_t)s * 16 + 512 * 8;
    const bool count = ctx->param(SD_P_FISHER_COUNT_STEPS) != 0;
    auto kern = count ? (unroll <= 4 ? fisher_pairs_kernel<4, true> : unroll <= 8 ? fisher_pairs_kernel<8, true> :
                         unroll <= 12 ? fisher_pairs_kernel<12, true> : unroll <= 16 ? fisher_pairs_kernel<16, true> :
                         unroll <= 20 ? fisher_pairs_kernel<20, true> : fisher_pairs_kernel<24, true>)
                      : (unroll <= 4 ? fisher_pairs_kernel<4, false> : unroll <= 8 ? fisher_pairs_kernel<8, false> :
                         unroll <= 12 ? fisher_pairs_kernel<12, false> : unroll <= 16 ? fisher_pairs_kernel<16, false> :
                         unroll <= 20 ? fisher_pairs_kernel<20, false> : fisher_pairs_kernel<24, false>);
    SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    SD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), 64, lds));
    if (per_cu < 1) per_cu = 1;
    int64_t blocks = std::min<int64_t>(n, (int64_t)ctx->n_cu * per_cu);     // the resident waves; junctions by counter
    SD_LAUNCH(ctx, "fisher_pairs_kernel", kern, dim3((unsigned)blocks), dim3(64), lds, d_incl, d_excl, n, (int)s, (int)n_pairs,
              d_p, t, pair_tab, refill, row_counter, row_flag);
    // junctions with a table beyond the log-factorial table (their workgroups return at once otherwise)
    SD_LAUNCH(ctx, "fisher_beyond_table_kernel", fisher_beyond_table_kernel, dim3((unsigned)n), dim3(256), 0, d_incl, d_excl, n,
              (int)s, n_pairs, d_p, pair_tab, row_flag);
    if (count) {
        SD_HIP(hipMemcpyAsync(ctx->fisher_steps, row_counter + 1, 16, hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SDICE_OK;
}

// the launch of a checked call (pairs.h)
static int fisher_call(const PairCall& c) {
    return fisher_launch(c.ctx, c.n, c.s, c.incl, c.excl, c.cols(), static_cast<const uint32_t*>(c.tab), c.p);
}

extern "C" int sdice_fisher_pairs_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl,
                                      const int64_t* d_excl, double* d_p) {
    return sd_pairs_dev({__func__, ctx, n, s, d_incl, d_excl, false, 0, nullptr, d_p, false, nullptr}, fisher_call);
}

extern "C" int sdice_fisher_pair_list_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                                          int64_t m, const uint32_t* d_tab, double* d_p) {
    return sd_pairs_dev({__func__, ctx, n, s, d_incl, d_excl, true, m, d_tab, d_p, false, nullptr}, fisher_call);
}

extern "C" int sdice_fisher_step_stats(sdice_ctx* ctx, uint64_t* useful, uint64_t* issued) {
    SD_ARG(ctx && useful && issued, "NULL pointer");
    *useful = ctx->fisher_steps[0];
    *issued = ctx->fisher_steps[1];
    return SDICE_OK;
}

extern "C" int sdice_fisher_pairs(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl,
                                  double* p) {
    return sd_pairs_host({__func__, ctx, n, s, incl, excl, false, 0, nullptr, p, false, nullptr}, fisher_call);
}

extern "C" int sdice_fisher_pair_list(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl,
                                      int64_t m, const int32_t* pairs, double* p) {
    return sd_pairs_host({__func__, ctx, n, s, incl, excl, true, m, pairs, p, false, nullptr}, fisher_call);
}

// the pair table of a caller's list, as pair_table_kernel builds it for every pair
extern "C" int sdice_pair_list_pack_dev(sdice_ctx* ctx, int32_t s, int64_t m, const int32_t* pairs, uint32_t* d_tab) {
    const char* who = __func__;
    return sd_no_throw(who, [&]() -> int {
        SD_ARG_AS(who, ctx, "ctx is NULL");
        SD_ARG_AS(who, s >= 0 && m >= 0, "negative size");
        SD_TRY(sd_pair_limits(who, s, m));
        if (m == 0) return SDICE_OK;
        SD_ARG_AS(who, pairs && d_tab, "NULL pointer");
        SD_TRY(sd_check_pair_list(who, s, m, pairs));
        return sd_pair_tab_upload(ctx, m, pairs, d_tab);
    });
}

extern "C" int sdice_fisher_tables(sdice_ctx* ctx, int64_t m, const int64_t* abcd, double* p) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(m >= 0, "negative size");
    if (m == 0) return SDICE_OK;
    SD_ARG(abcd && p, "NULL pointer");
    SD_TRY(sd_check_tables(__func__, m, abcd));
    SD_HIP(hipSetDevice(ctx->device));
    LfTable t;
    SD_TRY(get_lf_table(ctx, &t));
    HostStaging st(ctx);
    int64_t* dt;
    double* dp;
    SD_TRY(st.upload(&dt, abcd, 4 * m));
    SD_TRY(st.alloc(&dp, m));
    SD_LAUNCH(ctx, "fisher_tables_kernel", fisher_tables_kernel, dim3((unsigned)sd_ceil_div(m, 256)), dim3(256), 0, dt, m,
              dp, t);
    return st.download(p, dp, m);
}
