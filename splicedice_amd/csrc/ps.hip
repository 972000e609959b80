// K3: exclusion-sum + PS over the junction x sample matrix, K4: '.3f' quantise,
// and the --lowCoverageNan scatter.
//
// Replaces SPLICEDICE.calculatePsi (SPLICEDICE.py:297-310): for every junction row the
// reference adds up the count rows of all overlapping junctions (float64 accumulation of
// integer-valued float32 counts -> exact integer sums) and stores
// float32(float64(incl) / float64(incl + excl)).
//
// Design (HBM-bound, 8 algorithmic bytes per PS entry: 4 B count in + 4 B PS out):
//   * one workgroup owns a tile of consecutive output rows x a chunk of columns (all columns
//     up to 256 samples, 128-column chunks above); the chunks of one row tile are dispatched
//     back to back on ONE XCD -- with chunks spread over XCDs and time the cache lines straddling
//     a chunk boundary left L2 as two masked partial writes and the store stream ran at 1.5 TB/s
//     (2M x 500: 2.72 ms -> 1.85 ms with this mapping alone);
//   * it stages the rows [r0 - halo, r1 + halo) of the count matrix into LDS with one
//     coalesced 16 B/lane copy that depends on nothing but the tile index, so every load
//     of the tile is in flight at once (overlap clusters are gene sized: the neighbours of
//     a row lie a few rows away in (chrom,left,right,strand) order);
//   * meanwhile the tile's CSR segment is read and turned into LDS byte offsets of the
//     neighbour rows (or a sentinel for a neighbour outside the staged window);
//   * every (row, 4-column) item then gathers its neighbour rows from LDS with
//     ds_read_b128 and stores a float4 -- each count is read from HBM once per tile
//     (+halo, which is an L2 hit) and each PS value is written once;
//   * a neighbour outside the window (arbitrary user CSR, unusually long junction) is read
//     from global memory instead, so ANY valid CSR gives exact results; the halo only
//     decides how often that slower path runs.
// Arithmetic: sums are exact integers.  When a tile's bound (max count) * (max degree + 1)
// is below 2^24, sums are kept in 32 bits and the quotient is one IEEE float32 division:
// both operands are then exact float32 values and a correctly rounded float32 quotient of
// two such integers equals float32(float64 quotient) (a double rounding could only differ
// if the exact quotient were within 2^-53 of a float32 midpoint, impossible for a
// denominator below 2^24).  Otherwise 64-bit sums and the float64 division are used.
#include "common.h"
#include "ps.h"
#include <algorithm>
#include <type_traits>

namespace {

struct PsArgs {
    const int32_t* counts;
    const int64_t* row_ptr;
    const int32_t* col;
    int64_t* excl;
    float* ps;
    int64_t n;
    int s;
    int tile_rows;   // output rows per tile
    int halo;        // extra rows staged on each side of the tile
    int chunk_cols;  // columns per chunk == LDS row stride (multiple of VEC)
    int col_cap;     // LDS capacity for staged neighbour offsets (ints)
    int n_tiles;
    int tiles_per_xcd;  // 0 = no remap
    int n_chunks;       // column chunks per row tile
    int prio;           // raise the wave priority while the window loads go out (param ps.prio, default 1)
    int nt;             // non-temporal window loads (param ps.nt_loads, default 1; unchunked tables only)
    // second-generation kernel only:
    const uint32_t* reach;  // reach words of the lists per block of 16 rows (below | beyond << 8, 255 = that far or further), NULL: stage `halo` rows
    int lv_shift;       // column chunks: 6 - log2(vectors per row segment) (chunk_cols / 4 divides 64)
};

__device__ __forceinline__ int4 nt_load(const int4* p) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int nt_load(const int* p) { return __builtin_nontemporal_load(p); }

template <int VEC> struct Vt;
template <> struct Vt<4> { typedef int4 I; };
template <> struct Vt<1> { typedef int I; };

__device__ __forceinline__ float ps_value64(unsigned incl, unsigned long long excl) {
    // float32(float64(incl) / float64(incl + excl)), SPLICEDICE.py:306; 0/0 -> NaN
    const double a = (double)incl;
    const double t = a + (double)excl;
    return (float)(a / t);
}

__device__ __forceinline__ unsigned vmax(const int4& v) {
    return max(max((unsigned)v.x, (unsigned)v.y), max((unsigned)v.z, (unsigned)v.w));
}
__device__ __forceinline__ unsigned vmax(const int& v) { return (unsigned)v; }

template <typename ACC> __device__ __forceinline__ void acc_add(ACC (&acc)[4], const int4& v) {
    acc[0] += (unsigned)v.x; acc[1] += (unsigned)v.y; acc[2] += (unsigned)v.z; acc[3] += (unsigned)v.w;
}
template <typename ACC> __device__ __forceinline__ void acc_add(ACC (&acc)[1], const int& v) { acc[0] += (unsigned)v; }

__device__ __forceinline__ unsigned comp(const int4& v, int q) { return (unsigned)(q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w); }
__device__ __forceinline__ unsigned comp(const int& v, int) { return (unsigned)v; }

template <int VEC> __device__ __forceinline__ void store_f(float* p, const float (&o)[VEC]);
template <> __device__ __forceinline__ void store_f<4>(float* p, const float (&o)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
}
template <> __device__ __forceinline__ void store_f<1>(float* p, const float (&o)[1]) { *p = o[0]; }
__device__ __forceinline__ void store_f4_nt(float* p, const float (&o)[4]) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v = {o[0], o[1], o[2], o[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
}

template <int VEC, typename ACC> __device__ __forceinline__ void store_excl(int64_t* p, const ACC (&acc)[VEC]) {
    if (VEC == 4) {
        longlong2 a, b;
        a.x = (long long)acc[0]; a.y = (long long)acc[1]; b.x = (long long)acc[VEC - 2]; b.y = (long long)acc[VEC - 1];
        reinterpret_cast<longlong2*>(p)[0] = a;
        reinterpret_cast<longlong2*>(p)[1] = b;
    } else {
        *p = (int64_t)acc[0];
    }
}

__device__ __forceinline__ float div_small_ints(float a, float t) {
    // a / t for exact integers 0 <= a <= t < 2^24: the Newton / residual steps of the IEEE
    // float32 division sequence without v_div_scale / v_div_fixup (no scaling is ever needed in
    // this range), hence the same correctly rounded quotient in 8 instead of 13 instructions.
    // t == 0 (then a == 0): rcp = inf, e = NaN -> NaN, as 0/0.
    float r = __builtin_amdgcn_rcpf(t);
    const float e = __builtin_fmaf(-t, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    float q = a * r;
    float rem = __builtin_fmaf(-t, q, a);
    q = __builtin_fmaf(rem, r, q);
    rem = __builtin_fmaf(-t, q, a);
    return __builtin_fmaf(rem, r, q);
}

// The same sequence on two quotients at once: v_pk_fma_f32 / v_pk_mul_f32 carry two float32 lanes
// per instruction (the reciprocal seed has no packed form).
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f div_small_ints2(v2f a, v2f t) {
    v2f r;
    r.x = __builtin_amdgcn_rcpf(t.x); r.y = __builtin_amdgcn_rcpf(t.y);
    const v2f one = {1.0f, 1.0f};
    const v2f e = __builtin_elementwise_fma(-t, r, one);
    r = __builtin_elementwise_fma(e, r, r);
    v2f q = a * r;
    v2f rem = __builtin_elementwise_fma(-t, q, a);
    q = __builtin_elementwise_fma(rem, r, q);
    rem = __builtin_elementwise_fma(-t, q, a);
    return __builtin_elementwise_fma(rem, r, q);
}

// k = round-half-even(x * 1000) for a float32 x in [0, 1] (NaN stays NaN), as the decimal formatter of '%.3f' rounds the
// EXACT value of x -- without float64 (v_cvt_f64_f32, v_rndne_f64, v_cvt_f32_f64 are quarter-rate: 13 issue slots per
// value): p = fl(x * 1000) and e = fma(x, 1000, -p) give the exact product p + e (|e| <= ulp(p) / 2 <= 2^-15); k0 =
// rint(p) is the answer unless p sits exactly on a half integer and e is not zero -- then the true value lies on e's
// side of it.  (|p - k0| < 1/2 implies |p - k0| <= 1/2 - ulp(p), so e cannot carry the sum across a half integer.)
__device__ __forceinline__ v2f thousandths2(v2f x) {
    const v2f th = {1000.0f, 1000.0f};
    const v2f p = x * th;
    const v2f e = __builtin_elementwise_fma(x, th, -p);
    v2f k0, k;
    k0.x = __builtin_rintf(p.x); k0.y = __builtin_rintf(p.y);
    const v2f r = p - k0;
    k.x = (__builtin_fabsf(r.x) == 0.5f && e.x != 0.0f) ? p.x + __builtin_copysignf(0.5f, e.x) : k0.x;
    k.y = (__builtin_fabsf(r.y) == 0.5f && e.y != 0.0f) ? p.y + __builtin_copysignf(0.5f, e.y) : k0.y;
    return k;
}
// float32(k / 1000.0) for an integer-valued k in [0, 1000]: k * 0.001f and one residual step give the correctly rounded
// quotient for all 1001 keys (exhaustive test in rational arithmetic: test_ps_of_key_formula_reproduces_the_table)
__device__ __forceinline__ v2f key_over_1000(v2f k) {
    const v2f m = {0.001f, 0.001f}, th = {1000.0f, 1000.0f};
    const v2f q = k * m;
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-q, th, k), m, q);
}

// LDS offsets of a batch of GB neighbours of an item, k .. k + GB - 1 of the tile's offset stage; a short last batch is
// padded with the all-zero row kept behind the window.  Unconditional reads (a short last batch runs into the next
// row's entries or the words behind the stage -- always inside the LDS allocation) and a select: predicated reads
// compile to an exec-mask round trip per element.  CHECK: false = one of them is outside the window (a tile whose
// staged neighbours all lie inside it skips the test)
template <bool CHECK, int GB>
__device__ __forceinline__ bool ps_batch_offsets(const int* colL, int k, int k1, int zero_off, int (&off)[GB]) {
    int raw[GB];
#pragma unroll
    for (int u = 0; u < GB; ++u) raw[u] = colL[k + u];
#pragma unroll
    for (int u = 0; u < GB; ++u) off[u] = (k + u < k1) ? raw[u] : zero_off;
    if (CHECK) {
        int mn = off[0];
#pragma unroll
        for (int u = 1; u < GB; ++u) mn = min(mn, off[u]);
        if (mn < 0) return false;
    }
    return true;
}

// PS of the four columns of an item whose totals are below 2^24: two packed float32 quotients per instruction
template <bool Q3>
__device__ __forceinline__ void ps_quotients32(const unsigned (&in)[4], const unsigned (&acc)[4], float (&o)[4]) {
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
        const v2f num = {(float)in[q], (float)in[q + 1]};
        const v2f den = {(float)(in[q] + acc[q]), (float)(in[q + 1] + acc[q + 1])};
        v2f ps2 = div_small_ints2(num, den);
        if (Q3) ps2 = key_over_1000(thousandths2(ps2));     // fused K4: float32(f'{ps:.3f}')
        o[q] = ps2.x; o[q + 1] = ps2.y;
    }
}

// quotients and stores of a four-column item with 32-bit sums.  Non-temporal store: the PS matrix is written once and
// not re-read by this kernel, keeping it out of the L2 leaves the halo rows of the count matrix there (-2.5 % at 1M x 100)
template <bool WEXCL, bool WPS, bool Q3>
__device__ __forceinline__ void ps_finish32(const PsArgs& a, const unsigned (&in)[4], const unsigned (&acc)[4], int64_t out_index) {
    if (WPS) {
        float o[4];
        ps_quotients32<Q3>(in, acc, o);
        store_f4_nt(a.ps + out_index, o);
    }
    if (WEXCL) store_excl<4, unsigned>(a.excl + out_index, acc);
}

// quotients and stores of an item with 64-bit sums: float64 division, exact for any counts (ABL 4 = no PS store)
template <int VEC, bool WEXCL, bool WPS, bool Q3, int ABL>
__device__ __forceinline__ void ps_finish64(const PsArgs& a, const typename Vt<VEC>::I& own, const unsigned long long (&acc)[VEC],
                                            int64_t out_index) {
    if (WPS) {
        float o[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            o[q] = ps_value64(comp(own, q), acc[q]);
            if (Q3) o[q] = (float)(rint((double)o[q] * 1000.0) / 1000.0);
        }
        if (!(ABL & 4)) store_f<VEC>(a.ps + out_index, o);
    }
    if (WEXCL) store_excl<VEC, unsigned long long>(a.excl + out_index, acc);
}

// Fast item: every neighbour offset comes from the LDS stage and lies inside the staged window,
// the tile's bound keeps incl + excl < 2^24 -> 32-bit sums, float32 quotient.  Returns false
// (nothing stored) as soon as a neighbour is outside the window; the caller then runs ps_item_slow.
template <int VEC, bool WEXCL, bool WPS, bool CHECK, bool Q3, int ABL>
__device__ __forceinline__ bool ps_item_fast(const PsArgs& a, const char* tileB, const int* colL, int k0, int k1,
                                             int cbytes, int own_off, int64_t out_index, int zero_off) {
    typedef typename Vt<VEC>::I VI;
    unsigned acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0;
    // batches of GB neighbours: all offset reads, then all row reads, then the adds -- two LDS
    // round trips per batch instead of two per neighbour
    constexpr int GB = 4;
    for (int k = k0; k < k1; k += GB) {
        int off[GB];
        if (!ps_batch_offsets<CHECK, GB>(colL, k, k1, zero_off, off)) return false;
        VI v[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) v[u] = *reinterpret_cast<const VI*>(tileB + off[u] + cbytes);
#pragma unroll
        for (int u = 0; u < GB; ++u) acc_add(acc, v[u]);
    }
    const VI own = *reinterpret_cast<const VI*>(tileB + own_off + cbytes);
    if constexpr (VEC == 4 && ABL == 0) {
        const unsigned in[4] = {comp(own, 0), comp(own, 1), comp(own, 2), comp(own, 3)};
        ps_finish32<WEXCL, WPS, Q3>(a, in, acc, out_index);
    } else {
        if (WPS) {
            float o[VEC];
            if constexpr (VEC == 4) {
                const unsigned in[4] = {comp(own, 0), comp(own, 1), comp(own, 2), comp(own, 3)};
                ps_quotients32<Q3>(in, acc, o);
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    const unsigned in = comp(own, q);
                    o[q] = div_small_ints((float)in, (float)(in + acc[q]));
                    if (Q3) o[q] = div_small_ints((float)rint((double)o[q] * 1000.0), 1000.0f);
                }
            }
            // (ABL 8 = plain store where the production kernel stores non-temporally, ABL 4 = none)
            if (VEC == 4 && !(ABL & 8)) { if (!(ABL & 4)) store_f4_nt(a.ps + out_index, reinterpret_cast<const float (&)[4]>(o)); }
            else if (!(ABL & 4)) store_f<VEC>(a.ps + out_index, o);
        }
        if (WEXCL) store_excl<VEC, unsigned>(a.excl + out_index, acc);
    }
    return true;
}

// General item: neighbours from the LDS window or from global memory, indices from the LDS stage
// or from global memory, 64-bit sums, float64 division.  Exact for any valid CSR and any counts.
template <int VEC, bool WEXCL, bool WPS, bool Q3, int ABL>
__device__ __forceinline__ void ps_item_slow(const PsArgs& a, const char* tileB, const int* colL, bool col_in_lds,
                                             int64_t kbase, int k0, int k1, int slo, int wrows, int ldw, int c0, int cvec,
                                             int own_off, int64_t out_index, int wbase) {
    typedef typename Vt<VEC>::I VI;
    unsigned long long acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0;
    const int cbytes = cvec * 4;
    for (int k = k0; k < k1; ++k) {
        int off;
        if (col_in_lds) {
            off = colL[k];
        } else {
            const int j = a.nt ? __builtin_nontemporal_load(a.col + kbase + k) : a.col[kbase + k];
            const unsigned rel = (unsigned)(j - slo);
            off = rel < (unsigned)wrows ? (int)((unsigned)(j - wbase) * (unsigned)ldw * 4u) : -1 - j;
        }
        VI v;
        if (off >= 0) v = *reinterpret_cast<const VI*>(tileB + off + cbytes);
        else v = *reinterpret_cast<const VI*>(a.counts + (int64_t)(-1 - off) * a.s + c0 + cvec);
        acc_add(acc, v);
    }
    const VI own = *reinterpret_cast<const VI*>(tileB + own_off + cbytes);
    ps_finish64<VEC, WEXCL, WPS, Q3, ABL>(a, own, acc, out_index);
}

// workgroup id -> (row tile, column chunk) of a column-chunked launch.  1-D grid: the column chunks of one row tile are
// CONSECUTIVE work on ONE XCD, so the cache lines that two chunks share at a chunk boundary (rows are not 128 B aligned
// when 4*s is not) meet in that XCD's L2 and leave it as full lines instead of two masked partial writes.  With
// tiles_per_xcd (blocks are dealt round-robin over the 8 XCDs) each XCD gets a contiguous run of tiles, so that
// neighbouring tiles (which share halo rows) share one L2; the caller drops a workgroup whose tile >= n_tiles
__device__ __forceinline__ void ps_tile_of_block(const PsArgs& a, int bid, int& tile, int& chunk) {
    tile = bid / a.n_chunks;
    chunk = bid - tile * a.n_chunks;
    if (a.tiles_per_xcd) {
        const int k = bid >> 3;
        const int t_local = k / a.n_chunks;
        chunk = k - t_local * a.n_chunks;
        tile = (bid & 7) * a.tiles_per_xcd + t_local;
    }
}

// Q3: store the '.3f' text round trip of PS (K4 fused into the store, param ps.quantize3).
// ABL: timing experiments only (param ps.ablate: 1 skip gather, 2 skip staging loads, 4 skip stores);
//      the production instantiations have ABL = 0 and no trace of it.
template <int VEC, bool WEXCL, bool WPS, bool Q3, int ABL>
__device__ __forceinline__ void ps_tile_work(const PsArgs& a, const int bid, const int tid, int4* smem4) {
    typedef typename Vt<VEC>::I VI;
    const int win_cap = a.tile_rows + 2 * a.halo;
    int* tileL = reinterpret_cast<int*>(smem4);
    int* colL = tileL + (size_t)(win_cap + 1) * a.chunk_cols;   // row win_cap is the all-zero padding row
    int* rpL = colL + a.col_cap;
    unsigned* red = reinterpret_cast<unsigned*>(rpL + a.tile_rows + 1);  // [0] max count, [1] max degree

    const int T = blockDim.x;
    int tile, chunk;
    ps_tile_of_block(a, bid, tile, chunk);
    if (tile >= a.n_tiles) return;
    const int c0 = chunk * a.chunk_cols;
    const int cwc = min(a.chunk_cols, a.s - c0);
    const int V = cwc / VEC;
    const int ldw = a.chunk_cols;
    const int64_t r0 = (int64_t)tile * a.tile_rows;
    const int nr = (int)min((int64_t)a.tile_rows, a.n - r0);
    const int slo = (int)max((int64_t)0, r0 - a.halo);
    const int shi = (int)min(a.n, r0 + nr + a.halo);
    const int wrows = shi - slo;
    // A wave that is sending out its window loads goes ahead of the waves that are gathering: the memory pipe stays fed
    // while the co-resident workgroup computes (measured in one process: 0.1845 -> 0.1757 ms at 1 M x 100, 2.02 -> 1.82 ms
    // at 2 M x 500; priority levels 1..3 are equivalent, holding it until the first barrier is worse).
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    if (tid < 3) red[tid] = 0u;                 // [0] max count, [1] max degree, [2] a staged neighbour is outside the window
    for (int i = tid; i < a.chunk_cols; i += T) tileL[(size_t)win_cap * a.chunk_cols + i] = 0;
    const int zero_off = win_cap * a.chunk_cols * 4;

    // ---- CSR row pointers of the tile (their loads go out first, the data loads right behind)
    int64_t rp_mine[2];
    rp_mine[0] = (tid <= nr) ? a.row_ptr[r0 + tid] : 0;
    rp_mine[1] = (tid + T <= nr) ? a.row_ptr[r0 + tid + T] : 0;
    const int64_t kbase = a.row_ptr[r0];

    // ---- stage rows [slo, shi) x cols [c0, c0+cwc) into LDS, 16 B per lane, 4 loads in flight
    unsigned cmax = 0;
    {
        const int total = wrows * V;
        if (cwc == a.s) {
            const VI* g = reinterpret_cast<const VI*>(a.counts + (int64_t)slo * a.s);
            VI* l = reinterpret_cast<VI*>(tileL);
            int i = tid;
            if (ABL & 2) i = total;
            for (; i + 3 * T < total; i += 4 * T) {
                VI v0, v1, v2, v3;
                if (a.nt) {
                    v0 = nt_load(g + i); v1 = nt_load(g + i + T); v2 = nt_load(g + i + 2 * T); v3 = nt_load(g + i + 3 * T);
                } else { v0 = g[i]; v1 = g[i + T]; v2 = g[i + 2 * T]; v3 = g[i + 3 * T]; }
                l[i] = v0; l[i + T] = v1; l[i + 2 * T] = v2; l[i + 3 * T] = v3;
                cmax = max(max(cmax, vmax(v0)), max(vmax(v1), max(vmax(v2), vmax(v3))));
            }
            for (; i < total; i += T) { const VI v = g[i]; l[i] = v; cmax = max(cmax, vmax(v)); }
        } else {
            // row segments of cwc columns: 4 independent loads in flight per lane
            const int* gbase = a.counts + (int64_t)slo * a.s + c0;
            for (int i = (ABL & 2) ? total : tid; i < total; i += 4 * T) {
                VI v[4];
                int lofs[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ii = min(i + q * T, total - 1);      // the tail re-reads the last vector
                    const int rr = ii / V, cc = ii - rr * V;
                    v[q] = *reinterpret_cast<const VI*>(gbase + (int64_t)rr * a.s + cc * VEC);
                    lofs[q] = rr * ldw + cc * VEC;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (i + q * T < total) {
                        *reinterpret_cast<VI*>(tileL + lofs[q]) = v[q];
                        cmax = max(cmax, vmax(v[q]));
                    }
                }
            }
        }
    }
    if (a.prio) __builtin_amdgcn_s_setprio(0);
    // ---- CSR segment -> LDS: relative row pointers, neighbour LDS offsets, max degree
    const int64_t nk = a.row_ptr[r0 + nr] - kbase;
    const bool col_in_lds = nk <= (int64_t)a.col_cap;
    unsigned dmax = 0;
    if (tid <= nr) rpL[tid] = (int)(rp_mine[0] - kbase);
    if (tid + T <= nr) rpL[tid + T] = (int)(rp_mine[1] - kbase);
    for (int i = tid + 2 * T; i <= nr; i += T) rpL[i] = (int)(a.row_ptr[r0 + i] - kbase);
    if (col_in_lds) {
        bool outside = false;
        for (int k = tid; k < (int)nk; k += T) {
            const int j = a.col[kbase + k];
            const unsigned rel = (unsigned)(j - slo);
            outside = outside || rel >= (unsigned)wrows;
            colL[k] = rel < (unsigned)wrows ? (int)(rel * (unsigned)ldw * 4u) : -1 - j;
        }
        if (__ballot(outside) != 0ull && (tid & 63) == 0) atomicOr(&red[2], 1u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, (unsigned)__shfl_xor((int)cmax, o));
    if ((tid & 63) == 0) atomicMax(&red[0], cmax);
    __syncthreads();
    for (int i = tid; i < nr; i += T) dmax = max(dmax, (unsigned)(rpL[i + 1] - rpL[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmax = max(dmax, (unsigned)__shfl_xor((int)dmax, o));
    if ((tid & 63) == 0) atomicMax(&red[1], dmax);
    __syncthreads();
    const unsigned tile_cmax = red[0], tile_dmax = red[1];
    const unsigned thr = 0xFFFFFFu / (tile_dmax + 1u);   // per-count bound keeping incl+excl < 2^24
    const bool fast = tile_cmax <= thr && col_in_lds;     // block-uniform
    const bool all_in = red[2] == 0u;                     // block-uniform: no per-batch window check needed

    // ---- per (row, vector) item: gather neighbours from LDS, divide, store
    {
        const char* tileB = reinterpret_cast<const char*>(tileL);
        const int items = nr * V;
        int ri = tid / V, c = tid - ri * V;
        const int dr = T / V, dc = T - dr * V;
        const int own_base = (int)(r0 - slo);
        for (int it = tid; it < items; it += T) {
            const int k0 = rpL[ri], k1 = (ABL & 1) ? k0 : rpL[ri + 1];
            const int64_t o = (r0 + ri) * a.s + c0 + c * VEC;
            const int own_off = (own_base + ri) * ldw * 4;
            bool done = false;
            if (fast)
                done = all_in ? ps_item_fast<VEC, WEXCL, WPS, false, Q3, ABL>(a, tileB, colL, k0, k1, c * VEC * 4, own_off, o, zero_off)
                              : ps_item_fast<VEC, WEXCL, WPS, true, Q3, ABL>(a, tileB, colL, k0, k1, c * VEC * 4, own_off, o, zero_off);
            if (!done)
                ps_item_slow<VEC, WEXCL, WPS, Q3, ABL>(a, tileB, colL, col_in_lds, kbase, k0, k1, slo, wrows, ldw, c0, c * VEC,
                                              own_off, o, slo);
            c += dc; ri += dr;
            if (c >= V) { c -= V; ri += 1; }
        }
    }
}

// One workgroup per (tile, chunk) work item.  (A resident set of workgroups striding over the work items --
// the next tile's loads issued behind the current tile's stores, same LDS -- was measured against this in
// one process: 0.203 ms vs 0.173 ms at 1 M x 100, 2.05 ms vs 1.79 ms at 2 M x 500; the hardware's dynamic
// dispatch balances the tiles better than a static stride and the store drain is not what limits a CU.)
template <int VEC, bool WEXCL, bool WPS, bool Q3, int ABL>
__global__ void __launch_bounds__(1024) ps_tile_kernel(PsArgs a) {
    extern __shared__ int4 smem4[];
    ps_tile_work<VEC, WEXCL, WPS, Q3, ABL>(a, blockIdx.x, threadIdx.x, smem4);
}


// maximum over the 64 lanes by DPP steps (VALU latency; six ds_bpermute round trips on the tile's critical path were
// measurable): the result is valid in lane 63
__device__ __forceinline__ unsigned wave_max_dpp(unsigned x) {
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true));   // row_half_mirror
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true));   // row_mirror
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, true));   // row_bcast:15 -> rows 1, 3
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, true));   // row_bcast:31 -> rows 2, 3
    return x;
}

// ---------------------------------------------------------------------------------------------------
// What the register-staged tile kernels (ps_tile_v3_kernel, ps_tile_w16_kernel) share.  The ORDER stays with the kernels:
// the window loads are issued as (1) own vectors, (2) ps_tile_scalars, (3) low halo run, (4) neighbour indices, (5) row
// pointers, a compiler barrier, (6) last own vector and high halo run, and are consumed in that order further down (own
// vectors, low run, indices and pointers, last own vector, high run), so that hipcc's counted vmcnt waits retire them one
// by one.  (Steps (4)/(5) and their retirement stand in each kernel: as helpers they moved the VGPR count of either the
// chunked ps_tile_v3_kernel or ps_tile_w16_kernel by two -- EXPERIMENTS A.23.)

// Step (2), the uniform scalars of a tile: first / last row pointer and the halo rows the lists really reach (nlo below,
// nhi above the tile; `halo` without reach words).  Scalar loads: they return on lgkmcnt, the vector queue stays untouched
__device__ __forceinline__ void ps_tile_scalars(const PsArgs& a, int r0, int nr, long long& kbase, long long& kend, int& nlo, int& nhi) {
    nlo = a.halo; nhi = a.halo;
    const int64_t* pf = a.row_ptr + r0;
    const int64_t* pl = pf + nr;
    if (a.reach) {
        const int b0 = r0 >> 4, bl = (r0 + nr - 1) >> 4;
        const uint32_t* q0 = a.reach + b0;
        const uint32_t* q1 = a.reach + min(b0 + 1, bl);
        const uint32_t* q2 = a.reach + max(bl - 1, b0);
        const uint32_t* q3 = a.reach + bl;
        unsigned w0, w1, w2, w3;
        asm volatile("s_nop 4\n\ts_load_dwordx2 %0, %6, 0x0\n\ts_load_dwordx2 %1, %7, 0x0\n\t"
                     "s_load_dword %2, %8, 0x0\n\ts_load_dword %3, %9, 0x0\n\t"
                     "s_load_dword %4, %10, 0x0\n\ts_load_dword %5, %11, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(kbase), "=&s"(kend), "=&s"(w0), "=&s"(w1), "=&s"(w2), "=&s"(w3)
                     : "s"(pf), "s"(pl), "s"(q0), "s"(q1), "s"(q2), "s"(q3) : "memory");
        // block b reaches (w & 255) rows below row 16 b and (w >> 8 & 255) rows beyond row 16 b + 15
        const int e = r0 + nr - 1;
        int lo_need = (int)(w0 & 255u);
        if (b0 < bl) lo_need = max(lo_need, (int)(w1 & 255u) - 16);
        int hi_need = ((bl << 4) + 15 + (int)((w3 >> 8) & 255u)) - e;
        if (b0 < bl) hi_need = max(hi_need, (bl << 4) - 1 + (int)((w2 >> 8) & 255u) - e);
        nlo = min(max(lo_need, 0), a.halo);
        nhi = min(max(hi_need, 0), a.halo);
    } else {
        asm volatile("s_nop 4\n\ts_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(kbase), "=&s"(kend) : "s"(pf), "s"(pl) : "memory");
    }
}

// The tile's ONE workgroup barrier and what goes through it: every wave's largest count and whether one of its staged
// neighbours is outside the window.  One word per wave (the count saturating at 2^24: beyond that no item is fast, bit
// 31 = outside); sixteen words are read back, wave 0 clears the unused ones.  Returns the tile's largest count
// (uniform), all_in: no item needs the per-batch window check (uniform)
__device__ __forceinline__ unsigned ps_tile_sync_bound(unsigned cmax, bool outside, unsigned* red, int lane, int wave, int NW, bool& all_in) {
    cmax = wave_max_dpp(cmax);
    const unsigned long long any_out = __ballot(outside);
    if (lane == 63) red[wave] = min(cmax, 0x1000000u) | (any_out != 0ull ? 0x80000000u : 0u);
    if (wave == 0 && lane >= NW && lane < 16) red[lane] = 0u;
    __syncthreads();
    const uint4* r4 = reinterpret_cast<const uint4*>(red);
    const uint4 x0 = r4[0], x1 = r4[1], x2 = r4[2], x3 = r4[3];
    const unsigned tile_or = (x0.x | x0.y | x0.z | x0.w) | (x1.x | x1.y | x1.z | x1.w) | (x2.x | x2.y | x2.z | x2.w) | (x3.x | x3.y | x3.z | x3.w);
    const unsigned k = 0x7fffffffu;
    const unsigned m0 = max(max(x0.x & k, x0.y & k), max(x0.z & k, x0.w & k)), m1 = max(max(x1.x & k, x1.y & k), max(x1.z & k, x1.w & k));
    const unsigned m2 = max(max(x2.x & k, x2.y & k), max(x2.z & k, x2.w & k)), m3 = max(max(x3.x & k, x3.y & k), max(x3.z & k, x3.w & k));
    const unsigned tile_cmax = (unsigned)__builtin_amdgcn_readfirstlane((int)max(max(m0, m1), max(m2, m3)));
    all_in = __builtin_amdgcn_readfirstlane((int)tile_or) >= 0;
    return tile_cmax;
}

// The arguments with the outputs rebased to the tile's first element, and the walk of one thread over the tile's (row,
// 4-column vector) items tid, tid + T, ...: the outputs are addressed as (tile base: scalar) + (32-bit element offset
// inside the tile: the host keeps a tile below 2^30 elements), and the offsets of successive items follow by additions:
// no 64-bit multiply-add, no 32-bit multiplications (quarter-rate) per item -- the kernel runs at 3/4 of the VALU issue rate
template <bool WEXCL, bool WPS>
__device__ __forceinline__ PsArgs ps_tile_outputs(const PsArgs& a, int r0, int c0) {
    PsArgs b = a;
    const int64_t tile_base = (int64_t)r0 * a.s + c0;
    if (WPS) b.ps = a.ps + tile_base;
    if (WEXCL) b.excl = a.excl + tile_base;
    return b;
}
struct PsItemWalk {
    int ri, c;              // row of the tile, vector of the chunk
    unsigned o32;           // element offset of the item's outputs from the tile's first
    int own_off;            // LDS byte offset of the item's own window row
    int V, rowb, dr, dc, d_own;
    unsigned d_o, wrap_o;
    // V vectors per row of the chunk, window rows of rowb bytes
    __device__ __forceinline__ PsItemWalk(const PsArgs& a, int tid, int T, int V_, int rowb_) : V(V_), rowb(rowb_) {
        ri = tid / V; c = tid - ri * V;
        dr = T / V; dc = T - dr * V;
        o32 = (unsigned)ri * (unsigned)a.s + (unsigned)(c * 4);
        d_o = (unsigned)dr * (unsigned)a.s + (unsigned)(dc * 4); wrap_o = (unsigned)a.s - (unsigned)(V * 4);
        own_off = (a.halo + ri) * rowb;
        d_own = dr * rowb;
    }
    __device__ __forceinline__ int64_t out_index() const { return (int64_t)(uint64_t)o32; }
    __device__ __forceinline__ void next() {
        c += dc; ri += dr; o32 += d_o; own_off += d_own;
        if (c >= V) { c -= V; ri += 1; o32 += wrap_o; own_off += rowb; }
    }
};

// ---------------------------------------------------------------------------------------------------
// Register-staged tile kernel, second generation (VEC = 4 tables).  The window passes through the VGPRs
// (which gives the tile's count bound for free; an LDS-DMA staging, global_load_lds_dwordx4, was built in round 3,
// bit-exact and slower -- DESIGN appendix A.3):
//   * EVERY global load of the tile is issued before the first one is waited for: the tile's own rows (up to four
//     vectors per thread) but the last vector a tile of this shape has, then -- behind one scalar-load round trip for
//     the first / last row pointer and the reach words -- the halo rows below the tile that the lists really reach
//     (reach words of the clustering kernel, 16 rows in all on gene-shaped data instead of 2 x 16), the neighbour
//     indices and the row pointers, and last the tile's last own vector and the halo rows above it; hipcc's counted
//     vmcnt waits then retire them in issue order while the data moves to LDS, so the lists and the low end of the
//     window stand in LDS while the high end is still landing.  An own vector that no tile of the launch has (the
//     fourth at 96-row tiles of 128-column chunks) is not loaded at all;
//   * one workgroup barrier: the count bound goes through one LDS word per wave (DPP reduction, sixteen broadcast
//     reads after the barrier), the degree enters per item: an item is fast iff (degree + 1) * bound < 2^24.
template <bool CHUNKED, bool WEXCL, bool WPS, bool Q3>
__global__ void __launch_bounds__(1024, 8) ps_tile_v3_kernel(PsArgs a) {
    extern __shared__ int4 smem4[];
    constexpr int VEC = 4;
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = T >> 6;
    const int win_cap = a.tile_rows + 2 * a.halo;
    int* tileL = reinterpret_cast<int*>(smem4);
    int* colL = tileL + (win_cap + 1) * a.chunk_cols;            // row win_cap is the all-zero padding row
    int* rpL = colL + a.col_cap;
    unsigned* red = reinterpret_cast<unsigned*>(rpL + ((a.tile_rows + 1 + 3) & ~3));   // one word per wave (16-byte aligned)

    const int bid = blockIdx.x;
    int tile, chunk = 0;
    if (!CHUNKED) tile = a.tiles_per_xcd ? (bid & 7) * a.tiles_per_xcd + (bid >> 3) : bid;
    else ps_tile_of_block(a, bid, tile, chunk);
    if (tile >= a.n_tiles) return;
    const int c0 = chunk * a.chunk_cols;
    const int cwc = CHUNKED ? min(a.chunk_cols, a.s - c0) : a.s;
    const int V = cwc / VEC;
    const int ldw = a.chunk_cols, LV = ldw / VEC;
    const int lsh = 6 - a.lv_shift;                        // column chunks: log2(LV)
    const int r0 = tile * a.tile_rows;                     // (n < 2^31)
    const int nr = min(a.tile_rows, (int)a.n - r0);
    const int wbase = r0 - a.halo;                         // row that LDS window row 0 stands for (may be negative)
    const int rowb = ldw * 4;
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    for (int i = tid; i < LV; i += T) reinterpret_cast<int4*>(tileL + win_cap * a.chunk_cols)[i] = make_int4(0, 0, 0, 0);
    const int zero_off = win_cap * a.chunk_cols * 4;
    int4* win4 = reinterpret_cast<int4*>(tileL);

    // ---- (1) the tile's own rows, up to four vectors per thread: slots 0, 1 and -- where tiles have a fourth vector --
    // 2 go out now; slot 3 is the LAST vector a tile of this shape has (its third or fourth) and goes out in (6).  A
    // vector that no tile of this launch has is not loaded (wave-uniform branches)
    const char* gtile = reinterpret_cast<const char*>(a.counts + (int64_t)r0 * a.s + c0);
    const int64_t row_stride = (int64_t)a.s * 4;
    const int ctot = nr * LV;
    const int tvec = a.tile_rows * LV;                     // (uniform)
    const bool grp3 = tvec > 2 * T, grp4 = tvec > 3 * T;
    int4 cv[4];
    bool cok[4];
    int cdst[4];                                            // LDS vector index
    const int4* g[4];
    // unconditional loads at clamped positions (a predicated load drags exec-mask code and early waits into the
    // sequence); the predicate acts on the LDS store
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = tid + (k < 3 ? k : (grp4 ? 3 : 2)) * T;
        cok[k] = idx < ctot && (k < 2 || (k == 2 ? grp4 : grp3));
        cdst[k] = a.halo * LV + idx;
        const int ic = min(idx, ctot - 1);
        if (!CHUNKED) g[k] = reinterpret_cast<const int4*>(gtile) + ic;
        else {
            const int rr = ic >> lsh, cc = ic & (LV - 1);
            cok[k] = cok[k] && cc < V;
            g[k] = reinterpret_cast<const int4*>(gtile + rr * row_stride) + min(cc, V - 1);
        }
    }
    // (a.nt: unchunked tables only; cv[2] stays unset, and unused, where no tile has a fourth vector)
    if (!CHUNKED && a.nt) { cv[0] = nt_load(g[0]); cv[1] = nt_load(g[1]); if (grp4) cv[2] = nt_load(g[2]); }
    else                  { cv[0] = *g[0]; cv[1] = *g[1]; if (grp4) cv[2] = *g[2]; }

    // ---- (2) uniform scalars of the tile, one scalar-load round trip
    long long kbase, kend;
    int nlo, nhi;
    ps_tile_scalars(a, r0, nr, kbase, kend, nlo, nhi);
    const int nk = (int)(kend - kbase);
    const int slo = max(0, r0 - nlo);
    const int shi = min((int)a.n, r0 + nr + nhi);
    const int wrows = shi - slo;

    // ---- (3) halo rows: the run below the tile (loaded here) and the run above it (loaded in (6)), one vector per
    // thread each (the host keeps a run at T vectors)
    const int lo_rows = r0 - slo, hi_rows = shi - (r0 + nr);
    int4 hv[2];
    int hdst[2];                                            // LDS vector index, -1: nothing
    const int4* hg[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool is_lo = k == 0;
        bool ok = tid < (is_lo ? lo_rows : hi_rows) * LV;
        // (clamped: the tile's first vector stands in for a missing one)
        const char* grun = is_lo ? gtile - lo_rows * row_stride : (ok ? gtile + nr * row_stride : gtile);
        const int jc = ok ? tid : 0;
        const int ldst = (is_lo ? (slo - wbase) : (a.halo + nr)) * LV + tid;
        if (!CHUNKED) hg[k] = reinterpret_cast<const int4*>(grun) + jc;
        else {
            const int rr = jc >> lsh, cc = jc & (LV - 1);
            ok = ok && cc < V;
            hg[k] = reinterpret_cast<const int4*>(grun + rr * row_stride) + min(cc, V - 1);
        }
        hdst[k] = ok ? ldst : -1;
    }
    hv[0] = *hg[0];                                         // (halo rows are another tile's own rows: they may stay in the L2)
    // ---- (4) neighbour indices (three per thread) and (5) row pointers (two per thread)
    const bool col_in_lds = nk <= a.col_cap && nk <= 3 * T;
    int jv[3];
    {
        // (clamped; a tile without list entries reads the row pointers instead: a.col may end exactly at kbase, or be NULL)
        const int* cbase = nk > 0 ? a.col + kbase : reinterpret_cast<const int*>(a.row_ptr + r0);
        const int last = col_in_lds ? max(nk - 1, 0) : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) jv[k] = cbase[min(tid + k * T, last)];
    }
    int rp_mine[2];                                         // (low words: a tile's lists are < 2^31 entries)
    rp_mine[0] = reinterpret_cast<const int*>(a.row_ptr + r0 + min(tid, nr))[0];
    rp_mine[1] = reinterpret_cast<const int*>(a.row_ptr + r0 + min(tid + T, nr))[0];
    // ---- (6) the high end of the window, behind everything else in the vector queue (loads retire in issue order): the
    // tile's last own vector and the run above the tile
    asm volatile("" ::: "memory");
    if (!CHUNKED && a.nt) cv[3] = nt_load(g[3]); else cv[3] = *g[3];
    hv[1] = *hg[1];
    if (a.prio) __builtin_amdgcn_s_setprio(0);

    // ---- retire them in issue order: window vectors to LDS (their maximum on the way), offsets, pointers
    unsigned cmax = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (cok[k]) { win4[cdst[k]] = cv[k]; cmax = max(cmax, vmax(cv[k])); }
    if (hdst[0] >= 0) { win4[hdst[0]] = hv[0]; cmax = max(cmax, vmax(hv[0])); }
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int kk = tid + k * T;
        if (col_in_lds && kk < nk) {
            const int j = jv[k];
            const bool in = (unsigned)(j - slo) < (unsigned)wrows;
            outside = outside || !in;
            colL[kk] = in ? (int)__umul24((unsigned)(j - wbase), (unsigned)rowb) : -1 - j;      // (window rows < 2^12, row bytes < 2^18: full-rate 24-bit multiply)
        }
    }
    if (tid <= nr) rpL[tid] = rp_mine[0] - (int)kbase;
    if (tid + T <= nr) rpL[tid + T] = rp_mine[1] - (int)kbase;
    if (cok[3]) { win4[cdst[3]] = cv[3]; cmax = max(cmax, vmax(cv[3])); }
    // (the last load is consumed outside the predicate: its wait, vmcnt(0), then stands on every path, and the item
    // loop, whose registers these were, needs none -- a wait there would be a wait for its own stores)
    cmax = max(cmax, hdst[1] >= 0 ? vmax(hv[1]) : 0u);
    if (hdst[1] >= 0) win4[hdst[1]] = hv[1];
    bool all_in;                                                                         // block-uniform, as is tile_cmax
    const unsigned tile_cmax = ps_tile_sync_bound(cmax, outside, red, lane, wave, NW, all_in);
    // an item is fast (32-bit sums, float32 quotient) iff (degree + 1) * (largest count of the tile) < 2^24
    const bool fast_tile = tile_cmax <= 0xFFFFFFu && col_in_lds;                         // block-uniform

    // ---- per (row, vector) item: gather neighbours from LDS, divide, store
    {
        const char* tileB = reinterpret_cast<const char*>(tileL);
        const int items = nr * V;
        const PsArgs b = ps_tile_outputs<WEXCL, WPS>(a, r0, c0);
        PsItemWalk w(a, tid, T, V, rowb);
        // (degree + 1) * (largest count of the tile) < 2^24  <=>  degree + 1 <= deg_lim
        const unsigned deg_lim = tile_cmax ? 0xFFFFFFu / tile_cmax : 0xFFFFFFFFu;
        for (int it = tid; it < items; it += T, w.next()) {
            const int k0 = rpL[w.ri], k1 = rpL[w.ri + 1];
            const int64_t o = w.out_index();
            bool done = false;
            const unsigned deg = (unsigned)(k1 - k0);
            if (fast_tile && deg < 254u && deg + 1u <= deg_lim)
                done = all_in ? ps_item_fast<VEC, WEXCL, WPS, false, Q3, 0>(b, tileB, colL, k0, k1, w.c * VEC * 4, w.own_off, o, zero_off)
                              : ps_item_fast<VEC, WEXCL, WPS, true, Q3, 0>(b, tileB, colL, k0, k1, w.c * VEC * 4, w.own_off, o, zero_off);
            if (!done)
                ps_item_slow<VEC, WEXCL, WPS, Q3, 0>(b, tileB, colL, col_in_lds, kbase, k0, k1, slo, wrows, ldw, c0, w.c * VEC,
                                                     w.own_off, o, wbase);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Register-staged tile kernel with a 16-bit count window (column-chunked VEC = 4 tables, geometry: psplan.cpp).  The
// window stands in LDS as saturated 16-bit words, min(count, 0xFFFF): a window row is chunk_cols x 2 bytes, a neighbour
// is one 8-byte LDS read, and the same LDS holds twice the cells -- SIX items per thread share the per-tile fixed cost
// that three share in ps_tile_v3_kernel.  The two kernels share their steps through the helpers above: the XCD remap
// (ps_tile_of_block), the reach-sized halo runs (ps_tile_scalars), the single
// barrier (ps_tile_sync_bound), the item walk (PsItemWalk) and the batches and non-temporal stores of a 32-bit item
// (ps_batch_offsets, ps_finish32), in one load order; the tile's count bound is taken from the 32-bit registers before
// they are packed.  The row segments of a chunk divide the workgroup (T % LV == 0), so a thread keeps ONE column and
// its vectors lie T / LV rows apart: the loads are addressed as (tile base: scalar) + (32-bit byte offset), offsets that
// follow each other by additions.
// Arithmetic per item, bound = the largest count the tile loaded:
//   1. (degree + 1) x bound <= 0xFFFF: the sums fit the halves, one 32-bit addition adds two of them;
//   2. bound < 0xFFFF (then (degree + 1) x bound < 2^24 for every degree below the cutoff of 254): 32-bit sums of the halves;
//      bound >= 0xFFFF: the same, with a packed running maximum of every word read -- no half at 0xFFFF means every
//      count the item read is exact and below 0xFFFF, so its total is below 254 x 0xFFFF < 2^24;
//   3. otherwise (a saturated half, a neighbour outside the window, a degree from 254 on, lists beyond the offset
//      stage): 64-bit sums with EVERY count read from global memory -- the window cannot be trusted above 0xFFFE.
// All three give the exact sums and the correctly rounded quotient of the contract, i.e. the bits of ps_tile_v3_kernel.
__device__ __forceinline__ uint2 pack_sat16(const int4& v) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    uint2 r;                                                // (v_cvt_pk_u16_u32 saturates)
    r.x = __builtin_bit_cast(unsigned, (us2)__builtin_amdgcn_cvt_pk_u16((unsigned)v.x, (unsigned)v.y));
    r.y = __builtin_bit_cast(unsigned, (us2)__builtin_amdgcn_cvt_pk_u16((unsigned)v.z, (unsigned)v.w));
    return r;
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// tier 1: packed sums
template <bool WEXCL, bool WPS, bool CHECK, bool Q3>
__device__ __forceinline__ bool ps16_item_packed(const PsArgs& a, const char* tileB, const int* colL, int k0, int k1,
                                                 int cbytes, int own_off, int64_t out_index, int zero_off) {
    constexpr int GB = 4;
    unsigned s01 = 0, s23 = 0;
    for (int k = k0; k < k1; k += GB) {
        int off[GB];
        if (!ps_batch_offsets<CHECK, GB>(colL, k, k1, zero_off, off)) return false;
        uint2 v[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) v[u] = *reinterpret_cast<const uint2*>(tileB + off[u] + cbytes);
#pragma unroll
        for (int u = 0; u < GB; ++u) { s01 += v[u].x; s23 += v[u].y; }         // (no half overflows: no carry between them)
    }
    const uint2 own = *reinterpret_cast<const uint2*>(tileB + own_off + cbytes);
    const unsigned in[4] = {own.x & 0xFFFFu, own.x >> 16, own.y & 0xFFFFu, own.y >> 16};
    const unsigned acc[4] = {s01 & 0xFFFFu, s01 >> 16, s23 & 0xFFFFu, s23 >> 16};
    ps_finish32<WEXCL, WPS, Q3>(a, in, acc, out_index);
    return true;
}

// tier 2: 32-bit sums of the halves; SAT: false (nothing stored) when a word the item read holds a saturated half
template <bool WEXCL, bool WPS, bool CHECK, bool SAT, bool Q3>
__device__ __forceinline__ bool ps16_item_wide(const PsArgs& a, const char* tileB, const int* colL, int k0, int k1,
                                               int cbytes, int own_off, int64_t out_index, int zero_off) {
    constexpr int GB = 4;
    unsigned acc[4] = {0u, 0u, 0u, 0u};
    const uint2 own = *reinterpret_cast<const uint2*>(tileB + own_off + cbytes);
    unsigned m01 = own.x, m23 = own.y;
    for (int k = k0; k < k1; k += GB) {
        int off[GB];
        if (!ps_batch_offsets<CHECK, GB>(colL, k, k1, zero_off, off)) return false;
        uint2 v[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) v[u] = *reinterpret_cast<const uint2*>(tileB + off[u] + cbytes);
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            acc[0] += v[u].x & 0xFFFFu; acc[1] += v[u].x >> 16; acc[2] += v[u].y & 0xFFFFu; acc[3] += v[u].y >> 16;
            if (SAT) { m01 = pk_max_u16(m01, v[u].x); m23 = pk_max_u16(m23, v[u].y); }
        }
    }
    if (SAT) {
        const unsigned m = pk_max_u16(m01, m23);
        if ((m & 0xFFFFu) == 0xFFFFu || m >= 0xFFFF0000u) return false;
    }
    const unsigned in[4] = {own.x & 0xFFFFu, own.x >> 16, own.y & 0xFFFFu, own.y >> 16};
    ps_finish32<WEXCL, WPS, Q3>(a, in, acc, out_index);
    return true;
}

// tier 3: every count from global memory, 64-bit sums, float64 division
template <bool WEXCL, bool WPS, bool Q3>
__device__ __forceinline__ void ps16_item_global(const PsArgs& a, int64_t kbase, int k0, int k1, int64_t row, int col0,
                                                 int64_t out_index) {
    unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
    for (int k = k0; k < k1; ++k) {
        const int j = a.col[kbase + k];
        acc_add(acc, *reinterpret_cast<const int4*>(a.counts + (int64_t)j * a.s + col0));
    }
    const int4 own = *reinterpret_cast<const int4*>(a.counts + row * a.s + col0);
    ps_finish64<4, WEXCL, WPS, Q3, 0>(a, own, acc, out_index);
}

template <bool WEXCL, bool WPS, bool Q3>
__global__ void __launch_bounds__(1024, 8) ps_tile_w16_kernel(PsArgs a) {
    extern __shared__ int4 smem4[];
    constexpr int VEC = 4, NOWN = PS_W16_OWN_VECTORS;
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = T >> 6;
    const int win_cap = a.tile_rows + 2 * a.halo;
    const int ldw = a.chunk_cols, LV = ldw / VEC;
    const int rowb = ldw * 2;                              // bytes of a window row
    char* tileB = reinterpret_cast<char*>(smem4);
    uint2* win8 = reinterpret_cast<uint2*>(smem4);
    int* colL = reinterpret_cast<int*>(tileB + (win_cap + 1) * rowb);          // row win_cap is the all-zero padding row
    int* rpL = colL + a.col_cap;
    unsigned* red = reinterpret_cast<unsigned*>(rpL + ((a.tile_rows + 1 + 3) & ~3));   // one word per wave (16-byte aligned)

    int tile, chunk;
    ps_tile_of_block(a, blockIdx.x, tile, chunk);
    if (tile >= a.n_tiles) return;
    const int c0 = chunk * a.chunk_cols;
    const int cwc = min(a.chunk_cols, a.s - c0);
    const int V = cwc / VEC;
    const int lsh = 6 - a.lv_shift;                        // log2(LV)
    const int r0 = tile * a.tile_rows;                     // (n < 2^31)
    const int nr = min(a.tile_rows, (int)a.n - r0);
    const int wbase = r0 - a.halo;                         // row that LDS window row 0 stands for (may be negative)
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    for (int i = tid; i < LV; i += T) win8[win_cap * LV + i] = make_uint2(0u, 0u);
    const int zero_off = win_cap * rowb;

    // ---- (1) the tile's own rows: vector k of a thread is its column of row rr + k T / LV; five go out now, the last one
    // in (6).  Unconditional loads at clamped positions (a row past the tile reads its last row), the predicate acts on
    // the LDS store
    const char* gtile = reinterpret_cast<const char*>(a.counts + (int64_t)r0 * a.s + c0);
    const unsigned row_stride = (unsigned)a.s * 4u;        // (s < 2^19: a tile's rows span less than 2^31 bytes)
    const int rr = tid >> lsh, cc = tid & (LV - 1);
    const bool col_ok = cc < V;
    const unsigned ccb = (unsigned)min(cc, V - 1) * 16u;
    const unsigned rowoff = __umul24((unsigned)rr, row_stride);                 // (rr < 2^11, row bytes < 2^21)
    const unsigned step = (unsigned)(T >> lsh) * row_stride, last_row = (unsigned)(nr - 1) * row_stride;
    int4 cv[NOWN];
#pragma unroll
    for (int k = 0; k < NOWN - 1; ++k)
        cv[k] = *reinterpret_cast<const int4*>(gtile + (size_t)(min(rowoff + (unsigned)k * step, last_row) + ccb));

    // ---- (2) uniform scalars of the tile, one scalar-load round trip
    long long kbase, kend;
    int nlo, nhi;
    ps_tile_scalars(a, r0, nr, kbase, kend, nlo, nhi);
    const int nk = (int)(kend - kbase);
    const int slo = max(0, r0 - nlo);
    const int shi = min((int)a.n, r0 + nr + nhi);
    const int wrows = shi - slo;

    // ---- (3) halo rows: the run below the tile (loaded here) and the run above it (loaded in (6)), one vector per
    // thread each (the host keeps a run at T / LV rows): the thread's column of row rr of the run
    const int lo_rows = r0 - slo, hi_rows = shi - (r0 + nr);
    const bool lo_ok = col_ok && rr < lo_rows, hi_ok = col_ok && rr < hi_rows;
    // (clamped: a run's last row, or the tile's first row, stands in for a missing one)
    const char* glo = gtile - (int64_t)lo_rows * row_stride;
    const char* ghi = hi_rows > 0 ? gtile + (int64_t)nr * row_stride : gtile;
    const unsigned lo_off = min(rowoff, (unsigned)max(lo_rows - 1, 0) * row_stride) + ccb;
    const unsigned hi_off = min(rowoff, (unsigned)max(hi_rows - 1, 0) * row_stride) + ccb;
    int4 hv[2];
    hv[0] = *reinterpret_cast<const int4*>(glo + (size_t)lo_off);   // (halo rows are another tile's own rows: they may stay in the L2)
    // ---- (4) neighbour indices (three per thread) and (5) row pointers (two per thread)
    const bool col_in_lds = nk <= a.col_cap && nk <= 3 * T;
    int jv[3];
    {
        // (clamped; a tile without list entries reads the row pointers instead: a.col may end exactly at kbase, or be NULL)
        const int* cbase = nk > 0 ? a.col + kbase : reinterpret_cast<const int*>(a.row_ptr + r0);
        const int last = col_in_lds ? max(nk - 1, 0) : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) jv[k] = cbase[min(tid + k * T, last)];
    }
    int rp_mine[2];                                         // (low words: a tile's lists are < 2^31 entries)
    rp_mine[0] = reinterpret_cast<const int*>(a.row_ptr + r0 + min(tid, nr))[0];
    rp_mine[1] = reinterpret_cast<const int*>(a.row_ptr + r0 + min(tid + T, nr))[0];
    // ---- (6) the high end of the window, behind everything else in the vector queue (loads retire in issue order)
    asm volatile("" ::: "memory");
    cv[NOWN - 1] = *reinterpret_cast<const int4*>(gtile + (size_t)(min(rowoff + (unsigned)(NOWN - 1) * step, last_row) + ccb));
    hv[1] = *reinterpret_cast<const int4*>(ghi + (size_t)hi_off);
    if (a.prio) __builtin_amdgcn_s_setprio(0);

    // ---- retire them in issue order: window vectors to LDS as saturated halves (their 32-bit maximum on the way),
    // offsets, pointers
    unsigned cmax = 0;
    const int rstep = T >> lsh;                            // rows between a thread's own vectors
    uint2* own8 = win8 + a.halo * LV + tid;
#pragma unroll
    for (int k = 0; k < NOWN - 1; ++k)
        if (col_ok && rr + k * rstep < nr) { own8[k * T] = pack_sat16(cv[k]); cmax = max(cmax, vmax(cv[k])); }
    if (lo_ok) { win8[(slo - wbase) * LV + tid] = pack_sat16(hv[0]); cmax = max(cmax, vmax(hv[0])); }
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int kk = tid + k * T;
        if (col_in_lds && kk < nk) {
            const int j = jv[k];
            const bool in = (unsigned)(j - slo) < (unsigned)wrows;
            outside = outside || !in;
            colL[kk] = in ? (int)__umul24((unsigned)(j - wbase), (unsigned)rowb) : -1 - j;      // (window rows < 2^12, row bytes < 2^18)
        }
    }
    if (tid <= nr) rpL[tid] = rp_mine[0] - (int)kbase;
    if (tid + T <= nr) rpL[tid + T] = rp_mine[1] - (int)kbase;
    if (col_ok && rr + (NOWN - 1) * rstep < nr) { own8[(NOWN - 1) * T] = pack_sat16(cv[NOWN - 1]); cmax = max(cmax, vmax(cv[NOWN - 1])); }
    // (the last load is consumed outside the predicate: its wait, vmcnt(0), then stands on every path)
    cmax = max(cmax, hi_ok ? vmax(hv[1]) : 0u);
    if (hi_ok) win8[(a.halo + nr) * LV + tid] = pack_sat16(hv[1]);
    // a run of more than T / LV rows (the host keeps it at twice that): the few tiles whose reach words ask for one
    // load its further rows here, behind everything else (block-uniform branch)
    if (max(lo_rows, hi_rows) > rstep) {
        const int r2 = rr + rstep;
        if (col_ok && r2 < lo_rows) {
            const int4 v = *reinterpret_cast<const int4*>(glo + (size_t)(rowoff + step + ccb));
            win8[(slo - wbase) * LV + tid + T] = pack_sat16(v); cmax = max(cmax, vmax(v));
        }
        if (col_ok && r2 < hi_rows) {
            const int4 v = *reinterpret_cast<const int4*>(ghi + (size_t)(rowoff + step + ccb));
            win8[(a.halo + nr) * LV + tid + T] = pack_sat16(v); cmax = max(cmax, vmax(v));
        }
    }
    bool all_in;                                                                         // block-uniform, as is tile_cmax
    const unsigned tile_cmax = ps_tile_sync_bound(cmax, outside, red, lane, wave, NW, all_in);
    const bool hi_tile = tile_cmax >= 0xFFFFu;                                           // block-uniform: halves may be saturated
    // (degree + 1) * (largest count of the tile) <= 0xFFFF  <=>  degree + 1 <= lim16
    const unsigned lim16 = tile_cmax ? 0xFFFFu / tile_cmax : 0xFFFFFFFFu;

    // ---- per (row, vector) item: gather neighbours from LDS, divide, store
    {
        const int items = nr * V;
        const PsArgs b = ps_tile_outputs<WEXCL, WPS>(a, r0, c0);
        PsItemWalk w(a, tid, T, V, rowb);
        for (int it = tid; it < items; it += T, w.next()) {
            const int k0 = rpL[w.ri], k1 = rpL[w.ri + 1];
            const int64_t o = w.out_index();
            bool done = false;
            const unsigned deg = (unsigned)(k1 - k0);
            if (col_in_lds && deg < 254u) {
                if (hi_tile)
                    done = ps16_item_wide<WEXCL, WPS, true, true, Q3>(b, tileB, colL, k0, k1, w.c * 8, w.own_off, o, zero_off);
                else if (deg + 1u <= lim16)
                    done = all_in ? ps16_item_packed<WEXCL, WPS, false, Q3>(b, tileB, colL, k0, k1, w.c * 8, w.own_off, o, zero_off)
                                  : ps16_item_packed<WEXCL, WPS, true, Q3>(b, tileB, colL, k0, k1, w.c * 8, w.own_off, o, zero_off);
                else
                    done = all_in ? ps16_item_wide<WEXCL, WPS, false, false, Q3>(b, tileB, colL, k0, k1, w.c * 8, w.own_off, o, zero_off)
                                  : ps16_item_wide<WEXCL, WPS, true, false, Q3>(b, tileB, colL, k0, k1, w.c * 8, w.own_off, o, zero_off);
            }
            if (!done)
                ps16_item_global<WEXCL, WPS, Q3>(b, kbase, k0, k1, (int64_t)(r0 + w.ri), c0 + w.c * VEC, o);
        }
    }
}

__global__ void quantize3_kernel(float* __restrict__ x, int64_t n) {
    // f'{x:.3f}' -> float32: x*1000 is exact in float64 for a float32 x (24+10 bits), rint
    // is round-half-even like the decimal formatter, k/1000 -> f32 has no double-rounding
    // hazard (k/1000 is >= 2^-35 away from every f32 rounding boundary).
    // Any 4-byte-aligned pointer: up to three leading scalars bring x to a 16-byte boundary, float4 body, scalar tail.
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t lead = min((int64_t)((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2, n);
    if (gid < lead) x[gid] = (float)(rint((double)x[gid] * 1000.0) / 1000.0);
    x += lead; n -= lead;
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* x4 = reinterpret_cast<float4*>(x);
    for (int64_t i = gid; i < n4; i += stride) {
        float4 v = x4[i];
        v.x = (float)(rint((double)v.x * 1000.0) / 1000.0);
        v.y = (float)(rint((double)v.y * 1000.0) / 1000.0);
        v.z = (float)(rint((double)v.z * 1000.0) / 1000.0);
        v.w = (float)(rint((double)v.w * 1000.0) / 1000.0);
        x4[i] = v;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        x[i] = (float)(rint((double)x[i] * 1000.0) / 1000.0);
}

__global__ void mark_low_kernel(float* __restrict__ ps, const int64_t* __restrict__ idx, int64_t n_low,
                                int64_t n_elems) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_low; i += stride) {
        const int64_t k = idx[i];
        if (k >= 0 && k < n_elems) ps[k] = __builtin_nanf("");
    }
}

// (want_excl, want_ps, q3) -> one of the five <WE, WP, Q3> instantiations a tile kernel has: f is called with three
// std::integral_constant<bool, ...> arguments.  Exclusion sums alone have nothing to quantise: q3 is ignored there
template <typename F>
int ps_with_flags(bool wexcl, bool wps, bool q3, F&& f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (wexcl && wps) return q3 ? f(yes, yes, yes) : f(yes, yes, no);
    if (wexcl) return f(yes, no, no);
    return q3 ? f(no, yes, yes) : f(no, yes, no);
}

template <int VEC, bool WE, bool WP, bool Q3, int ABL>
int launch_ps_one(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid) {
    SD_LAUNCH_LDS(ctx, "ps_tile_kernel", (ps_tile_kernel<VEC, WE, WP, Q3, ABL>), grid, dim3(threads), lds, a);
    return SDICE_OK;
}

template <bool CH, bool WE, bool WP, bool Q3>
int launch_ps_v3_one(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid) {
    SD_LAUNCH_LDS(ctx, "ps_tile_v3_kernel", (ps_tile_v3_kernel<CH, WE, WP, Q3>), grid, dim3(threads), lds, a);
    return SDICE_OK;
}
template <bool CH>
int launch_ps_v3(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid, bool wexcl, bool wps, bool q3) {
    return ps_with_flags(wexcl, wps, q3, [&](auto we, auto wp, auto q) {
        return launch_ps_v3_one<CH, decltype(we)::value, decltype(wp)::value, decltype(q)::value>(ctx, a, threads, lds, grid);
    });
}

template <bool WE, bool WP, bool Q3>
int launch_ps_w16_one(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid) {
    // (the context profile books it under the name of the register-staged kernels: one entry for "the PS tile kernel
    //  of vector tables", which is what the benchmark's roofline line asks for; sdice_ps_last_plan tells them apart)
    SD_LAUNCH_LDS(ctx, "ps_tile_v3_kernel", (ps_tile_w16_kernel<WE, WP, Q3>), grid, dim3(threads), lds, a);
    return SDICE_OK;
}
int launch_ps_w16(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid, bool wexcl, bool wps, bool q3) {
    return ps_with_flags(wexcl, wps, q3, [&](auto we, auto wp, auto q) {
        return launch_ps_w16_one<decltype(we)::value, decltype(wp)::value, decltype(q)::value>(ctx, a, threads, lds, grid);
    });
}

template <int VEC>
int launch_ps(sdice_ctx* ctx, const PsArgs& a, int threads, size_t lds, dim3 grid, bool wexcl, bool wps, bool q3, int abl) {
    if (abl && VEC == 4 && !wexcl && wps && !q3) {        // timing experiments (one shape only)
        if (abl & 8) return launch_ps_one<4, false, true, false, 8>(ctx, a, threads, lds, grid);
        switch (abl & 7) {
            case 1: return launch_ps_one<4, false, true, false, 1>(ctx, a, threads, lds, grid);
            case 2: return launch_ps_one<4, false, true, false, 2>(ctx, a, threads, lds, grid);
            case 3: return launch_ps_one<4, false, true, false, 3>(ctx, a, threads, lds, grid);
            case 4: return launch_ps_one<4, false, true, false, 4>(ctx, a, threads, lds, grid);
            case 5: return launch_ps_one<4, false, true, false, 5>(ctx, a, threads, lds, grid);
            case 6: return launch_ps_one<4, false, true, false, 6>(ctx, a, threads, lds, grid);
            default: return launch_ps_one<4, false, true, false, 7>(ctx, a, threads, lds, grid);
        }
    }
    return ps_with_flags(wexcl, wps, q3, [&](auto we, auto wp, auto q) {
        return launch_ps_one<VEC, decltype(we)::value, decltype(wp)::value, decltype(q)::value, 0>(ctx, a, threads, lds, grid);
    });
}

}  // namespace

extern "C" int sdice_ps_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_counts,
                            const int64_t* d_row_ptr, const int32_t* d_col, int64_t* d_excl, float* d_ps) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(n < (int64_t)1 << 31, "n must be < 2^31 (int32 row indices)");
    SD_ARG(d_excl || d_ps, "both outputs are NULL");
    if (n == 0 || s == 0) return SDICE_OK;
    SD_ARG(d_counts && d_row_ptr, "NULL input");
    SD_HIP(hipSetDevice(ctx->device));

    SdPsFacts f;
    f.n = n; f.s = s;
    f.aligned = ((uintptr_t)d_counts % 16 == 0) && (!d_ps || (uintptr_t)d_ps % 16 == 0) && (!d_excl || (uintptr_t)d_excl % 16 == 0);
    f.want_excl = d_excl != nullptr; f.want_ps = d_ps != nullptr;
    f.ctx_list = d_col != nullptr && d_col == ctx->d_col;
    f.reach_rows_match = ctx->reach_n == n;
    f.have_reach_words = ctx->d_reach != nullptr;
    f.cluster_reach = ctx->cluster_reach;
    SdPsPlan pl;                                           // tile shape, kernel generation, grid: psplan.cpp
    SD_TRY(sd_ps_launch_plan(ctx->params, f, &pl));
    {
        const int32_t fields[SDICE_PS_PLAN_FIELDS] = {pl.kern, pl.vec, pl.chunk_cols, pl.tile_rows, pl.halo, pl.n_tiles, pl.n_chunks,
                                                      pl.lv_shift, pl.tiles_per_xcd, pl.use_reach, pl.nt, pl.prio, pl.q3, pl.threads};
        std::copy(fields, fields + SDICE_PS_PLAN_FIELDS, ctx->ps_plan);     // (test support: sdice_ps_last_plan)
        ctx->ps_planned = true;
    }

    PsArgs a;
    a.counts = d_counts; a.row_ptr = d_row_ptr; a.col = d_col; a.excl = d_excl; a.ps = d_ps;
    a.n = n; a.s = s;
    a.tile_rows = pl.tile_rows;
    a.halo = pl.halo;
    a.chunk_cols = pl.chunk_cols;
    a.col_cap = pl.col_cap;
    a.n_tiles = pl.n_tiles;
    a.tiles_per_xcd = pl.tiles_per_xcd;
    a.n_chunks = pl.n_chunks;
    a.prio = pl.prio;
    a.nt = pl.nt;
    a.reach = pl.use_reach ? ctx->d_reach : nullptr;
    a.lv_shift = pl.lv_shift;
    const size_t lds_bytes = (size_t)pl.lds_bytes;
    const dim3 grid((unsigned)pl.grid);
    if (pl.kern == PS_W16_KERN) return launch_ps_w16(ctx, a, pl.threads, lds_bytes, grid, f.want_excl, f.want_ps, pl.q3);
    if (pl.kern == 0) return pl.n_chunks == 1 && pl.chunk_cols == s ? launch_ps_v3<false>(ctx, a, pl.threads, lds_bytes, grid, f.want_excl, f.want_ps, pl.q3)
                                                                    : launch_ps_v3<true>(ctx, a, pl.threads, lds_bytes, grid, f.want_excl, f.want_ps, pl.q3);
    if (pl.vec == 4) return launch_ps<4>(ctx, a, pl.threads, lds_bytes, grid, f.want_excl, f.want_ps, pl.q3, pl.ablate);
    return launch_ps<1>(ctx, a, pl.threads, lds_bytes, grid, f.want_excl, f.want_ps, pl.q3, pl.ablate);
}

// Test support: which path the last launch took (the fields and their order: sdice.h).
extern "C" int sdice_ps_last_plan(sdice_ctx* ctx, int32_t* out, int32_t cap, int32_t* n_fields) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(cap >= 0 && (out || cap == 0), "bad arguments");
    if (!ctx->ps_planned) {
        sdice_set_error("%s: no sdice_ps_dev launch yet", __func__);
        return SDICE_ERR_STATE;
    }
    if (n_fields) *n_fields = SDICE_PS_PLAN_FIELDS;
    for (int i = 0; i < cap && i < SDICE_PS_PLAN_FIELDS; ++i) out[i] = ctx->ps_plan[i];
    return SDICE_OK;
}

int sd_check_csr(const char* who, int64_t n_out, int64_t n_rows, const int64_t* row_ptr, const int32_t* col) {
    const int64_t nnz = row_ptr[n_out];
    const char* bad = nullptr;
    if (row_ptr[0] != 0 || nnz < 0) bad = "row_ptr must start at 0 and be non-decreasing";
    else if (nnz != 0 && !col) bad = "col is NULL";
    for (int64_t i = 0; i < n_out && !bad; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) bad = "row_ptr must be non-decreasing";
    for (int64_t k = 0; k < nnz && !bad; ++k)
        if (col[k] < 0 || col[k] >= n_rows) bad = "col index out of range";
    if (!bad) return SDICE_OK;
    sdice_set_error("%s: %s", who, bad);
    return SDICE_ERR_ARG;
}

extern "C" int sdice_ps(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* counts,
                        const int64_t* row_ptr, const int32_t* col, int64_t* excl, float* ps) {
    SD_ARG(ctx, "ctx is NULL");
    SD_ARG(n >= 0 && s >= 0, "negative size");
    SD_ARG(excl || ps, "both outputs are NULL");
    if (n == 0 || s == 0) return SDICE_OK;
    SD_ARG(counts && row_ptr, "NULL input");
    SD_TRY(sd_check_csr(__func__, n, n, row_ptr, col));
    const int64_t cells = n * s;
    HostStaging st(ctx);
    int32_t *d_counts, *d_col;
    int64_t *d_rp, *d_excl = nullptr;
    float* d_ps = nullptr;
    SD_TRY(st.upload(&d_counts, counts, cells));
    SD_TRY(st.upload(&d_rp, row_ptr, n + 1));
    SD_TRY(st.upload(&d_col, col, row_ptr[n]));          // (nnz == 0: a valid empty buffer, never NULL)
    if (excl) SD_TRY(st.alloc(&d_excl, cells));
    if (ps) SD_TRY(st.alloc(&d_ps, cells));
    SD_TRY(sdice_ps_dev(ctx, n, s, d_counts, d_rp, d_col, d_excl, d_ps));
    if (excl) SD_TRY(st.download(excl, d_excl, cells));
    if (ps) SD_TRY(st.download(ps, d_ps, cells));
    return SDICE_OK;
}

extern "C" int sdice_quantize3_dev(sdice_ctx* ctx, int64_t n_elems, float* d_ps_inout) {
    SD_ARG(ctx && n_elems >= 0, "bad arguments");
    if (n_elems == 0) return SDICE_OK;
    SD_ARG(d_ps_inout && (uintptr_t)d_ps_inout % 4 == 0, "pointer must be a float pointer (4-byte aligned)");
    int64_t blocks = sd_ceil_div(sd_ceil_div(n_elems, 4), 256);
    if (blocks > 2048) blocks = 2048;
    SD_LAUNCH(ctx, "quantize3_kernel", quantize3_kernel, dim3((unsigned)blocks), dim3(256), 0, d_ps_inout, n_elems);
    return SDICE_OK;
}

extern "C" int sdice_quantize3(sdice_ctx* ctx, int64_t n_elems, float* ps_inout) {
    SD_ARG(ctx && n_elems >= 0, "bad arguments");
    if (n_elems == 0) return SDICE_OK;
    SD_ARG(ps_inout, "NULL pointer");
    HostStaging st(ctx);
    float* d;
    SD_TRY(st.upload(&d, ps_inout, n_elems));
    SD_TRY(sdice_quantize3_dev(ctx, n_elems, d));
    return st.download(ps_inout, d, n_elems);
}

extern "C" int sdice_mark_low_dev(sdice_ctx* ctx, int64_t n_elems, float* d_ps, const int64_t* d_low_idx,
                                  int64_t n_low) {
    SD_ARG(ctx && n_elems >= 0 && n_low >= 0, "bad arguments");
    if (n_low == 0) return SDICE_OK;
    SD_ARG(d_ps && d_low_idx, "NULL pointer");
    int64_t blocks = sd_ceil_div(n_low, 256);
    if (blocks > 2048) blocks = 2048;
    SD_LAUNCH(ctx, "mark_low_kernel", mark_low_kernel, dim3((unsigned)blocks), dim3(256), 0, d_ps, d_low_idx, n_low,
              n_elems);
    return SDICE_OK;
}

extern "C" int sdice_mark_low(sdice_ctx* ctx, int64_t n_elems, float* ps, const int64_t* low_idx, int64_t n_low) {
    SD_ARG(ctx && n_elems >= 0 && n_low >= 0, "bad arguments");
    if (n_low == 0) return SDICE_OK;
    SD_ARG(ps && low_idx, "NULL pointer");
    for (int64_t i = 0; i < n_low; ++i) SD_ARG(low_idx[i] >= 0 && low_idx[i] < n_elems, "low index out of range");
    HostStaging st(ctx);
    float* d;
    int64_t* di;
    SD_TRY(st.upload(&d, ps, n_elems));
    SD_TRY(st.upload(&di, low_idx, n_low));
    SD_TRY(sdice_mark_low_dev(ctx, n_elems, d, di, n_low));
    return st.download(ps, d, n_elems);
}
