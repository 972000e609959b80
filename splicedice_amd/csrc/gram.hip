// K15: sample-by-sample integer sums of a PS table over the rows two samples share (`sample_matrix`).  For the m listed
// columns, k_a(r) the 3-decimal key of ps[r, cols[a]] and v_a(r) = 1 when that value is not NaN:
//   shared[a,b] = sum v_a v_b     sum1[a,b] = sum k_a v_a v_b     sum2[a,b] = sum k_a^2 v_a v_b     prod[a,b] = sum k_a k_b v_a v_b
// Every sum is an integer, so the result does not depend on tile shape, row slices or the order of the atomic adds.
//
// gram_pack_kernel gathers the listed columns into a row-major uint16 key table (NaN = 0xFFFF, the convention of
// ranksum.hip), padded to a multiple of 64 columns with absent keys, and finds the first value that is not on the grid.
// gram_tile_kernel: a workgroup owns a 64 x 64 tile of (a, b) column pairs with a-tile <= b-tile and a slice of rows.  It
// stages 32 rows of both sides in LDS as three planes of 32-bit words (key with absent = 0, key^2, present flag), so the
// inner loop is six ds_read_b128 and 96 v_mad_u32_u24 per row and thread, nothing else: a thread keeps a 4 x 4 block of
// pairs (columns ty + 16 i against tx + 16 j, so that 16 lanes add into 128 contiguous bytes) with six 32-bit accumulators
// per pair -- shared, prod, a's sum1 / sum2 and b's sum1 / sum2; a diagonal tile computes both orders of a pair itself
// and leaves b's out (64 mads).  One product is at most 10^6 and 4096 * 10^6 < 2^32,
// so the accumulators are added into the 64-bit outputs (atomicAdd) every 4096 rows at the latest.  b's sums of an
// off-diagonal tile go to two scratch planes at [a, b]; gram_mirror_kernel writes the lower triangle from them.
#include <string.h>
#include "rowsum.h"

namespace {

constexpr int GR_MIN_COLS = 2;
constexpr int GR_MAX_COLS = 4096;
constexpr int GR_TILE = 64;          // columns of a tile side
constexpr int GR_ROWS = 32;          // rows staged in LDS per step
constexpr int GR_THREADS = 256;      // 16 x 16 threads, 4 x 4 pairs each
constexpr int GR_FOLD = 4096;        // rows a 32-bit accumulator holds
constexpr int GR_MIN_SLICE = 64;     // smallest row slice of a workgroup (gram.rows_per_wg is raised to a multiple of it)
constexpr unsigned GR_ABSENT = 0xFFFFu;
typedef unsigned long long u64;

// keys[r, a] = key of ps[r, cols[a]] for a < m, absent for m <= a < mp.  bad[0]: the smallest r * mp + a of a value that is
// neither NaN nor float32(k / 1000); bad[1]: the smallest a whose column index is outside [0, s).  Both start at ~0.
__global__ void __launch_bounds__(256) gram_pack_kernel(const float* __restrict__ ps, int64_t n, int s,
                                                        const int32_t* __restrict__ cols, int m, int mp, int lanes,
                                                        unsigned short* __restrict__ keys, u64* bad) {
    const int rows_per_block = 256 / lanes;
    const int sub = threadIdx.x / lanes, a0 = threadIdx.x % lanes;
    for (int64_t r = (int64_t)blockIdx.x * rows_per_block + sub; r < n; r += (int64_t)gridDim.x * rows_per_block) {
        const float* prow = ps + r * s;
        for (int a = a0; a < mp; a += lanes) {
            unsigned key = GR_ABSENT;
            if (a < m) {
                const int c = cols[a];
                if ((unsigned)c >= (unsigned)s) {
                    atomicMin(bad + 1, (u64)a);
                } else {
                    const float v = prow[c];
                    if (v == v) {
                        const PsKey k = key_of_ps(v);
                        if (k.exact()) key = (unsigned)k.key();
                        else atomicMin(bad, (u64)r * (u64)mp + (u64)a);
                    }
                }
            }
            keys[r * mp + a] = (unsigned short)key;
        }
    }
}

template <bool DIAG>
struct GramAcc {
    uint32_t S[4][4], P[4][4], A1[4][4], A2[4][4], B1[DIAG ? 1 : 4][DIAG ? 1 : 4], B2[DIAG ? 1 : 4][DIAG ? 1 : 4];
};

template <bool DIAG>
__device__ __forceinline__ void gram_zero(GramAcc<DIAG>& c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c.S[i][j] = c.P[i][j] = c.A1[i][j] = c.A2[i][j] = 0;
            if constexpr (!DIAG) c.B1[i][j] = c.B2[i][j] = 0;
        }
}

// acc += a * b on operands below 2^24: the one instruction.  (__umul24 + add becomes the same instruction behind a
// v_and_b32 0xffffff of every operand read from LDS, a quarter more vector issue in the row loop.)
__device__ __forceinline__ void gram_mad(uint32_t& acc, uint32_t a, uint32_t b) {
    asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

__device__ __forceinline__ void gram_add(u64* p, uint32_t v) {
    // (a copy the optimiser cannot see through: otherwise each accumulator lives in a 64-bit register pair with a zero high
    // half throughout the row loop, and the kernel spills)
    uint32_t w;
    asm volatile("v_mov_b32 %0, %1" : "=v"(w) : "v"(v));
    if (w) atomicAdd(p, (u64)w);
}

template <bool DIAG>
__device__ __forceinline__ void gram_flush(GramAcc<DIAG>& c, int a_base, int b_base, int m, u64* shared, u64* sum1, u64* sum2,
                                           u64* prod, u64* q1, u64* q2) {
    // (opaque to the optimiser: otherwise the 96 output addresses are formed ahead of the row loop and held in registers)
    asm volatile("" : "+v"(a_base), "+v"(b_base));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = a_base + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b_base + 16 * j;
            if (a < m && b < m) {
                const int64_t at = (int64_t)a * m + b;
                gram_add(shared + at, c.S[i][j]);
                gram_add(prod + at, c.P[i][j]);
                gram_add(sum1 + at, c.A1[i][j]);
                gram_add(sum2 + at, c.A2[i][j]);
                if constexpr (!DIAG) {
                    gram_add(q1 + at, c.B1[i][j]);
                    gram_add(q2 + at, c.B2[i][j]);
                }
            }
        }
    }
    gram_zero(c);
}

// LDS image of a step: [plane: key, key^2, present][side: a, b][row][slot]; column c of a tile side sits in slot
// (c & 15) * 4 + (c >> 4), so the four columns of a thread (c = t + 16 i) are one aligned 16-byte read
struct GramLds {
    uint32_t w[3][2][GR_ROWS][GR_TILE];
};

template <bool DIAG>
__device__ __forceinline__ void gram_tile(GramLds& L, const unsigned short* __restrict__ keys, int64_t r_begin, int64_t r_end,
                                          int m, int mp, int ta, int tb, u64* shared, u64* sum1, u64* sum2, u64* prod, u64* q1,
                                          u64* q2) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    GramAcc<DIAG> c;
    gram_zero(c);
    for (int64_t f0 = r_begin; f0 < r_end; f0 += GR_FOLD) {          // as many rows as the 32-bit accumulators hold
    const int64_t f_end = f0 + GR_FOLD < r_end ? f0 + GR_FOLD : r_end;
    for (int64_t r0 = f0; r0 < f_end; r0 += GR_ROWS) {
        __syncthreads();                             // the previous step's reads are done
#pragma unroll
        for (int it = 0; it < GR_ROWS * 32 / GR_THREADS; ++it) {
            const int idx = tid + GR_THREADS * it;
            const int row = idx >> 5, side = (idx >> 4) & 1, q = idx & 15;
            const int64_t r = r0 + row;
            uint2 w = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);         // rows past the slice are absent
            if (r < f_end) w = *reinterpret_cast<const uint2*>(keys + r * mp + (side ? tb : ta) * GR_TILE + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned k16 = ((e < 2 ? w.x : w.y) >> (16 * (e & 1))) & 0xFFFFu;
                const int col = q * 4 + e, slot = (col & 15) * 4 + (col >> 4);
                const unsigned v = k16 != GR_ABSENT ? 1u : 0u, k = v ? k16 : 0u;
                L.w[0][side][row][slot] = k;
                L.w[1][side][row][slot] = k * k;
                L.w[2][side][row][slot] = v;
            }
        }
        __syncthreads();
#pragma clang loop vectorize(disable)
#pragma unroll 2
        for (int r = 0; r < GR_ROWS; ++r) {
            const uint4 ak4 = *reinterpret_cast<const uint4*>(&L.w[0][0][r][ty * 4]);
            const uint4 aq4 = *reinterpret_cast<const uint4*>(&L.w[1][0][r][ty * 4]);
            const uint4 av4 = *reinterpret_cast<const uint4*>(&L.w[2][0][r][ty * 4]);
            const uint4 bk4 = *reinterpret_cast<const uint4*>(&L.w[0][1][r][tx * 4]);
            const uint4 bq4 = *reinterpret_cast<const uint4*>(&L.w[1][1][r][tx * 4]);
            const uint4 bv4 = *reinterpret_cast<const uint4*>(&L.w[2][1][r][tx * 4]);
            const uint32_t ak[4] = {ak4.x, ak4.y, ak4.z, ak4.w}, aq[4] = {aq4.x, aq4.y, aq4.z, aq4.w};
            const uint32_t av[4] = {av4.x, av4.y, av4.z, av4.w}, bk[4] = {bk4.x, bk4.y, bk4.z, bk4.w};
            const uint32_t bq[4] = {bq4.x, bq4.y, bq4.z, bq4.w}, bv[4] = {bv4.x, bv4.y, bv4.z, bv4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gram_mad(c.S[i][j], av[i], bv[j]);
                    gram_mad(c.P[i][j], ak[i], bk[j]);
                    gram_mad(c.A1[i][j], ak[i], bv[j]);
                    gram_mad(c.A2[i][j], aq[i], bv[j]);          // key^2 <= 10^6 < 2^24
                    if constexpr (!DIAG) {
                        gram_mad(c.B1[i][j], bk[j], av[i]);
                        gram_mad(c.B2[i][j], bq[j], av[i]);
                    }
                }
        }
    }
    gram_flush(c, ta * GR_TILE + ty, tb * GR_TILE + tx, m, shared, sum1, sum2, prod, q1, q2);
    }
}

// block = slice * tiles + t: the tile pairs of one row slice are neighbours in launch order and read the same key rows
__global__ void __launch_bounds__(GR_THREADS) gram_tile_kernel(const unsigned short* __restrict__ keys, int64_t n, int m,
                                                                int mp, int nt, int tiles, int64_t rows_per_wg, u64* shared,
                                                                u64* sum1, u64* sum2, u64* prod, u64* q1, u64* q2) {
    __shared__ __attribute__((aligned(16))) GramLds L;
    const int64_t slice = blockIdx.x / (unsigned)tiles;
    int rem = (int)(blockIdx.x % (unsigned)tiles), ta = 0;
    while (rem >= nt - ta) {
        rem -= nt - ta;
        ++ta;
    }
    const int tb = ta + rem;
    const int64_t r_begin = slice * rows_per_wg;
    const int64_t r_end = r_begin + rows_per_wg < n ? r_begin + rows_per_wg : n;
    if (ta == tb) gram_tile<true>(L, keys, r_begin, r_end, m, mp, ta, tb, shared, sum1, sum2, prod, q1, q2);
    else gram_tile<false>(L, keys, r_begin, r_end, m, mp, ta, tb, shared, sum1, sum2, prod, q1, q2);
}

// the entries below the diagonal tiles: shared and prod are symmetric, b's sums wait in q1 / q2 at [a, b]
__global__ void __launch_bounds__(256) gram_mirror_kernel(int m, u64* shared, u64* sum1, u64* sum2, u64* prod,
                                                          const u64* __restrict__ q1, const u64* __restrict__ q2) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (int64_t)m * m) return;
    const int a = (int)(at / m), b = (int)(at % m);
    if (a / GR_TILE >= b / GR_TILE) return;
    const int64_t to = (int64_t)b * m + a;
    shared[to] = shared[at];
    prod[to] = prod[at];
    sum1[to] = q1[at];
    sum2[to] = q2[at];
}

int gram_check_scalars(int64_t n, int32_t s, int32_t m) {
    SD_ARG(n >= 0 && s >= 0, "negative size");
    if (m < GR_MIN_COLS || m > GR_MAX_COLS) {
        sdice_set_error("sdice_sample_gram: %d columns listed, %d..%d are supported", (int)m, GR_MIN_COLS, GR_MAX_COLS);
        return SDICE_ERR_ARG;
    }
    SD_ARG(m <= s, "more columns listed than the table has (a column may be listed once)");
    return SDICE_OK;
}

}  // namespace

extern "C" int sdice_sample_gram_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t m,
                                     int64_t* d_shared, int64_t* d_sum1, int64_t* d_sum2, int64_t* d_prod) {
    SD_ARG(ctx, "ctx is NULL");
    SD_TRY(gram_check_scalars(n, s, m));
    SD_ARG(d_shared && d_sum1 && d_sum2 && d_prod, "NULL output");
    SD_ARG(d_cols && (d_ps || n == 0), "NULL input");
    SD_HIP(hipSetDevice(ctx->device));
    const size_t out_bytes = (size_t)m * m * sizeof(int64_t);
    int64_t* outs[4] = {d_shared, d_sum1, d_sum2, d_prod};
    if (n == 0) {
        for (int64_t* o : outs) SD_HIP(hipMemsetAsync(o, 0, out_bytes, ctx->stream));
        return SDICE_OK;
    }
    const int nt = (m + GR_TILE - 1) / GR_TILE, mp = nt * GR_TILE, tiles = nt * (nt + 1) / 2;
    const size_t key_bytes = (size_t)n * mp * sizeof(unsigned short);
    SD_TRY(ctx->arena.reserve(key_bytes + 2 * out_bytes + 4096, ctx->stream));
    unsigned short* keys = (unsigned short*)ctx->arena.alloc(key_bytes);
    u64* q1 = (u64*)ctx->arena.alloc(out_bytes);
    u64* q2 = (u64*)ctx->arena.alloc(out_bytes);
    u64* bad = (u64*)ctx->arena.alloc(2 * sizeof(u64));
    if (!keys || !q1 || !q2 || !bad) return SDICE_ERR_NOMEM;

    // ---- pre-pass: keys + the grid check, one read-back
    SD_HIP(hipMemsetAsync(bad, 0xFF, 2 * sizeof(u64), ctx->stream));
    {
        const int lanes = mp >= 256 ? 256 : 64;
        int64_t blocks = sd_ceil_div(n, 256 / lanes);
        const int64_t cap = (int64_t)ctx->n_cu * 32;
        if (blocks > cap) blocks = cap;
        SD_LAUNCH(ctx, "gram_pack_kernel", gram_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, d_ps, n, (int)s, d_cols,
                  (int)m, mp, lanes, keys, bad);
    }
    u64* hb = (u64*)ctx->h_pinned;
    SD_HIP(hipMemcpyAsync(hb, bad, 2 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    if (hb[1] != ~0ull) {
        sdice_set_error("sdice_sample_gram_dev: cols[%lld] is not a column of the table (0 .. %d)", (long long)hb[1], (int)s - 1);
        return SDICE_ERR_ARG;
    }
    if (hb[0] != ~0ull) {
        const int64_t r = (int64_t)(hb[0] / (u64)mp);
        const int a = (int)(hb[0] % (u64)mp);
        int32_t col = -1;
        float v = 0.0f;
        SD_HIP(hipMemcpy(&col, d_cols + a, sizeof(col), hipMemcpyDeviceToHost));
        SD_HIP(hipMemcpy(&v, d_ps + r * s + col, sizeof(v), hipMemcpyDeviceToHost));
        sdice_set_error("sdice_sample_gram: row %lld, column %d holds %.9g, which is neither NaN nor a 3-decimal PS value "
                        "float32(k / 1000), k = 0 .. 1000", (long long)r, (int)col, (double)v);
        return SDICE_ERR_ARG;
    }

    // ---- the sums
    for (int64_t* o : outs) SD_HIP(hipMemsetAsync(o, 0, out_bytes, ctx->stream));
    if (nt > 1) {
        SD_HIP(hipMemsetAsync(q1, 0, out_bytes, ctx->stream));
        SD_HIP(hipMemsetAsync(q2, 0, out_bytes, ctx->stream));
    }
    int64_t rows_per_wg = ctx->param(SD_P_GRAM_ROWS_PER_WG);
    if (rows_per_wg <= 0) {
        // as long a slice as a 32-bit accumulator holds (one round of atomics per workgroup), shorter while the grid
        // would not fill the chip a few times over
        rows_per_wg = GR_FOLD;
        while (rows_per_wg > 256 && sd_ceil_div(n, rows_per_wg) * tiles < (int64_t)ctx->n_cu * 12) rows_per_wg >>= 1;
    }
    rows_per_wg = sd_ceil_div(rows_per_wg, GR_MIN_SLICE) * GR_MIN_SLICE;
    while (sd_ceil_div(n, rows_per_wg) * tiles > (int64_t)1 << 30) rows_per_wg *= 2;
    const int64_t blocks = sd_ceil_div(n, rows_per_wg) * tiles;
    SD_LAUNCH(ctx, "gram_tile_kernel", gram_tile_kernel, dim3((unsigned)blocks), dim3(GR_THREADS), 0, keys, n, (int)m, mp, nt,
              tiles, rows_per_wg, (u64*)d_shared, (u64*)d_sum1, (u64*)d_sum2, (u64*)d_prod, q1, q2);
    if (nt > 1)
        SD_LAUNCH(ctx, "gram_mirror_kernel", gram_mirror_kernel, dim3((unsigned)sd_ceil_div((int64_t)m * m, 256)), dim3(256), 0,
                  (int)m, (u64*)d_shared, (u64*)d_sum1, (u64*)d_sum2, (u64*)d_prod, q1, q2);
    return SDICE_OK;
}

extern "C" int sdice_sample_gram(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t m,
                                 int64_t* shared, int64_t* sum1, int64_t* sum2, int64_t* prod) {
    SD_ARG(ctx, "ctx is NULL");
    SD_TRY(gram_check_scalars(n, s, m));
    SD_ARG(cols, "column list is NULL");
    SD_TRY(check_columns(__func__, {cols}, m, s, "column index out of range", "a column may be listed once"));
    SD_ARG(shared && sum1 && sum2 && prod, "NULL output");
    SD_ARG(ps || n == 0, "ps is NULL");
    const int64_t mm = (int64_t)m * m;
    if (n == 0) {
        for (int64_t* o : {shared, sum1, sum2, prod}) memset(o, 0, (size_t)mm * sizeof(int64_t));
        return SDICE_OK;
    }
    HostStaging st(ctx);
    float* d_ps;
    int32_t* dc;
    int64_t *d_shared, *d_sum1, *d_sum2, *d_prod;
    SD_TRY(st.upload(&d_ps, ps, n * s));
    SD_TRY(st.upload(&dc, cols, m));
    st.result(&d_shared, shared, mm);
    st.result(&d_sum1, sum1, mm);
    st.result(&d_sum2, sum2, mm);
    st.result(&d_prod, prod, mm);
    SD_TRY(st.alloc_results());
    SD_TRY(sdice_sample_gram_dev(ctx, n, s, d_ps, dc, m, d_shared, d_sum1, d_sum2, d_prod));
    return st.download_results();
}
