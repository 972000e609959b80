/*
 * sdice.h -- C ABI of libsplicedice_hip.so: the MI355X (gfx950) hot path of splicedice.
 *
 * The reference (BrooksLabUCSC/splicedice) is pure Python and has NO FFI/plugin
 * interface; its only extension seam is add_cmd(name, add_parser, run_with)
 * (splicedice/__main__.py:17-33).  This header is therefore the boundary a maintainer
 * would bind with ctypes from inside the four hot `run_with` functions; each entry
 * point cites the reference loop it replaces (file:line relative to the reference
 * checkout).  See INTEGRATION.md for the ctypes stub.
 *
 * Conventions
 *  - plain C, every function returns int status (0 = ok, <0 = error);
 *    sdice_last_error() returns a thread-local message; no exceptions cross the ABI.
 *  - host entry points (no suffix): caller owns all host buffers (C-contiguous,
 *    pointer + explicit sizes); the call copies in, runs the HIP kernels, copies out and
 *    is synchronous on return.
 *  - device entry points (`_dev`): all pointers are device pointers obtained from
 *    sdice_dmalloc; work is enqueued on the context's HIP stream and NOT synchronised
 *    (call sdice_sync).  These keep tables resident in HBM between stages.
 *  - a context is bound to one GPU and used from one thread at a time.
 *  - there is no CPU backend: without a usable HIP device sdice_ctx_create fails.
 */
#ifndef SDICE_H
#define SDICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdice_ctx sdice_ctx;

#define SDICE_OK          0
#define SDICE_ERR_ARG    -1
#define SDICE_ERR_HIP    -2
#define SDICE_ERR_NOMEM  -3
#define SDICE_ERR_STATE  -4
#define SDICE_ERR_COMM   -5

#define SDICE_ABI_VERSION 1

/* ---- lifecycle / errors ---------------------------------------------------------- */
int         sdice_version(void);
const char* sdice_last_error(void);
int         sdice_ctx_create(int device_ordinal, sdice_ctx** out);
int         sdice_ctx_destroy(sdice_ctx* ctx);
int         sdice_sync(sdice_ctx* ctx);
/* synchronise and hand the context's cached device scratch (the per-call arena, kept between calls) back to the
 * driver; a long-lived context calls it after an unusually large job (no reference counterpart: the reference's
 * numpy temporaries die with each call, e.g. pairwise_fisher.py:187-191) */
int         sdice_trim(sdice_ctx* ctx);
/* name: caller buffer of name_cap bytes; any out pointer may be NULL */
int         sdice_device_info(sdice_ctx* ctx, char* name, int name_cap, int* compute_units,
                              int64_t* hbm_bytes);

/* ---- device memory (for the _dev entry points) ------------------------------------ */
int sdice_dmalloc(sdice_ctx* ctx, int64_t bytes, void** dptr);
int sdice_dfree(sdice_ctx* ctx, void* dptr);
int sdice_h2d(sdice_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
int sdice_d2h(sdice_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
int sdice_dmemset(sdice_ctx* ctx, void* dptr, int value, int64_t bytes);

/* ---- clustering: replaces SPLICEDICE.getClusters (SPLICEDICE.py:230-255), its twin
 *      counts_to_ps.determine_clusters (counts_to_ps.py:16-41) and the junctionIndex
 *      sort (SPLICEDICE.py:96).
 *  in : n junctions as parallel arrays, any order, all distinct (a duplicate is reported as
 *       SDICE_ERR_ARG: the reference holds the junctions in a set / dict, SPLICEDICE.py:156).
 *       chrom_rank = dense rank of the chromosome name under Python string sort,
 *       0 <= left <= right < 2^31, strand 0 = '+', 1 = '-'.
 *  out: row_of[n]   output row of input junction i = its rank in
 *                   (chrom, left, right, strand) order (SPLICEDICE.py:96);
 *       row_ptr[n+1], col[nnz]: per output row, the rows of all junctions on the same
 *                   chromosome+strand whose closed interval overlaps it
 *                   (prior.right >= cur.left, SPLICEDICE.py:250), in the reference's
 *                   list order: earlier-in-sweep overlaps most recent first, then
 *                   later ones in sweep order.
 *  The column list lives in the context until the next sdice_cluster* call and is
 *  fetched with sdice_cluster_col (host) / sdice_cluster_col_dev (device pointer).
 */
int sdice_cluster(sdice_ctx* ctx, int64_t n, const int32_t* chrom_rank, const int32_t* left,
                  const int32_t* right, const int8_t* strand,
                  int32_t* row_of, int64_t* row_ptr, int64_t* nnz);
int sdice_cluster_col(sdice_ctx* ctx, int32_t* col, int64_t capacity);
/* Device variant.  nnz != NULL: synchronous on return (*nnz = list length; invalid or duplicate
 * junctions are reported here).  nnz == NULL: ASYNCHRONOUS -- the whole chain (sort, row order,
 * lists) is enqueued with no host round trip, so that a dependent sdice_ps_dev can be enqueued right
 * behind it; validation results, nnz and the list capacity check are then reported by the next
 * sdice_sync / sdice_cluster_status / sdice_cluster_col_dev(nnz != NULL) (deferred-error semantics,
 * as for asynchronous HIP work).  A chain that failed leaves row_ptr all zero, so dependent launches
 * stay in bounds.  The list buffer holds at least 16 entries per junction; one synchronous call sizes
 * it for denser data. */
int sdice_cluster_dev(sdice_ctx* ctx, int64_t n, const int32_t* d_chrom_rank,
                      const int32_t* d_left, const int32_t* d_right, const int8_t* d_strand,
                      int32_t* d_row_of, int64_t* d_row_ptr, int64_t* nnz /* host out, may be NULL */);
/* resolves a pending asynchronous sdice_cluster_dev (synchronises); nnz / reach (largest
 * |row(neighbour) - row|) may be NULL */
int sdice_cluster_status(sdice_ctx* ctx, int64_t* nnz, int32_t* reach);
int sdice_cluster_col_dev(sdice_ctx* ctx, const int32_t** d_col, int64_t* nnz);

/* ---- PS: replaces SPLICEDICE.calculatePsi (SPLICEDICE.py:297-310), counts_to_ps
 *      writePsValues' arithmetic (counts_to_ps.py:63-68) and pairwise's exclusion
 *      gather (pairwise_fisher.py:158-160).
 *  counts[n,s] int32 row-major, rows in output-row order; CSR as above (any valid CSR
 *  over rows is accepted, e.g. one parsed from an _allClusters.tsv).
 *  excl[n,s] int64 (optional, may be NULL): sum of the count rows of the neighbours.
 *  ps[n,s] float32 (optional, may be NULL) = float32(double(incl) / double(incl+excl));
 *  0/0 -> NaN.
 */
int sdice_ps(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* counts,
             const int64_t* row_ptr, const int32_t* col, int64_t* excl, float* ps);
int sdice_ps_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_counts,
                 const int64_t* d_row_ptr, const int32_t* d_col, int64_t* d_excl, float* d_ps);

/* ---- PS of a float64 count table: counts_to_ps.writePsValues (counts_to_ps.py:58-70) as written --
 *      the table is parsed with dtype=float (:50), so fractional / normalised counts are legal there.
 *  counts[n_rows,s] float64 row-major; rows 0..n_out-1 get a result, rows n_out..n_rows-1 are
 *  sources only (overlaps that are named in a cluster list but are not cluster keys themselves);
 *  row_ptr[n_out+1], col[nnz] with 0 <= col < n_rows.
 *  ps[n_out,s] float64 = counts[r] / (counts[r] + counts[col[k0]] + counts[col[k0+1]] + ...), the sum
 *  taken left to right in list order, one IEEE addition at a time; 0/0 -> NaN, x/0 -> inf.
 */
int sdice_ps_f64(sdice_ctx* ctx, int64_t n_out, int64_t n_rows, int32_t s, const double* counts,
                 const int64_t* row_ptr, const int32_t* col, double* ps);
int sdice_ps_f64_dev(sdice_ctx* ctx, int64_t n_out, int64_t n_rows, int32_t s, const double* d_counts,
                     const int64_t* d_row_ptr, const int32_t* d_col, double* d_ps);

/* ---- exclusion sums of a float64 count table: `pairwise` on fractional counts.  pairwise_fisher.py:46-61 parses the
 *      table with dtype=float and :158-160 adds the rows named in the event's cluster, np.sum(counts[mask], axis=0):
 *      one IEEE addition per row in TABLE order; scipy.stats.fisher_exact then truncates the float sums (and the
 *      float inclusion counts) to int64.  Same shapes as sdice_ps_f64; excl[n_out,s] float64 =
 *      counts[col[k0]] + counts[col[k0+1]] + ... left to right (0.0 for an empty list).  The caller lists the rows of
 *      every event in ascending (table) order and truncates.
 */
int sdice_excl_f64(sdice_ctx* ctx, int64_t n_out, int64_t n_rows, int32_t s, const double* counts,
                   const int64_t* row_ptr, const int32_t* col, double* excl);
int sdice_excl_f64_dev(sdice_ctx* ctx, int64_t n_out, int64_t n_rows, int32_t s, const double* d_counts,
                       const int64_t* d_row_ptr, const int32_t* d_col, double* d_excl);

/* --lowCoverageNan (SPLICEDICE.py:307-309): ps[low_idx[i]] = NaN, flat indices r*s+c */
int sdice_mark_low(sdice_ctx* ctx, int64_t n_elems, float* ps, const int64_t* low_idx,
                   int64_t n_low);
int sdice_mark_low_dev(sdice_ctx* ctx, int64_t n_elems, float* d_ps, const int64_t* d_low_idx,
                       int64_t n_low);

/* the `_allPS.tsv` text round trip between quant and compare_sample_sets:
 * f'{x:.3f}' (SPLICEDICE.py:353) re-read as float32 (compareSampleSets.py:202).  The device variant takes any
 * 4-byte-aligned float pointer, e.g. a row-range view of a resident table with odd s. */
int sdice_quantize3(sdice_ctx* ctx, int64_t n_elems, float* ps_inout);
int sdice_quantize3_dev(sdice_ctx* ctx, int64_t n_elems, float* d_ps_inout);

/* ---- compare_sample_sets: replaces the per-row loop compareSampleSets.py:216-232
 *      (NaN drop, <3 skip, scipy.stats.ranksums, np.median x2, np.mean x2).
 *  ps[n,s] float32; g1[n1], g2[n2] column indices (table order).
 *  Outputs are un-compacted, one slot per row: tested[n] (1 = row was tested),
 *  p[n] float64, med1/med2/mean1/mean2/delta[n] float32 (0 where not tested);
 *  z[n] float64 optional (NULL to skip).  The host compacts in row order.
 *  Any float32 values, NaN meaning "no value": signed zeros (one tie group), subnormals (distinct values), values
 *  outside [0, 1] and infinities included; rows of 3-decimal PS values take the 16-bit-key / histogram kernels, every
 *  other row the sorting kernels, with the same results.  A row whose kept values are all equal is tested with z = 0,
 *  p = 1.  mean1 / mean2 are np.mean of a group's kept values bit for bit (+0.0 for a group of -0.0 values, +-inf or
 *  NaN where the float32 sum overflows or meets inf - inf), med1 / med2 np.median by value; p = erfc(|z| / sqrt 2)
 *  within 1e-9 relative down to 1e-280, below 2e-280 under that and 0 past the float64 range.  Groups of up to 4096
 *  columns. */
int sdice_ranksum(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps,
                  const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2,
                  uint8_t* tested, double* p, double* z, float* med1, float* med2,
                  float* mean1, float* mean2, float* delta);
int sdice_ranksum_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps,
                      const int32_t* d_g1, int32_t n1, const int32_t* d_g2, int32_t n2,
                      uint8_t* d_tested, double* d_p, double* d_z, float* d_med1, float* d_med2,
                      float* d_mean1, float* d_mean2, float* d_delta);

/* ---- compare_sample_sets -mx: Kruskal-Wallis H test across k sets, scipy.stats.kruskal per row under the row rules
 *      above (per set: NaN drop; the row is tested when every set keeps >= 3 values).
 *  cols: the column indices of all sets back to back; set_ptr[k+1]: CSR-style offsets into cols (set i is
 *  cols[set_ptr[i] .. set_ptr[i+1])).  2 <= k <= 64, every set non-empty, a column in one set only, at most 16384
 *  selected columns; otherwise SDICE_ERR_ARG before any launch, outputs untouched.  set_ptr is a HOST array in both
 *  calls (launch metadata, like n1 / n2 above); the host call also checks the indices and the one-set rule.
 *  Outputs, one slot per row: tested[n], p[n] = chi2.sf(H, k-1) and h[n] float64 (h optional, NULL to skip),
 *  med[k][n] / mean[k][n] float32 SET-major (np.median / np.mean of a set's kept values), delta[n] = largest minus
 *  smallest set median; 0 where not tested.  A row whose kept values are all equal is tested with H = 0, p = 1
 *  (scipy raises there).  Any finite float32 values; rows of 3-decimal PS values take the histogram kernel. */
int sdice_kruskal(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                  const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* h,
                  float* med, float* mean, float* delta);
int sdice_kruskal_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                      const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_h,
                      float* d_med, float* d_mean, float* d_delta);

/* ---- compare_sample_sets -mx --posthoc: sdice_kruskal with Dunn's test for every pair of sets, from the same joint
 *      ranking.  Inputs, row rules, checks and refusals are sdice_kruskal's, and tested, p, h, med, mean, delta are its
 *      outputs bit for bit; in addition SDICE_ERR_ARG for k > SDICE_DUNN_MAX_SETS and for a NULL pair_z.
 *  Pairs i < j in the order (0,1), (0,2), .., (k-2,k-1), m = k (k - 1) / 2 of them; pair_z / pair_p / pair_padj are float64
 *  PAIR-major [m][n] (pair_p and pair_padj optional, NULL to skip).  With R_i-bar the mean joint mid-rank of set i, N the
 *  kept values of the row and t the sizes of its tie groups:
 *    z = (R_i-bar - R_j-bar) / sqrt(sigma2 (1 / n_i + 1 / n_j)),  sigma2 = (N^3 - N - sum(t^3 - t)) / (12 (N - 1)),
 *  no continuity correction, z > 0 where set i ranks above set j, within 1 ulp of the correctly rounded value and +0.0
 *  where the two mean ranks are equal; p = erfc(|z| / sqrt 2), two-sided, to the p bars of sdice_ranksum; padj: Holm's
 *  step-down over the row's m p-values, padj_(r) = min(1, max_{t <= r} (m - t + 1) p_(t)) over the p's in ascending order,
 *  equal p's get equal padj.  A row whose kept values are all equal is tested with z = 0, p = 1, padj = 1 in every pair; a
 *  row that is not tested carries 0 in every pair slot. */
#define SDICE_DUNN_MAX_SETS 11 /* 55 pairs: one pair per lane of a 64-lane wave (sdice_kruskal itself takes 64 sets) */
int sdice_kruskal_dunn(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                       const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* h,
                       float* med, float* mean, float* delta, double* pair_z, double* pair_p, double* pair_padj);
int sdice_kruskal_dunn_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                           const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_h,
                           float* d_med, float* d_mean, float* d_delta, double* d_pair_z, double* d_pair_p,
                           double* d_pair_padj);

/* ---- compare_sample_sets -mx --trend: Jonckheere-Terpstra trend test across k ORDERED sets (set 0 < set 1 < ... as
 *      given) under the row rules, the inputs, the checks and the refusals of sdice_kruskal above.
 *  J = sum over the set pairs i < j of #{x in i, y in j: x < y} + #{x == y} / 2; E[J] = sum_{i<j} n_i n_j / 2; Var(J) is the
 *  exact conditional (permutation) variance given the row's ties, evaluated in integers; z = (J - E[J]) / sqrt(Var J)
 *  without a continuity correction, z > 0 when the values rise along the set order; p = erfc(|z| / sqrt 2), two-sided,
 *  asymptotic only.  Ties are by float32 equality (-0.0 == +0.0, subnormals are distinct values).
 *  Outputs, one slot per row: tested[n], p[n], z[n] float64, j[n] float64 = J exactly (optional, NULL to skip);
 *  med[k][n] / mean[k][n] SET-major and delta[n] are those of sdice_kruskal bit for bit; 0 where not tested.  A row whose
 *  kept values are all equal is tested with z = 0, p = 1, J = E[J].  Any finite float32 values; rows of 3-decimal PS
 *  values take the histogram kernel. */
int sdice_jonckheere(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                     const int32_t* set_ptr, int32_t k, uint8_t* tested, double* p, double* z, double* j,
                     float* med, float* mean, float* delta);
int sdice_jonckheere_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                         const int32_t* set_ptr, int32_t k, uint8_t* d_tested, double* d_p, double* d_z, double* d_j,
                         float* d_med, float* d_mean, float* d_delta);

/* ---- compare_sample_sets --repeated: Friedman's test across k MATCHED sets (the same m subjects in every set), per row
 *      scipy.stats.friedmanchisquare under the row rules below; with --trend Page's L test over the sets as ORDERED.
 *  cols is SET-major: cols[j m + q] is the column of set j (0-based) for subject q.  2 <= k <= 64, 1 <= m <= 4096,
 *  k m <= 16384, a column at most once; otherwise SDICE_ERR_ARG before any launch, outputs untouched (the host call checks
 *  the index range and the one-appearance rule, the _dev call k, m, k m and k m <= s).  Values are finite float32 or NaN.
 *  Per row: block q (subject q's k values) is kept when none of them is NaN; with fewer than 3 kept blocks (m') the row is
 *  not tested and every output slot is 0.  blocks[n] int32 = m' (optional, NULL to skip).  med[k][n] / mean[k][n] float32
 *  SET-major are np.median / np.mean of set j's values over the KEPT blocks in subject order, bit for bit as in
 *  sdice_signedrank; delta[n] = largest minus smallest set median in float32.
 *  Ranks are taken inside a block, as integers: r2(q, j) = 2 #{l: x_ql < x_qj} + #{l: x_ql == x_qj} + 1 (twice the
 *  mid-rank; ties by float32 equality, -0.0 == +0.0, subnormals are distinct values), D_j = sum_q r2(q, j) - m'(k + 1),
 *  C = sum over blocks and tie groups of t^3 - t, den = m'(k^3 - k) - C.  No value is subtracted from another: 3-decimal
 *  rows and others are one path.
 *  sdice_friedman: q[n] = Q = 3 (k - 1) sum D_j^2 / den and w[n] = Kendall's W = 3 sum D_j^2 / (m' den) = Q / (m'(k - 1)),
 *  float64, each the correctly rounded quotient of two exact integers (both optional, NULL to skip); p[n] = chi2.sf(Q,
 *  k - 1), to the p bars of sdice_kruskal.  Always the chi-square approximation: there is no exact form here.
 *  sdice_page: the sets are ORDERED as given.  l[n] = L = sum_j (j + 1) R_j float64, exact (optional, NULL to skip); E[L] =
 *  m' k (k + 1)^2 / 4, Var L = k (k + 1) den / 144, the conditional (within-block permutation) variance given the row's
 *  ties (scipy.stats.page_trend_test uses the untied variance: the two differ on tied rows, on purpose); z[n] = (L - E[L])
 *  / sqrt(Var L) = 6 sum_j (j + 1) D_j / sqrt(k (k + 1) den), no continuity correction, within 2 ulp of the correctly
 *  rounded value, > 0 where the values rise along the set order, +0.0 where L = E[L]; the call on the reversed sets gives
 *  -z bit for bit.  p[n] = erfc(|z| / sqrt 2), two-sided, asymptotic only, to the p bars of sdice_ranksum.  z is required.
 *  A row whose kept blocks are all fully tied (den = 0) is tested with Q = W = z = 0 and p = 1 (scipy: NaN).  Permuting
 *  the sets or the subjects leaves Q, W, p and |z| bit for bit. */
int sdice_friedman(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t k, int32_t m,
                   uint8_t* tested, double* p, double* q, double* w, int32_t* blocks, float* med, float* mean,
                   float* delta);
int sdice_friedman_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t k,
                       int32_t m, uint8_t* d_tested, double* d_p, double* d_q, double* d_w, int32_t* d_blocks,
                       float* d_med, float* d_mean, float* d_delta);
int sdice_page(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t k, int32_t m,
               uint8_t* tested, double* p, double* z, double* l, int32_t* blocks, float* med, float* mean,
               float* delta);
int sdice_page_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t k,
                   int32_t m, uint8_t* d_tested, double* d_p, double* d_z, double* d_l, int32_t* d_blocks,
                   float* d_med, float* d_mean, float* d_delta);

/* ---- compare_sample_sets --paired: Wilcoxon signed-rank test over m matched column pairs, per row
 *      scipy.stats.wilcoxon(d, zero_method="wilcox", correction=False, alternative="two-sided", method="asymptotic")
 *      under the row rules above.
 *  Pair q is the columns (a[q], b[q]), 1 <= m <= 4096, a column at most once over both lists; otherwise SDICE_ERR_ARG
 *  before any launch, outputs untouched (the host call checks the index range and the one-appearance rule, the _dev
 *  call m and 2 m <= s).  Values are finite float32 or NaN.
 *  Per row: a pair is kept when both of its values are non-NaN; with fewer than 3 kept pairs the row is not tested and
 *  every output slot is 0.  mean1 / med1 are np.mean / np.median of the a-side values of the kept pairs in pair order,
 *  bit for bit as in sdice_ranksum, mean2 / med2 of the b side, delta = med1 - med2 in float32; equal pairs count here.
 *  Differences: when every kept value of the row is a 3-decimal PS value float32(key / 1000), key = 0..1000, d =
 *  key_a - key_b as an integer (thousandths), otherwise d = x - y in float32.  This departs from scipy on purpose: a
 *  floating subtraction of 3-decimal values breaks ties by rounding noise (float32(0.3) - float32(0.2) !=
 *  float32(0.2) - float32(0.1)), and equal printed differences must tie.
 *  Zero differences are dropped (n' are left), |d| gets average ranks, R+ is the rank sum of the positive ones:
 *  z = (R+ - n'(n'+1)/4) / sqrt((n'(n'+1)(2n'+1) - sum(t^3 - t)/2) / 24), positive when side 1 is larger (scipy
 *  reports -|z|), p = erfc(|z| / sqrt 2), as accurate as sdice_ranksum's.  A tested row with n' = 0 has z = 0, p = 1
 *  (scipy: NaN).  Always the normal approximation, from 3 pairs up: scipy's exact and permutation p-values
 *  (method="auto") are not offered by this call (sdice_signedrank_exact below has the exact one).  z optional (NULL to skip). */
int sdice_signedrank(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a,
                     const int32_t* b, int32_t m, uint8_t* tested, double* p, double* z, float* med1,
                     float* med2, float* mean1, float* mean2, float* delta);
int sdice_signedrank_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a,
                         const int32_t* d_b, int32_t m, uint8_t* d_tested, double* d_p, double* d_z,
                         float* d_med1, float* d_med2, float* d_mean1, float* d_mean2, float* d_delta);

/* ---- compare_sample_sets --exact: the two tests above with the exact conditional p-value on small rows (not in the
 *      reference).  Arguments, refusals and limits are those of sdice_ranksum / sdice_signedrank plus a trailing
 *      exact[n] (uint8, required); the row rules, tested, med1/2, mean1/2, delta and z are theirs bit for bit.  Only p
 *      changes, and only on eligible rows: exact[row] = 1 where p is the exact value, 0 where the row is not tested or
 *      keeps the asymptotic p (bit for bit that of the plain call).  Groups of up to 4096 columns stay legal; their rows
 *      are eligible only where NaNs leave few enough values.
 *  Rank-sum: a tested row is eligible when its kept counts satisfy n1' + n2' = N <= 32 (C(32, 16) fits 32 bits).
 *  Doubled mid-ranks r_i = 2 #(v_j < v_i) + #(v_j == v_i) + 1 by float32 value: -0.0 == +0.0 is one tie group,
 *  subnormals are distinct values, +-inf are ordinary values.  k = min(n1', n2'), W = the doubled rank sum of that set
 *  (set 1 on a tie of sizes), D = |W - k(N+1)|,
 *      p = #{k-subsets S of the N doubled ranks : |sum(S) - k(N+1)| >= D} / C(N, k),
 *  both integers, p one float64 division: the permutation distribution given the observed ties, the exact counterpart
 *  of erfc(|z| / sqrt 2), symmetric in which set is taken.  Untied rows: scipy.stats.mannwhitneyu(method="exact").  An
 *  all-equal row has D = 0, p = 1.
 *  Signed-rank: a tested row is eligible when it has 1 <= n' <= 31 non-zero differences (2^31 fits 32 bits); n' = 0
 *  keeps p = 1 with exact = 1.  The differences are sdice_signedrank's (integer thousandths on a row of 3-decimal
 *  values, float32 otherwise), doubled mid-ranks of |d|, W = the doubled rank sum of the positive ones,
 *  D = |2W - n'(n'+1)|,
 *      p = #{sign patterns : |2 sum(S) - n'(n'+1)| >= D} / 2^n'.
 *  Rows without ties or zeros: scipy.stats.wilcoxon(method="exact"). */
int sdice_ranksum_exact(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps,
                        const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2,
                        uint8_t* tested, double* p, double* z, float* med1, float* med2,
                        float* mean1, float* mean2, float* delta, uint8_t* exact);
int sdice_ranksum_exact_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps,
                            const int32_t* d_g1, int32_t n1, const int32_t* d_g2, int32_t n2,
                            uint8_t* d_tested, double* d_p, double* d_z, float* d_med1, float* d_med2,
                            float* d_mean1, float* d_mean2, float* d_delta, uint8_t* d_exact);
int sdice_signedrank_exact(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a,
                           const int32_t* b, int32_t m, uint8_t* tested, double* p, double* z, float* med1,
                           float* med2, float* mean1, float* mean2, float* delta, uint8_t* exact);
int sdice_signedrank_exact_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a,
                               const int32_t* d_b, int32_t m, uint8_t* d_tested, double* d_p, double* d_z,
                               float* d_med1, float* d_med2, float* d_mean1, float* d_mean2, float* d_delta,
                               uint8_t* d_exact);

/* ---- compare_sample_sets --strata: the rank-sum test stratified by batch (van Elteren's stratified Wilcoxon test; not
 *      in the reference), per row under the row rules above.  What coin::wilcox_test(y ~ g | batch) computes.
 *  g1[n1], g2[n2]: the column indices of the two groups as in sdice_ranksum; strat1[n1], strat2[n2]: the int32 stratum id
 *  of each listed column, in [0, n_strata), parallel to g1 and g2.  1 <= n_strata <= 64, 1 <= n1, n2 <= 4096, a column
 *  at most once over both lists; otherwise SDICE_ERR_ARG before any launch, outputs untouched, the reason in
 *  sdice_last_error (the host call checks the index range, the stratum ids and the one-appearance rule, the _dev call
 *  n1, n2, n_strata and n1 + n2 <= s).  Values are finite float32 or NaN.
 *  Per row and stratum h: the values at the group-1 and at the group-2 columns of h with NaNs dropped, n1h and n2h kept,
 *  N_h = n1h + n2h.  A stratum is informative when n1h >= 1 and n2h >= 1; any other stratum (one that holds samples of
 *  one group only, or none after the NaN drop) contributes nothing.  Inside an informative stratum, over its N_h values
 *  only: r2(v) = 2 #{x < v} + #{x == v} + 1 (twice the mid-rank, an integer; ties by float32 equality, -0.0 == +0.0),
 *      D_h = sum of r2 over group 1 of h - n1h (N_h + 1)            (= 2 (W_h - E[W_h]))
 *      T_h = sum of t^3 - t over the stratum's tie runs
 *      d_h = D_h / (2 (N_h + 1))
 *      V_h = n1h n2h (N_h^3 - N_h - T_h) / (12 N_h (N_h - 1) (N_h + 1)^2)
 *  and over the strata z = sum d_h / sqrt(sum V_h), p = erfc(|z| / sqrt 2): weights 1 / (N_h + 1), the tie-corrected
 *  variance, no continuity correction; z > 0 when group 1 is larger.  z and p do not depend on how the strata are
 *  numbered (bit for bit), and swapping the groups gives -z and the same p.
 *  With n1', n2' the kept counts summed over the informative strata the row is tested when n1' >= 3 and n2' >= 3;
 *  otherwise every output slot is 0.  A tested row with sum V_h = 0 (every informative stratum fully tied) has z = 0,
 *  p = 1.  With one stratum and no ties z is scipy.stats.ranksums'; with ties p is scipy.stats.mannwhitneyu(
 *  use_continuity=False, method="asymptotic")'s, NOT sdice_ranksum's, which has no tie correction.
 *  med1 / med2 / mean1 / mean2 are np.median / np.mean of ALL kept values of a group (every stratum, informative or not)
 *  in the order of g1 / g2, delta = med1 - med2 in float32: on every row this call tests, bit for bit what sdice_ranksum
 *  reports for the same lists.  p is as accurate as sdice_ranksum's.  z optional (NULL to skip). */
int sdice_ranksum_strata(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps,
                         const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2,
                         const int32_t* strat1, const int32_t* strat2, int32_t n_strata,
                         uint8_t* tested, double* p, double* z, float* med1, float* med2,
                         float* mean1, float* mean2, float* delta);
int sdice_ranksum_strata_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps,
                             const int32_t* d_g1, int32_t n1, const int32_t* d_g2, int32_t n2,
                             const int32_t* d_strat1, const int32_t* d_strat2, int32_t n_strata,
                             uint8_t* d_tested, double* d_p, double* d_z, float* d_med1, float* d_med2,
                             float* d_mean1, float* d_mean2, float* d_delta);

/* ---- compare_sample_sets --ks: the two-sample Kolmogorov-Smirnov test per row (not in the reference): any difference
 *      between the two empirical distributions, not a shift alone.
 *  Row rules are sdice_ranksum's: ps[n,s] float32, NaN = no value; NaNs are dropped per group, n1' and n2' kept; the row
 *  is tested when n1' >= 3 and n2' >= 3, otherwise every output slot is 0.  Any float32 value is legal: signed zeros
 *  (-0.0 == +0.0 is one value), subnormals (distinct values), values outside [0, 1], +-inf (ordinary values at the ends of
 *  the order).  1 <= n1, n2 <= 4096, a column at most once over both lists; otherwise SDICE_ERR_ARG before any launch,
 *  outputs untouched, the reason in sdice_last_error (the host call checks the index range and the one-appearance rule,
 *  the _dev call n1, n2 and n1 + n2 <= s).
 *  Per tested row, with c1(v) = #{x in group 1 : x <= v} and c2(v) likewise, by float32 comparison:
 *      M    = max over the distinct kept values v of |c1(v) n2' - c2(v) n1'|        (an integer, at most 2^24)
 *      D    = M / (n1' n2')                          one float64 division: bit for bit float(Fraction(M, n1' n2'))
 *      lam2 = M^2 / (n1' n2' (n1' + n2'))            both integers exact in float64, one division
 *      p    = min(1, 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lam2))         = scipy.special.kolmogorov(sqrt(lam2))
 *  The empirical distribution functions are compared at the END of a tie run only, never inside one.  p is Kolmogorov's
 *  limiting distribution: no Stephens or continuity correction, no finite-n form (scipy's kstwo / method="auto" differ).
 *  M = 0 (all kept values equal, or identical samples) gives D = 0, p = 1.  p is as accurate as sdice_ranksum's: within
 *  1e-9 relative down to 1e-280, 0 past the float64 range.
 *  want_exact != 0: a tested row with N = n1' + n2' <= 32 (C(32, 16) fits 32 bits) gets the exact conditional
 *  (permutation) p given the row's ties and exact[row] = 1.  With T the tie-run ends of the merged order as cumulative
 *  counts t, inside = the number of lattice paths (0,0) -> (n1', n2') with |i n2' - (t - i) n1'| < M at every t in T (i =
 *  group-1 values among the first t), p = (C(N, n1') - inside) / C(N, n1'), both integers, one float64 division.  What
 *  R >= 4.2 ks.test(exact = TRUE) computes with ties and scipy.stats.ks_2samp(method="exact") on untied rows.  Rows
 *  with N > 32 keep the asymptotic p and exact[row] = 0; so does every row when want_exact == 0.
 *  med1 / med2 / mean1 / mean2 / delta: bit for bit sdice_ranksum's on every tested row.  Swapping the groups gives the
 *  same D and p.  d optional (NULL to skip); exact is required when want_exact != 0 and may be NULL otherwise. */
int sdice_ks(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps,
             const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2, int32_t want_exact,
             uint8_t* tested, double* p, double* d, float* med1, float* med2,
             float* mean1, float* mean2, float* delta, uint8_t* exact);
int sdice_ks_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps,
                 const int32_t* d_g1, int32_t n1, const int32_t* d_g2, int32_t n2, int32_t want_exact,
                 uint8_t* d_tested, double* d_p, double* d_d, float* d_med1, float* d_med2,
                 float* d_mean1, float* d_mean2, float* d_delta, uint8_t* d_exact);

/* ---- compare_sample_sets --shift: the Hodges-Lehmann shift of group 1 against group 2 per row with its distribution-free
 *      confidence interval (Moses / Lehmann; Hollander & Wolfe sections 4.2-4.3; R's wilcox.test(conf.int = TRUE) reports
 *      the same interval; not in the reference): the size of the difference that the rank-sum statistic tests.
 *  Inputs are sdice_ranksum's plus zq, the standard normal quantile at 1 - (1 - conf) / 2 (1.959963984540054 for 95 %).
 *  1 <= n1, n2 <= 4096, a column at most once over both lists, zq finite and > 0; otherwise SDICE_ERR_ARG before any launch,
 *  outputs untouched, the reason in sdice_last_error (the host call checks the index range and the one-appearance rule,
 *  the _dev call n1, n2 and n1 + n2 <= s).
 *  Outputs, one slot per row, all required: tested[n] uint8, shift[n], lo[n], hi[n] float64, rank[n] int32; every slot of
 *  a row that is not tested is 0.
 *  Row rules are sdice_ranksum's: NaN = no value, NaNs are dropped per group, n1' and n2' kept, the row is tested when
 *  n1' >= 3 and n2' >= 3; tested equals sdice_ranksum's bit for bit.
 *  With x the kept values of group 1, y those of group 2, M = n1' n2', N = n1' + n2', the M differences d_ij = x_i - y_j in
 *  ascending order D_(1) <= ... <= D_(M):
 *    on-grid row (every kept value is a 3-decimal PS value float32(key / 1000), key = 0..1000): d is the INTEGER
 *      key_x - key_y in thousandths and an order statistic k is reported as (double)k / 1000.0 -- the rule of
 *      sdice_signedrank, for its reason: equal printed differences must tie;
 *    any other row: d = (double)x - (double)y, one IEEE float64 subtraction (-0.0 == +0.0).
 *    shift = the median of D: D_((M+1)/2) for odd M; for even M the mean of the two middle ones, (k_a + k_b) / 2000.0
 *      on-grid and 0.5 * (D_a + D_b) otherwise.
 *    rank  = c = max(1, floor(M/2 - zq sqrt(M (N + 1) / 12))), evaluated in float64 as written: the normal approximation
 *      of the rank-sum null distribution without a tie correction.
 *    lo = D_(c), hi = D_(M + 1 - c).
 *  c = 1 means that the interval is the whole range of the differences and that the requested level is NOT reached: the
 *  groups are too small for it (3 v 3 at 95 % is such a row).  A zero result is +0.0.  A row that keeps a +-inf value
 *  gets shift = lo = hi = NaN, with tested and rank as usual.  Any other float32 value is legal: signed zeros, subnormals,
 *  values outside [0, 1], +-FLT_MAX (a difference of 2 FLT_MAX is finite in float64).  Swapping the groups gives
 *  (-shift, -hi, -lo) and the same rank, bit for bit up to the +0.0 rule.
 *  Not offered: an exact (qwilcox) rank for small rows, a tie-corrected variance, a stratified form.  The paired estimate
 *  (the median of the Walsh averages) is sdice_walsh's, below. */
int sdice_shift(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps,
                const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2, double zq,
                uint8_t* tested, double* shift, double* lo, double* hi, int32_t* rank);
int sdice_shift_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps,
                    const int32_t* d_g1, int32_t n1, const int32_t* d_g2, int32_t n2, double zq,
                    uint8_t* d_tested, double* d_shift, double* d_lo, double* d_hi, int32_t* d_rank);

/* ---- compare_sample_sets --paired --pseudomedian: the paired shift per row with its distribution-free confidence interval
 *      (the one-sample Hodges-Lehmann estimate of the within-pair differences, Hollander & Wolfe sections 3.2-3.3; R's
 *      wilcox.test(paired = TRUE, conf.int = TRUE) prints the estimate as "(pseudo)median"; not in the reference): the size of
 *      the difference that the signed-rank statistic tests.
 *  Inputs are sdice_signedrank's plus zq, the standard normal quantile at 1 - (1 - conf) / 2 (1.959963984540054 for 95 %).
 *  Pair q is the columns (a[q], b[q]), 1 <= m <= 4096, a column at most once over both lists, zq finite and > 0; otherwise
 *  SDICE_ERR_ARG before any launch, outputs untouched, the reason in sdice_last_error (the host call checks the index range
 *  and the one-appearance rule, the _dev call m, 2 m <= s and zq).
 *  Outputs, one slot per row, all required: tested[n] uint8, shift[n], lo[n], hi[n] float64, rank[n] int32 (the outputs of
 *  sdice_shift); every slot of a row that is not tested is 0.
 *  Per row: a pair is kept when both of its values are non-NaN, m' pairs are kept, the row is tested when m' >= 3; tested
 *  equals sdice_signedrank's bit for bit.
 *  ZERO DIFFERENCES ARE KEPT: the estimator and its interval use all m' differences, unlike the test, which drops the zeros
 *  (Hollander & Wolfe 3.2-3.3), so m' here is sdice_signedrank's kept count, not its n'.
 *  The differences d are sdice_signedrank's: on-grid row (every kept value is a 3-decimal PS value float32(key / 1000), key =
 *  0..1000): d = key_a - key_b, an integer in [-1000, 1000]; any other row: d = x - y in float32 (-0.0 == +0.0).  The estimate
 *  and its interval thus belong to the test made on the same row.
 *  The M = m'(m'+1)/2 Walsh sums S_ij = d_i + d_j, i <= j: integers in [-2000, 2000] on the grid, where an order statistic is
 *  reported as (double)S / 2000.0; S = (double)d_i + (double)d_j, one IEEE float64 addition, on any other row, where an order
 *  statistic is reported as 0.5 * S.  With W_(1) <= ... <= W_(M) the Walsh averages so ordered:
 *    shift = the median of W: W_((M+1)/2) for odd M; for even M, with a and b the two middle ones, (double)(S_a + S_b) / 4000.0
 *      on the grid and 0.5 * (W_a + W_b) otherwise.
 *    rank  = c = max(1, floor(M/2 - zq sqrt(m'(m'+1)(2m'+1)/24))), evaluated in float64 as written: the normal approximation
 *      of the signed-rank null distribution without a tie correction.
 *    lo = W_(c), hi = W_(M + 1 - c).
 *  c = 1 means that the interval is the whole range of the averages and that the requested level is NOT reached: at 95 %
 *  that is every row with m' <= 6 (m' = 7 is the first with c = 2).  A zero result is +0.0.  A row that keeps a +-inf value,
 *  or whose float32 d overflows to +-inf (FLT_MAX - (-FLT_MAX)), gets shift = lo = hi = NaN, with tested and rank as usual.
 *  Any other float32 value is legal: signed zeros, subnormals, values outside [0, 1].  Swapping a and b gives (-shift, -hi,
 *  -lo) and the same rank, bit for bit up to the +0.0 rule.
 *  Not offered: an exact (qsignrank) rank for small rows (R takes it below 50 untied pairs), R's root-finding interval under
 *  ties, a tie-corrected variance, one-sided intervals. */
int sdice_walsh(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* a, const int32_t* b, int32_t m,
                double zq, uint8_t* tested, double* shift, double* lo, double* hi, int32_t* rank);
int sdice_walsh_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_a, const int32_t* d_b,
                    int32_t m, double zq, uint8_t* d_tested, double* d_shift, double* d_lo, double* d_hi, int32_t* d_rank);

/* ---- correlate: Spearman rank correlation of the PS values of m listed columns with one covariate value per listed
 *      column, per row scipy.stats.spearmanr(x_kept, ps_kept) under the row rules above (not in the reference).
 *  The covariate does not cross the ABI.  cols[m]: the columns sorted by covariate value, ties in table order; xg[m]: the
 *  dense tie-group id of each listed column: xg[0] = 0, never decreasing, steps of 0 or 1 (equal covariate values share
 *  an id; engine.spearman_order() makes both).  3 <= m <= 4096, every index in [0, s), a column listed once; otherwise,
 *  or with a malformed xg, SDICE_ERR_ARG before any launch, outputs untouched (the host call checks the two arrays, the
 *  _dev call m, m <= s and the sizes).  Values are finite float32 or NaN.
 *  Per row: a sample is kept when its PS value is not NaN; with fewer than 3 kept the row is not tested and every output
 *  slot is 0.  n_kept is the kept count; mean / med are np.mean / np.median of the kept values in the order of cols, bit
 *  for bit as in sdice_ranksum.  Both sides get average ranks among the kept samples of the row (PS ties by float32
 *  equality, -0.0 == +0.0; covariate ties by xg), rho is the Pearson correlation of the ranks, formed from exact integer
 *  sums of the doubled ranks, and p = 2 t.sf(|t|, n' - 2) = I_{1 - rho^2}((n' - 2) / 2, 1 / 2) in float64.
 *  A row whose kept PS values, or whose kept covariate values, are all equal is tested with rho = 0, p = 1 (scipy: NaN).
 *  |rho| = 1 gives p = 0 and rho = 0 gives p = 1 exactly, from 3 kept samples up: always scipy's t approximation, no
 *  exact or permutation p.  rho optional (NULL to skip). */
int sdice_spearman(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols,
                   const int32_t* xg, int32_t m, uint8_t* tested, double* p, double* rho, int32_t* n_kept,
                   float* med, float* mean);
int sdice_spearman_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols,
                       const int32_t* d_xg, int32_t m, uint8_t* d_tested, double* d_p, double* d_rho,
                       int32_t* d_n_kept, float* d_med, float* d_mean);

/* ---- sample_matrix: sample-by-sample sums over the rows two samples share (not in the reference).
 *  cols[m]: the selected columns in output order, 2 <= m <= 4096, every index in [0, s), each at most once.  The four
 *  outputs are m x m int64, row-major, entry [a * m + b].  With k_a(r) the integer key of ps[r, cols[a]] (the value is
 *  float32(k / 1000), k = 0 .. 1000; -0.0 is key 0) and v_a(r) = 1 when that value is not NaN (any payload), else 0, over
 *  the rows r of the table:
 *    shared[a,b] = sum v_a v_b            the junctions both samples have (symmetric)
 *    sum1[a,b]   = sum k_a v_a v_b        a's key sum over the shared rows (sum1[b,a] is b's)
 *    sum2[a,b]   = sum k_a^2 v_a v_b
 *    prod[a,b]   = sum k_a k_b v_a v_b    (symmetric)
 *  All sums are exact integers, whatever the launch shape (param gram.rows_per_wg).  Any other value in a selected column
 *  -- off the 3-decimal grid, outside [0, 1], +-inf -- is refused: SDICE_ERR_ARG, sdice_last_error() names the row and the
 *  table column of the first one, and the check runs before any accumulation, so the outputs are untouched.  Unselected
 *  columns are never read.  m out of range, a column out of range or listed twice, a NULL output: SDICE_ERR_ARG before any
 *  launch, outputs untouched (the host call checks the column list; the _dev call checks m, m <= s and the pointers, and
 *  refuses a column index outside [0, s) that its pre-pass meets).  n = 0 gives all-zero matrices.  Every call zeroes its
 *  outputs itself.  The _dev call synchronises the context stream ONCE, after the pre-pass, to read the result of the
 *  bad-value check back; the sums are then queued asynchronously.  Device scratch: 2 bytes per row and selected column
 *  (rounded up to 64 columns) + two m x m int64 planes. */
int sdice_sample_gram(sdice_ctx* ctx, int64_t n, int32_t s, const float* ps, const int32_t* cols, int32_t m,
                      int64_t* shared, int64_t* sum1, int64_t* sum2, int64_t* prod);
int sdice_sample_gram_dev(sdice_ctx* ctx, int64_t n, int32_t s, const float* d_ps, const int32_t* d_cols, int32_t m,
                          int64_t* d_shared, int64_t* d_sum1, int64_t* d_sum2, int64_t* d_prod);
/* The host finish of the four matrices above (no context, no GPU): per pair, N = shared[a,b], all integers formed exactly
 * (128-bit):  num = N prod[a,b] - sum1[a,b] sum1[b,a],  va = N sum2[a,b] - sum1[a,b]^2,  vb likewise from [b,a].
 *  corr[a,b] = double(num) / sqrt(double(va) double(vb)) clamped to [-1, 1], the Pearson correlation of the two samples'
 *  PS values over the shared rows; NaN when N < min_shared or va <= 0 or vb <= 0; the diagonal is exactly 1.0 when va > 0.
 *  rmsd[a,b] = sqrt(double(sum2[a,b] + sum2[b,a] - 2 prod[a,b]) / double(N)) / 1000, the root-mean-square PS difference
 *  over the shared rows; NaN when N < min_shared or N = 0; defined for constant samples, 0 on the diagonal.
 *  Both come out symmetric bit for bit.  min_shared < 1, m < 1 or a NULL pointer: SDICE_ERR_ARG. */
int sdice_sample_matrix_finish(int32_t m, const int64_t* shared, const int64_t* sum1, const int64_t* sum2,
                               const int64_t* prod, int64_t min_shared, double* corr, double* rmsd);

/* ---- pairwise: replaces the per-pair loop pairwise_fisher.py:164-179
 *      (scipy.stats.fisher_exact two-sided on [[incl_a, incl_b],[excl_a, excl_b]]).
 *  incl[n,s] int32, excl[n,s] int64 (from sdice_ps); p[n, s(s-1)/2] float64 row-major,
 *  pair order (0,1),(0,2)...(s-2,s-1) (pairwise_fisher.py:142-147).
 *  COUNT RANGE of sdice_fisher_* and sdice_chi2_*: counts are non-negative, and the kernels take them as doubles, so for
 *  ANY two samples i != j of a junction -- the table [[a, b], [c, d]] = [[incl_i, incl_j], [excl_i, excl_j]] -- the
 *  total a + b + c + d must be at most 2^53; for sdice_fisher_* also a*d <= 2^53 and b*c <= 2^53 (the ratio walk steps on
 *  these products, and only an exact product ends at 0 where the support ends: beyond 2^53 the sum, and with it p, can
 *  come out with any value or sign).  So an inclusion count of 2^31 - 1 goes with exclusion sums up to 2^22, an
 *  exclusion sum of 2^40 with inclusion counts up to 8192.  The host entry points -- sdice_fisher_pairs, _pair_list,
 *  _tables, sdice_chi2_pairs, _pair_list -- check every junction (the pair-list forms too check all its samples, listed
 *  or not) and return SDICE_ERR_ARG before any launch, outputs untouched; the _dev forms cannot look and leave the range
 *  to the caller.  sdice_fisher_tables applies it per table.
 *  ACCURACY within the range, relative to the exact two-sided sum (scipy's rule: pmf(k) <= pmf(a)), for p >= 1e-280:
 *  1e-9 for totals up to 5e4, 1e-7 up to the log-factorial table's end (context parameter "fisher.table_max", 2^20: pmf(a)
 *  is a difference of nine log-factorials), 1e-6 beyond it at every accepted magnitude (pmf(a) in the saddle-point form,
 *  whose error does not grow with the counts; observed: DESIGN.md section 7).  Smaller p come out below 2e-280.  A table
 *  with a ratio pmf(k) / pmf(a) within 1e-12 above 1 counts that term as a tie.  chi2: 1e-9 against the formula below in
 *  exact arithmetic, for p >= 1e-280.  Walk length grows with the counts (about half the smaller margin for a balanced
 *  table): counts of 1e8 take seconds per pair.
 */
int sdice_fisher_pairs(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl,
                       const int64_t* excl, double* p);
int sdice_fisher_pairs_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl,
                           const int64_t* d_excl, double* d_p);
/* measurement aid (no reference counterpart): with the context parameter "fisher.count_steps" = 1 the pair kernel
 * counts the lane-steps it issues and those that advanced a live walk inside its support; this returns the two
 * counts of the last sdice_fisher_pairs[_dev] call (bench.py: roofline.valu_f64.useful_lane_frac). */
int sdice_fisher_step_stats(sdice_ctx* ctx, uint64_t* useful, uint64_t* issued);
/* m independent 2x2 tables abcd[m,4] int64 -> p[m] (same kernel math; KAT entry point) */
int sdice_fisher_tables(sdice_ctx* ctx, int64_t m, const int64_t* abcd, double* p);

/* pairwise --chi2: replaces test_method = scipy.stats.chi2_contingency (pairwise_fisher.py:133-136,
 * :179): Yates-corrected 2x2 chi-square, p = chdtrc(1, chi2).  scipy raises ValueError on a zero
 * expected frequency (the reference run aborts); such tables get p = NaN and are counted in *n_bad
 * so that the caller can raise.  Same shapes and pair order as sdice_fisher_pairs. */
int sdice_chi2_pairs(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl,
                     const int64_t* excl, double* p, int64_t* n_bad);
int sdice_chi2_pairs_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl,
                         const int64_t* d_excl, double* d_p, int64_t* d_n_bad /* device */);

/* ---- pairwise over a chosen list of sample pairs: the loops above (pairwise_fisher.py:142-147, :164-179) for the m
 *      pairs the caller names instead of all s(s-1)/2 -- matched tumour/normal, treated x control, each sample against
 *      one reference (no reference counterpart: pairwise_fisher.py always builds every pair).
 *  pairs[m,2] int32: column indices (i, j) into the count table; any order, i > j allowed (the 2x2 table is then
 *  [[incl_i, incl_j],[excl_i, excl_j]] with its columns in that order, as the reference would compute it on a table
 *  with its sample columns swapped), the same pair more than once allowed; i == j or an index outside [0, s) is
 *  SDICE_ERR_ARG.  1 <= m <= 33 550 336 (the pair count of s = 8192; m = 0 is a no-op), s <= 8192.
 *  p[n,m] float64 row-major, column q = pair q of the list; n_bad counts the listed tables only.
 *  The list (i, j) = (0,1),(0,2)...(s-2,s-1) gives bit for bit what sdice_fisher_pairs / sdice_chi2_pairs give. */
int sdice_fisher_pair_list(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl,
                           int64_t m, const int32_t* pairs, double* p);
int sdice_chi2_pair_list(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl,
                         int64_t m, const int32_t* pairs, double* p, int64_t* n_bad);
/* Device forms: the list lives on the device as a packed table of m uint32 (i << 16 | j), written ONCE by
 * sdice_pair_list_pack_dev -- which validates the host list pairs[m,2] against s as above and copies the table into
 * d_tab, a buffer of m * 4 bytes the caller owns (sdice_dmalloc); synchronous -- and then read by any number of
 * asynchronous calls.  The _dev calls trust d_tab: hand them nothing but what sdice_pair_list_pack_dev wrote for the
 * same s. */
int sdice_pair_list_pack_dev(sdice_ctx* ctx, int32_t s, int64_t m, const int32_t* pairs /* host */, uint32_t* d_tab);
int sdice_fisher_pair_list_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                               int64_t m, const uint32_t* d_tab, double* d_p);
int sdice_chi2_pair_list_dev(sdice_ctx* ctx, int64_t n, int32_t s, const int32_t* d_incl, const int64_t* d_excl,
                             int64_t m, const uint32_t* d_tab, double* d_p, int64_t* d_n_bad /* device */);

/* ---- Benjamini-Hochberg: replaces statsmodels multipletests(p, method="fdr_bh")[1]
 *      (compareSampleSets.py:235; pairwise_fisher.py:185,190). */
int sdice_bh(sdice_ctx* ctx, int64_t m, const double* p, double* q);
int sdice_bh_dev(sdice_ctx* ctx, int64_t m, const double* d_p, double* d_q);
/* BH over the PRESENT entries of a padded vector: entry i is present when tested[i] != 0 (tested == NULL:
 * when p[i] >= 0); absent entries are left out of the ranking and of m and get q = 0.  The sharded
 * compare gathers the per-junction table of every rank (padded to equal length) and corrects it in
 * place on the device -- the reference compacts the tested rows first (compareSampleSets.py:223-235). */
int sdice_bh_masked_dev(sdice_ctx* ctx, int64_t n, const double* d_p, const uint8_t* d_tested, double* d_q);
/* BH down each of `cols` columns of a row-major [n, cols] table, in place
 * (pairwise_fisher.py:187-191) */
int sdice_bh_columns(sdice_ctx* ctx, int64_t n, int64_t cols, double* p_inout);
int sdice_bh_columns_dev(sdice_ctx* ctx, int64_t n, int64_t cols, double* d_p_inout);
/* the same for a table whose rows are `pitch` elements apart (a column range of a wider table), pitch >= cols */
int sdice_bh_columns_pitched_dev(sdice_ctx* ctx, int64_t n, int64_t cols, int64_t pitch, double* d_p_inout);

/* measurement aid (tools/bench_cli.py): out3 = seconds spent formatting, seconds spent writing, bytes written by
 * sdice_write_table on the calling thread since the last reset */
int sdice_textio_stats(double* out3, int reset);

/* ---- host-side table text I/O (no device, no context): multithreaded, byte-compatible with the
 *      reference's writers  f'{x:.3f}' (SPLICEDICE.py:353, counts_to_ps.py:69), f'{x:.0f}'
 *      (SPLICEDICE.py:340), str(numpy.float64) (pairwise_fisher.py:200)  and with its readers
 *      (text -> float64 -> dtype: compareSampleSets.py:202, pairwise_fisher.py:60, counts_to_ps.py:50).
 *  Tables are  header-line '\n'  then one line per row:  name '\t' v '\t' v ... '\n'.
 *  names: concatenated row names, name_off[n+1] byte offsets into it.
 *  dtype 0 float32, 1 float64, 2 int32;  mode 0 '%.3f', 1 '%.0f', 2 numpy str() shortest repr;
 *  mode | 0x100 appends to an existing file (tables streamed in row slabs). */
int sdice_write_table(const char* path, const char* header /* incl. '\n' */, int64_t n, int32_t s,
                      const char* names, const int64_t* name_off, const void* data, int dtype, int mode,
                      int threads /* 0 = all cores */);
/* Column-major variant: column c is cols[c] (n values) with its own dtype / mode -- the
 * compare_sample_sets output table mixes float32 and float64 numpy-repr columns
 * (compareSampleSets.py:252-270). */
int sdice_write_columns(const char* path, const char* header, int64_t n, const char* names, const int64_t* name_off,
                        int32_t ncols, const void* const* cols, const int32_t* dtypes, const int32_t* modes, int threads);
/* sdice_write_columns with a ready-made text suffix per row (written after the last numeric column): the
 * gene / overlapping / transcript_id columns of an annotated table (compareSampleSets.py:238-264). */
int sdice_write_columns_sfx(const char* path, const char* header, int64_t n, const char* names, const int64_t* name_off,
                            int32_t ncols, const void* const* cols, const int32_t* dtypes, const int32_t* modes,
                            const char* sfx, const int64_t* sfx_off, int threads);
/* The interval scan of the GTF annotation join (compareSampleSets.py:246-252): event e (group ev_group[e], -1 =
 * none; positions ev_a[e], ev_b[e]) matches interval k of its group (grp_ptr CSR over lo[] / hi[]) when
 * lo <= a <= hi or lo <= b <= hi.  out_idx == NULL: fill out_ptr[0..n_events] with the prefix sums of the match
 * counts; otherwise also write the matching interval indices (increasing k per event). */
int sdice_interval_overlaps(int64_t n_events, const int32_t* ev_group, const int64_t* ev_a, const int64_t* ev_b,
                            int32_t n_groups, const int64_t* grp_ptr, const int64_t* lo, const int64_t* hi,
                            int64_t* out_ptr, int64_t* out_idx, int64_t out_cap, int threads);
/* `<prefix>_allClusters.tsv` (SPLICEDICE.py:316-326): name<TAB>comma-joined names of the row's
 * neighbour list (CSR in row indices), one line per junction row. */
int sdice_write_clusters(const char* path, int64_t n, const char* names, const int64_t* name_off,
                         const int64_t* row_ptr, const int32_t* col, int threads);
/* `<prefix>_junctions.bed` (SPLICEDICE.py:316-321): chrom<TAB>left<TAB>right<TAB>chrom:left-right:strand<TAB>0<TAB>strand
 * per junction row; chrom[r] indexes the n_chrom names in chrom_names / chrom_off, strand[r] is the character. */
int sdice_write_junction_bed(const char* path, int64_t n, const char* chrom_names, const int64_t* chrom_off,
                             int32_t n_chrom, const int32_t* chrom, const int32_t* left, const int32_t* right,
                             const char* strand, int threads);
/* sdice_write_table keeps its threads' text buffers between calls (a table written in slabs); this frees them. */
int sdice_textio_trim(void);
/* Row names 'chrom:left-right:strand' (SPLICEDICE.py:312-314) of n junction rows as one byte string + off[n + 1], the
 * form the table writers above take their names in.  *need = bytes the names take; out_cap too small (or out NULL, to
 * ask for the size): SDICE_ERR_ARG with off and *need filled. */
int sdice_junction_names(int64_t n, const char* chrom_names, const int64_t* chrom_off, int32_t n_chrom,
                         const int32_t* chrom, const int32_t* left, const int32_t* right, const char* strand,
                         char* out, int64_t out_cap, int64_t* off, int64_t* need);
typedef struct sdice_table sdice_table;
int sdice_table_open(const char* path, sdice_table** out, int64_t* n, int32_t* s, int64_t* names_bytes,
                     int64_t* header_bytes);
int sdice_table_read(sdice_table* t, char* header, char* names, int64_t* name_off, void* data,
                     int dtype /* 0 float32, 1 float64 */, int threads);
int sdice_table_close(sdice_table* t);

/* ---- host-side junction-file parser (no device, no context): one pass over a sample file of
 *      `splicedice quant` with the reference's per-type admission filters
 *      (SPLICEDICE.getAllJunctions, SPLICEDICE.py:147-228) and every line's key + score for the
 *      count pass (SPLICEDICE.getJunctionCounts, SPLICEDICE.py:257-295).
 *  type: 0 bed / leafcutter, 1 splicedicebed, 2 STAR SJ.out.tab.
 *  Per line: chrom_id (index into the file's chromosome table, first-appearance order), left, right,
 *  strand (0 '+', 1 '-', 2 other), score, admit (1 = passes the admission filters).
 *  sdice_junc_lookup: row of every query junction in rows sorted by (chrom, left, right, strand), -1 if absent. */
typedef struct sdice_juncfile sdice_juncfile;
int sdice_junc_open(const char* path, int type, sdice_juncfile** out, int64_t* n_lines, int32_t* n_chroms,
                    int64_t* chrom_bytes);
int sdice_junc_read(sdice_juncfile* f, int32_t min_length, int32_t max_length, int32_t min_unique,
                    int32_t min_overhang, double min_entropy, int no_multimap, int32_t* chrom_id,
                    int32_t* left, int32_t* right, int8_t* strand, int64_t* score, uint8_t* admit,
                    char* chrom_names, int64_t* chrom_off /* [n_chroms+1] */, int threads);
int sdice_junc_close(sdice_juncfile* f);
int sdice_junc_lookup(int64_t n_rows, const int32_t* row_chrom, const int32_t* row_left,
                      const int32_t* row_right, const int8_t* row_strand, int64_t n_q,
                      const int32_t* q_chrom, const int32_t* q_left, const int32_t* q_right,
                      const int8_t* q_strand, int32_t* row_out, int threads);
/* One sample's column of the count table (SPLICEDICE.getJunctionCounts, SPLICEDICE.py:257-295: later lines of a file
 * overwrite earlier ones, no score filter): col[row] = score for every line whose junction is among the rows, in line
 * order.  col: the sample's int32 [n_rows] stretch of the TRANSPOSED table [sample][row], zeroed by the caller;
 * low (or NULL): set to 1 where a line with score < min_unique hits the row.  A final value outside [0, 2^31) is
 * SDICE_ERR_ARG ("junction counts must be non-negative and below 2**31", the reference's int conversion limit here).
 * Single-threaded: one call per sample, side by side.  sdice_transpose_i32: dst[c][r] = src[r][c] (threads).
 * sdice_host_threads: the default worker count of the host-side calls (hardware threads capped by the cgroup quota). */
int sdice_junc_count_column(int64_t n_rows, const int32_t* row_chrom, const int32_t* row_left,
                            const int32_t* row_right, const int8_t* row_strand, int64_t n_q,
                            const int32_t* q_chrom, const int32_t* q_left, const int32_t* q_right,
                            const int8_t* q_strand, const int64_t* score, int32_t min_unique, int32_t* col,
                            uint8_t* low);
/* Second step of the ingest, per file (the junction set of SPLICEDICE.getAllJunctions, SPLICEDICE.py:147-228):
 * chrom_rank[i] = rank_of_chrom[chrom_id[i]], and the admitted lines' keys, packed order-preservingly as
 * chrom 12 | left 31 | right - left 20 | strand 1 bits, compacted into keys_out (room for n; input of
 * sdice_sort_unique_u64).  *packable = 0 when an admitted junction does not fit the packing. */
int sdice_junc_pack_keys(int64_t n, const int32_t* chrom_id, const int32_t* rank_of_chrom, int32_t n_chroms,
                         const int32_t* left, const int32_t* right, const int8_t* strand, const uint8_t* admit,
                         int32_t* chrom_rank, uint64_t* keys_out, int64_t* n_keys, int32_t* packable);
int sdice_transpose_i32(int64_t rows, int64_t cols, const int32_t* src, int32_t* dst, int threads);
int sdice_host_threads(void);

/* ---- K0: sorted set of 64-bit keys, in place: the junction union of `quant`
 * (`self.junctions.add(...)` over every sample file + `sorted(self.junctions)`, SPLICEDICE.py:147-228,
 * :96) on order-preserving packed keys chrom|left|right-left|strand.  keys_inout holds n keys on
 * entry and the *n_unique distinct keys in ascending order on return. */
int sdice_sort_unique_u64(sdice_ctx* ctx, int64_t n, uint64_t* keys_inout, int64_t* n_unique);

/* ---- K8: `similarity` scoring (similarity.py:25-47).  For every row with sign != 0 (event
 * significant in the comparison table: p <= 0.05 and delta != 0, similarity.py:13-20) and every
 * column with a non-NaN PS: counts[c] += 1; scores[c] += (ps < mid) if sign < 0 else (ps > mid).
 * PS and midpoints are float64: the reference compares Python floats parsed from both tables.
 * The _dev call zeroes d_scores / d_counts before it adds (s == 0: nothing is written).  NULL ctx, a negative size, a
 * NULL output with s > 0 or a NULL input with n > 0: SDICE_ERR_ARG before anything is written. */
int sdice_similarity(sdice_ctx* ctx, int64_t n, int32_t s, const double* ps, const double* mid, const int8_t* sign,
                     int64_t* scores, int64_t* counts);
int sdice_similarity_dev(sdice_ctx* ctx, int64_t n, int32_t s, const double* d_ps, const double* d_mid,
                         const int8_t* d_sign, int64_t* d_scores, int64_t* d_counts);

/* ---- K9: per-row np.nanmean / np.nanstd over k selected columns (findOutliers.py:125-135), in the
 * matrix's own dtype (0 float32, 1 float64), bit-identical to numpy: NaNs replaced by zero in place,
 * numpy's pairwise summation, both divisions by the valid count in float64 then rounded.
 * mean / std are arrays of that dtype, n_nan the number of NaNs among the selected columns.  Bit-identical means NaN
 * where numpy has NaN and numpy's bit pattern everywhere else, the sign of a zero included (np.sum starts from +0).
 * idx may be in any order and repeat a column: the sums run in idx order, as numpy's r[idx] does.  1 <= k <= 1024,
 * dtype 0 or 1, no NULL pointer with n > 0 (the host call also checks 0 <= idx < s); otherwise SDICE_ERR_ARG before any
 * launch, outputs untouched. */
int sdice_rowstats(sdice_ctx* ctx, int64_t n, int32_t s, const void* data, int dtype, const int32_t* idx, int32_t k,
                   void* mean, void* std_, int32_t* n_nan);
int sdice_rowstats_dev(sdice_ctx* ctx, int64_t n, int32_t s, const void* d_data, int dtype, const int32_t* d_idx,
                       int32_t k, void* d_mean, void* d_std, int32_t* d_nan);

/* ---- junction-axis shard plan (host only, no context): `world` contiguous row ranges cut at clean
 *      positions (no overlap edge crosses the cut) nearest to k*n/world; where none lies within
 *      max_shift_frac * n / world of it the ideal position is kept and the shard gets a read-only halo.
 *      plan[world][4] = own_lo, own_hi (rows whose results the rank produces), ext_lo, ext_hi (rows it holds). */
int sdice_shard_plan(int64_t n, const int64_t* row_ptr, const int32_t* col, int32_t world, double max_shift_frac,
                     int64_t* plan);
/* the same plan from the junction coordinates alone -- rows in output order, i.e. sorted by (chrom rank, left, right,
 * strand) and distinct -- so that no rank has to cluster the whole set before it knows its range: i < j of one
 * (chrom, strand) are joined iff left[j] <= right[i] (SPLICEDICE.py:237-250).  A rank then clusters rows
 * [ext_lo, ext_hi) alone (sdice_cluster*): the lists of its own rows are complete, indices relative to ext_lo. */
int sdice_shard_plan_junctions(int64_t n, const int32_t* chrom_rank, const int32_t* left, const int32_t* right,
                               const int8_t* strand, int32_t world, double max_shift_frac, int64_t* plan);

/* ---- multi-GPU (new; the reference is single-process): one context per rank,
 *      RCCL communicator owned by the context.  id is SDICE_COMM_ID_BYTES opaque
 *      bytes created on rank 0 and distributed by the caller (any channel). */
#define SDICE_COMM_ID_BYTES 128
int sdice_comm_unique_id(sdice_ctx* ctx, void* id_out);
int sdice_comm_init(sdice_ctx* ctx, const void* id, int rank, int world);
int sdice_comm_destroy(sdice_ctx* ctx);
/* collectives beside compute: after sdice_comm_fork the context's collectives run on a second stream, behind everything
 * enqueued on the main stream so far (call it again before a collective whose input has just been produced);
 * sdice_comm_join makes the main stream wait for them and takes collectives back to the main stream (sdice_sync joins) */
int sdice_comm_fork(sdice_ctx* ctx);
int sdice_comm_join(sdice_ctx* ctx);
/* all-gather equal-sized row shards: recv holds world * bytes_per_rank */
int sdice_allgather_dev(sdice_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes_per_rank);
/* All-to-all of equal blocks: block q of d_send (bytes_per_peer each) goes to rank q, block r of
 * d_recv comes from rank r.  Used for the rows->columns transpose that `pairwise`'s default
 * per-pair-column BH (pairwise_fisher.py:187-191) needs when junction rows are sharded. */
int sdice_alltoall_dev(sdice_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes_per_peer);
/* Strided device copy (pack / unpack a column block of a row-major matrix), async on the ctx stream. */
int sdice_copy2d_dev(sdice_ctx* ctx, void* d_dst, int64_t dpitch, const void* d_src, int64_t spitch,
                     int64_t width_bytes, int64_t rows);

/* ---- per-kernel timing with HIP events on the context's stream ---------------------- */
/* on: 0 = off, 1 = every kernel, 2 = only the dominant kernel of each path (ps_tile_kernel,
 * ranksum_*_kernel, fisher_pairs_kernel, rccl_allgather) so that a timed loop is not perturbed */
int sdice_prof_enable(sdice_ctx* ctx, int on);
int sdice_prof_reset(sdice_ctx* ctx);
/* total device time and launch count of kernel `name` since the last reset (syncs) */
int sdice_prof_query(sdice_ctx* ctx, const char* name, int64_t* launches, double* total_ms);
/* newline-separated "name launches total_ms" table into buf */
int sdice_prof_report(sdice_ctx* ctx, char* buf, int cap);
/* stream-level stopwatch (hipEvents on the context stream) */
int sdice_timer_start(sdice_ctx* ctx);
int sdice_timer_stop(sdice_ctx* ctx, double* elapsed_ms);

/* Tuning and test knobs (integer parameters by name); unknown name -> ERR_ARG.  The one table of their names, defaults
 * and meanings is splicedice_amd/csrc/params.h (INTEGRATION.md lists it; sdice_param_info enumerates it); the defaults are
 * the measured optima. */
int sdice_set_param(sdice_ctx* ctx, const char* name, int64_t value);
/* the value in force: what sdice_set_param stored last, the default if the parameter was never set */
int sdice_get_param(sdice_ctx* ctx, const char* name, int64_t* value);
/* row `index` (0, 1, ...) of the parameter table: its name and default (either may be NULL); needs no context and no
 * device; past the end -> ERR_ARG */
int sdice_param_info(int32_t index, const char** name, int64_t* dflt);

/* Test support.  Region `index` (0, 1, ...) of the device memory this context keeps between calls and treats as
 * scratch: every arena chunk over its whole capacity ("arena"), the neighbour-list buffer over col_cap entries
 * ("cluster.col"), the block-reach buffer over reach_cap words ("cluster.reach").  Synchronises the context stream.
 * Not listed, because their contents carry meaning: the clustering status block, the Fisher log-factorial table.
 * Any out pointer may be NULL.  SDICE_ERR_ARG past the last region.  Changes nothing. */
int sdice_scratch_region(sdice_ctx* ctx, int32_t index, const char** name, void** dptr, int64_t* bytes);

/* Test support.  The launch plan of this context's last sdice_ps_dev launch (sdice_ps goes through it), as int32
 * fields in this fixed order:
 *    0 kern           0 = register-staged kernel (ps_tile_v3_kernel), 2 = first-generation kernel (ps_tile_kernel),
 *                     3 = register-staged kernel with a 16-bit count window (ps_tile_w16_kernel; the context profile
 *                     books its launches under "ps_tile_v3_kernel")
 *    1 vec            columns per item: 4 or 1
 *    2 chunk_cols     columns per column chunk (= s: unchunked)
 *    3 tile_rows      4 halo          5 n_tiles       6 n_chunks
 *    7 lv_shift       6 - log2(16-byte vectors per chunk row) where that is a power of two up to 64, else 0
 *    8 tiles_per_xcd  0 = no XCD remap
 *    9 use_reach     10 nt           11 prio         12 q3          13 threads
 * *n_fields (may be NULL) = 14; the first min(cap, 14) fields go to out (may be NULL when cap = 0).  A call that was
 * refused or had nothing to do (n = 0, s = 0) leaves the plan of the launch before it.  SDICE_ERR_STATE before the
 * first launch.  Changes nothing and launches nothing. */
#define SDICE_PS_PLAN_FIELDS 14
int sdice_ps_last_plan(sdice_ctx* ctx, int32_t* out, int32_t cap, int32_t* n_fields);

#ifdef __cplusplus
}
#endif
#endif /* SDICE_H */
