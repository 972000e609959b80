// What bh.hip (the entry points, the radix paths) and bh_cols.hip (the sample-sort paths) share, and the host-only
// arithmetic of the column-group loop (bhplan.cpp: `make asan` builds it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sdice.h"

// per pair column (bh_cols.hip): `segs` columns of m values of a row-major table, in place; scratch from the context arena
size_t sd_bh_cols_scratch(int64_t m, int64_t segs);
bool sd_bh_cols_supported(int64_t m, int64_t segs);
int sd_bh_cols_samplesort(sdice_ctx* ctx, int64_t m, int64_t segs, double* d_rm, int64_t pitch);
// one vector (bh_cols.hip)
bool sd_bh_vector_supported(int64_t n);
size_t sd_bh_vector_scratch(sdice_ctx* ctx, int64_t n);
int sd_bh_vector_samplesort(sdice_ctx* ctx, int64_t n, const double* d_p, const uint8_t* d_tested, bool masked, double* d_q);

// Columns of a table of `cols` that one pass corrects when a group of g columns needs per_column * g + fixed bytes of
// scratch: what `budget` holds, at least 1, at most cols and max_group; a group that is not the whole table and holds more
// than 16 columns is rounded down to a multiple of 16 (whole 128-byte lines of the row-major table).
int64_t sd_bh_column_group(int64_t budget, int64_t per_column, int64_t fixed, int64_t cols, int64_t max_group);
