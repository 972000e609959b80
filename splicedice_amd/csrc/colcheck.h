// Argument checks of the column lists of the row tests (colcheck.cpp, host only: `make asan` builds it).  Every list is a
// HOST array; a refusal is SDICE_ERR_ARG with the message the entry point has always given, for the first violation.
#pragma once
#include <stdint.h>
#include <initializer_list>

// k sample sets (kruskal.hip, jonckheere.hip): sets a call takes, and selected columns per row
constexpr int KW_MAX_SETS = 64;
constexpr int KW_MAX_N = 16384;          // both kernels (block kernel: 8 B of LDS per column)

// every one of the m entries of each list is a column of the table (0 .. s) and no column is listed twice, in one list or
// two; `fn` is the entry point the error names
int check_columns(const char* fn, std::initializer_list<const int32_t*> lists, int m, int s, const char* range_msg,
                  const char* once_msg);

// the checks the k-set entry points share: 2..KW_MAX_SETS sets, set_ptr from 0 and increasing, at most KW_MAX_N columns
// (that refusal names `fn`) and no more than the table has
int kw_check_sets(const char* fn, const int32_t* set_ptr, int32_t k, int32_t s);

// k matched sets of m columns each, set-major (friedman.hip): 2 <= k <= KW_MAX_SETS, 1 <= m <= FR_MAX_BLOCKS, k m <= KW_MAX_N
// and k m <= s, in this order; cols != NULL (the host entry points: a HOST list of k m entries): then also every entry a
// column of the table and no column listed twice.  cols == NULL: the list is on the device, the counts alone are checked.
constexpr int FR_MAX_BLOCKS = 4096;
int fr_check_sets(const char* fn, const int32_t* cols, int32_t k, int32_t m, int32_t s);

// Two column groups of their own lengths (strata.hip, ks.hip, shift.hip), at most `limit` columns each; max_strata != 0: every
// column carries a stratum id in [0, n_strata), 1 <= n_strata <= max_strata.  In this order:
//   the lists, when they are given and every count is in range: an index outside the table, a column listed twice over
//   both lists, a stratum id out of range (entry by entry, g1 first);
//   a group above the limit, a group without a column, the number of strata, more columns than the table has.
// g1 == NULL: the lists are on the device, the counts alone are checked (the _dev entry points).
int check_two_groups(const char* fn, const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2, int32_t s, int limit,
                     const int32_t* strat1 = nullptr, const int32_t* strat2 = nullptr, int32_t n_strata = 0,
                     int max_strata = 0);
