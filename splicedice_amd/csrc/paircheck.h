// Argument checks of the pair tests (paircheck.cpp, host only: `make asan` builds it); SDICE_ERR_ARG prefixed with `who`.
#pragma once
#include <stdint.h>
#include <vector>

// Pair lists of the pairwise kernels: a column index takes 16 bits of a packed table entry (s <= 8192) and the pair kernel
// counts pairs in an int below 2^25 -- a list may be as long as every pair of 8192 samples.  sd_check_pair_list: every
// (i, j) of pairs[m][2] lies in [0, s) and i != j.  sd_pack_pair_list: tab[q] = i << 16 | j of a checked list.
constexpr int64_t SD_MAX_PAIRS = (int64_t)8192 * 8191 / 2;
int sd_check_pair_list(const char* who, int32_t s, int64_t m, const int32_t* pairs);
void sd_pack_pair_list(int64_t m, const int32_t* pairs, std::vector<uint32_t>& tab);
// Count range of the pair tests (host entry points; include/sdice.h): the kernels take the counts as doubles, so for ANY
// two samples i != j of a junction -- the table [[a, b], [c, d]] = [[incl_i, incl_j], [excl_i, excl_j]] -- the total
// a + b + c + d must not exceed 2^53 (every count, margin and total an exact double) and, walk (Fisher): neither must
// a d or b c (the walk's step products, fisher.hip Walk).  Non-negative counts.  sd_check_tables: the same per table
// abcd[m][4], walk included (sdice_fisher_tables).
constexpr int64_t SD_MAX_COUNT = (int64_t)1 << 53;
int sd_check_pair_counts(const char* who, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, bool walk);
int sd_check_tables(const char* who, int64_t m, const int64_t* abcd);
