// Host-only: the argument checks of the pair tests (paircheck.h) -- what a caller's pair list and count tables must
// satisfy before fisher.hip and chi2.hip launch anything.  No HIP in here: `make asan` builds this file as it stands.
#include <algorithm>
#include "sdice.h"
#include "paircheck.h"

void sdice_set_error(const char* fmt, ...);

int sd_check_pair_list(const char* who, int32_t s, int64_t m, const int32_t* pairs) {
    for (int64_t q = 0; q < m; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || j < 0 || i >= s || j >= s) {
            sdice_set_error("%s: pair %lld is (%d, %d): column indices must lie in [0, %d)", who, (long long)q, i, j, s);
            return SDICE_ERR_ARG;
        }
        if (i == j) {
            sdice_set_error("%s: pair %lld pairs column %d with itself", who, (long long)q, i);
            return SDICE_ERR_ARG;
        }
    }
    return SDICE_OK;
}

void sd_pack_pair_list(int64_t m, const int32_t* pairs, std::vector<uint32_t>& tab) {
    tab.resize((size_t)m);
    for (int64_t q = 0; q < m; ++q) tab[q] = ((uint32_t)pairs[2 * q] << 16) | (uint32_t)pairs[2 * q + 1];
}

int sd_check_pair_counts(const char* who, int64_t n, int32_t s, const int32_t* incl, const int64_t* excl, bool walk) {
    typedef unsigned __int128 u128;
    for (int64_t row = 0; row < n; ++row) {
        // the two largest sample totals, inclusion counts and exclusion sums of the junction (and whose they are)
        int64_t t1 = 0, t2 = 0, i1 = 0, i2 = 0, e1 = 0, e2 = 0;
        int32_t i1k = -1, e1k = -1;
        for (int32_t k = 0; k < s; ++k) {
            const int64_t a = incl[row * s + k], c = excl[row * s + k];
            if (a < 0 || c < 0) {
                sdice_set_error("%s: counts must be non-negative", who);
                return SDICE_ERR_ARG;
            }
            if (c > SD_MAX_COUNT) {
                sdice_set_error("%s: junction %lld, sample %d: an exclusion sum of %lld is above 2^53", who, (long long)row, k,
                                (long long)c);
                return SDICE_ERR_ARG;
            }
            const int64_t t = a + c;
            if (t > t1) { t2 = t1; t1 = t; } else if (t > t2) t2 = t;
            if (a > i1) { i2 = i1; i1 = a; i1k = k; } else if (a > i2) i2 = a;
            if (c > e1) { e2 = e1; e1 = c; e1k = k; } else if (c > e2) e2 = c;
        }
        if (t1 + t2 > SD_MAX_COUNT) {
            sdice_set_error("%s: junction %lld: two samples' counts add up to %lld, above 2^53", who, (long long)row,
                            (long long)(t1 + t2));
            return SDICE_ERR_ARG;
        }
        if (walk) {
            // the largest incl_i * excl_j over i != j
            const u128 prod = i1k != e1k ? (u128)i1 * (u128)e1 : std::max((u128)i1 * (u128)e2, (u128)i2 * (u128)e1);
            if (prod > (u128)SD_MAX_COUNT) {
                sdice_set_error("%s: junction %lld: an inclusion count times another sample's exclusion sum is above 2^53 "
                                "(largest inclusion count %lld, largest exclusion sum %lld)", who, (long long)row, (long long)i1,
                                (long long)e1);
                return SDICE_ERR_ARG;
            }
        }
    }
    return SDICE_OK;
}

int sd_check_tables(const char* who, int64_t m, const int64_t* abcd) {
    typedef unsigned __int128 u128;
    for (int64_t i = 0; i < 4 * m; ++i)
        if (abcd[i] < 0) { sdice_set_error("%s: table entries must be non-negative", who); return SDICE_ERR_ARG; }
    for (int64_t i = 0; i < m; ++i) {                                 // the count range of sd_check_pair_counts, per table
        const int64_t* t = abcd + 4 * i;
        const bool fits = t[0] <= SD_MAX_COUNT && t[1] <= SD_MAX_COUNT && t[2] <= SD_MAX_COUNT && t[3] <= SD_MAX_COUNT &&
                          (u128)t[0] + (u128)t[1] + (u128)t[2] + (u128)t[3] <= (u128)SD_MAX_COUNT;
        if (!fits || (u128)t[0] * (u128)t[3] > (u128)SD_MAX_COUNT || (u128)t[1] * (u128)t[2] > (u128)SD_MAX_COUNT) {
            sdice_set_error("%s: table %lld (%lld, %lld, %lld, %lld): the total, a*d and b*c must not exceed 2^53", who,
                            (long long)i, (long long)t[0], (long long)t[1], (long long)t[2], (long long)t[3]);
            return SDICE_ERR_ARG;
        }
    }
    return SDICE_OK;
}
