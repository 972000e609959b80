// Host-only: the argument checks of the column lists (colcheck.h) -- what a caller's column, set and stratum lists must
// satisfy before a row test launches anything.  No HIP in here: `make asan` builds this file as it stands.
#include <stddef.h>
#include <vector>
#include "sdice.h"
#include "colcheck.h"

void sdice_set_error(const char* fmt, ...);

static int refuse(const char* fn, const char* msg) {
    sdice_set_error("%s: %s", fn, msg);
    return SDICE_ERR_ARG;
}

int check_columns(const char* fn, std::initializer_list<const int32_t*> lists, int m, int s, const char* range_msg,
                  const char* once_msg) {
    std::vector<char> seen((size_t)s, 0);
    for (const int32_t* l : lists)
        for (int q = 0; q < m; ++q) {
            const char* msg = (l[q] < 0 || l[q] >= s) ? range_msg : (seen[l[q]] ? once_msg : nullptr);
            if (msg) return refuse(fn, msg);
            seen[l[q]] = 1;
        }
    return SDICE_OK;
}

int kw_check_sets(const char* fn, const int32_t* set_ptr, int32_t k, int32_t s) {
    const char* msg = nullptr;
    if (!set_ptr) msg = "set_ptr is NULL";
    else if (!(k >= 2 && k <= KW_MAX_SETS)) msg = "the number of sets must be 2..64";
    else if (set_ptr[0] != 0) msg = "set_ptr[0] must be 0";
    for (int i = 0; !msg && i < k; ++i)
        if (!(set_ptr[i + 1] > set_ptr[i])) msg = "empty set (set_ptr must increase)";
    if (msg) return refuse("kw_check_sets", msg);
    if (set_ptr[k] > KW_MAX_N) {
        sdice_set_error("%s: %d selected columns, at most %d are supported", fn, (int)set_ptr[k], KW_MAX_N);
        return SDICE_ERR_ARG;
    }
    if (set_ptr[k] > s)
        return refuse("kw_check_sets", "more selected columns than the table has (a column belongs to one set only)");
    return SDICE_OK;
}

int fr_check_sets(const char* fn, const int32_t* cols, int32_t k, int32_t m, int32_t s) {
    if (!(k >= 2 && k <= KW_MAX_SETS)) return refuse(fn, "the number of sets must be 2..64");
    if (!(m >= 1 && m <= FR_MAX_BLOCKS)) {
        sdice_set_error("%s: %d columns per set, each set needs 1..%d (one per subject)", fn, (int)m, FR_MAX_BLOCKS);
        return SDICE_ERR_ARG;
    }
    if ((int64_t)k * m > KW_MAX_N) {
        sdice_set_error("%s: %d selected columns, at most %d are supported", fn, (int)(k * m), KW_MAX_N);
        return SDICE_ERR_ARG;
    }
    if ((int64_t)k * m > s) return refuse(fn, "more selected columns than the table has (a column may appear once)");
    if (!cols) return SDICE_OK;
    return check_columns(fn, {cols}, k * m, s, "column index out of range", "a column may appear once over all sets");
}

int check_two_groups(const char* fn, const int32_t* g1, int32_t n1, const int32_t* g2, int32_t n2, int32_t s, int limit,
                     const int32_t* strat1, const int32_t* strat2, int32_t n_strata, int max_strata) {
    const bool counts_ok = n1 >= 1 && n1 <= limit && n2 >= 1 && n2 <= limit;
    const bool strata_ok = !max_strata || (n_strata >= 1 && n_strata <= max_strata);
    if (g1 && counts_ok && strata_ok) {
        std::vector<char> seen((size_t)s, 0);
        const int32_t* lists[2] = {g1, g2};
        const int32_t* strats[2] = {strat1, strat2};
        const int32_t counts[2] = {n1, n2};
        for (int l = 0; l < 2; ++l)
            for (int q = 0; q < counts[l]; ++q) {
                const int32_t c = lists[l][q];
                if (c < 0 || c >= s) return refuse(fn, "column index out of range");
                if (seen[c]) return refuse(fn, "a column may appear once over both lists");
                seen[c] = 1;
                if (max_strata && (strats[l][q] < 0 || strats[l][q] >= n_strata))
                    return refuse(fn, "stratum id outside [0, n_strata)");
            }
    }
    if (n1 > limit || n2 > limit) {
        sdice_set_error("%s: groups of %d and %d columns, at most %d each are supported", fn, (int)n1, (int)n2, limit);
        return SDICE_ERR_ARG;
    }
    if (n1 < 1 || n2 < 1) {
        sdice_set_error("%s: groups of %d and %d columns, each needs 1..%d", fn, (int)n1, (int)n2, limit);
        return SDICE_ERR_ARG;
    }
    if (!strata_ok) {
        sdice_set_error("%s: %d strata, the number of strata must be 1..%d", fn, (int)n_strata, max_strata);
        return SDICE_ERR_ARG;
    }
    if ((int64_t)n1 + n2 > s)
        return refuse(fn, "more selected columns than the table has (a column may appear once over both lists)");
    return SDICE_OK;
}
