// What fisher.hip and chi2.hip share: the pair index and the packed pair table entry on the device, and the host side of
// their eight entry points sdice_{fisher,chi2}_{pairs,pair_list}{,_dev} -- one argument check, one host staging routine.
#pragma once
#include "common.h"
#include <math.h>
#include <exception>

// pair index q -> (i, j), i < j, row-major (pairwise_fisher.py:142-147): q = i*s - i(i+1)/2 + (j-i-1)
__device__ __forceinline__ void sd_pair_of(int64_t q, int s, int& i, int& j) {
    const double bb = 2.0 * s - 1.0;
    i = (int)((bb - sqrt(bb * bb - 8.0 * (double)q)) * 0.5);
    if (i < 0) i = 0;
    if (i > s - 2) i = s - 2;
    while (i > 0 && (int64_t)i * s - (int64_t)i * (i + 1) / 2 > q) --i;
    while ((int64_t)(i + 1) * s - (int64_t)(i + 1) * (i + 2) / 2 <= q) ++i;
    j = (int)(q - ((int64_t)i * s - (int64_t)i * (i + 1) / 2)) + i + 1;
}

// a pair table entry i << 16 | j (pair_table_kernel, sd_pack_pair_list)
__device__ __forceinline__ void sd_pair_unpack(unsigned ij, int& i, int& j) {
    i = (int)(ij >> 16);
    j = (int)(ij & 0xffffu);
}

// The arguments of one entry point, host or device pointers alike.  list: the m pairs of tab (a host form's pairs[m][2], a
// _dev form's packed table) instead of every pair (m = 0, tab = NULL).  chi2: the call has n_bad and its counts need not fit the walk.
struct PairCall {
    const char* who;
    sdice_ctx* ctx;
    int64_t n;
    int32_t s;
    const int32_t* incl;
    const int64_t* excl;
    bool list; int64_t m; const void* tab;
    double* p;
    bool chi2; int64_t* n_bad;
    int64_t cols() const { return list ? m : (int64_t)s * (s - 1) / 2; }
};

static int sd_pair_limits(const char* who, int32_t s, int64_t m) {
    SD_ARG_AS(who, s <= 8192, "more than 8192 samples per junction is not supported");
    SD_ARG_AS(who, m <= SD_MAX_PAIRS, "more than 33550336 pairs in one list is not supported");
    return SDICE_OK;
}

// The one argument check, in the order of the list forms: sizes, n_bad (zeroed at once, so before every early return),
// limits, a host form's list, nothing to do (*todo is left false: every pair of s < 2 samples, an empty list, n = 0), pointers.
// An all-pairs host form leaves the limits to its _dev form, whose name that message has always carried.
static int sd_pair_args(const PairCall& c, bool dev, bool* todo) {
    SD_ARG_AS(c.who, c.ctx, "ctx is NULL");
    SD_ARG_AS(c.who, c.n >= 0 && c.s >= 0 && c.m >= 0, "negative size");
    if (c.chi2) {
        SD_ARG_AS(c.who, c.n_bad, dev ? "d_n_bad is NULL" : "n_bad is NULL");
        if (dev) {
            SD_HIP(hipSetDevice(c.ctx->device));
            SD_HIP(hipMemsetAsync(c.n_bad, 0, 8, c.ctx->stream));
        } else {
            *c.n_bad = 0;
        }
    }
    if (dev || c.list) SD_TRY(sd_pair_limits(c.who, c.s, c.m));
    if (c.list && !dev) {
        SD_ARG_AS(c.who, c.m == 0 || c.tab, "NULL pointer");
        SD_TRY(sd_check_pair_list(c.who, c.s, c.m, static_cast<const int32_t*>(c.tab)));
    }
    if (c.n == 0 || (c.list ? c.m == 0 : c.s < 2)) return SDICE_OK;
    if (c.list) SD_ARG_AS(c.who, c.s >= 2, "a pair list needs at least two samples");     // (a host form's list check was first)
    SD_ARG_AS(c.who, c.incl && c.excl && c.p && (c.tab || !c.list), "NULL pointer");
    *todo = true;
    return SDICE_OK;
}

// what an entry point's body throws (std::vector, std::string) becomes a status and a message
template <class Body> static int sd_no_throw(const char* who, Body body) {
    try {
        return body();
    } catch (const std::exception& e) {
        sdice_set_error("%s: %s", who, e.what());
        return SDICE_ERR_NOMEM;
    } catch (...) {
        sdice_set_error("%s: unknown exception", who);
        return SDICE_ERR_STATE;
    }
}

// a checked list, packed and copied to d_tab[m]
static int sd_pair_tab_upload(sdice_ctx* ctx, int64_t m, const int32_t* pairs, uint32_t* d_tab) {
    std::vector<uint32_t> tab;
    sd_pack_pair_list(m, pairs, tab);
    return sdice_h2d(ctx, d_tab, tab.data(), m * 4);
}

// A _dev form: the check, then launch(c) -- fisher_launch or chi2_launch over c.cols() columns.
template <class Launch> static int sd_pairs_dev(const PairCall& c, Launch launch) {
    bool todo = false;
    SD_TRY(sd_pair_args(c, true, &todo));
    return todo ? launch(c) : SDICE_OK;
}

// A host form: the checks (its list, the count range), device copies of the arguments, the _dev form of the same call
// under that form's own name, and the results back.
template <class Launch> static int sd_pairs_host(const PairCall& c, Launch launch) {
    return sd_no_throw(c.who, [&]() -> int {
        bool todo = false;
        SD_TRY(sd_pair_args(c, false, &todo));
        if (!todo) return SDICE_OK;
        SD_TRY(sd_check_pair_counts(c.who, c.n, c.s, c.incl, c.excl, !c.chi2));
        const std::string who_dev = std::string(c.who) + "_dev";
        HostStaging st(c.ctx);
        int32_t* di;
        int64_t *de, *db = nullptr;
        uint32_t* dt = nullptr;
        double* dp;
        SD_TRY(st.upload(&di, c.incl, c.n * c.s));
        SD_TRY(st.upload(&de, c.excl, c.n * c.s));
        if (c.list) {
            SD_TRY(st.alloc(&dt, c.m));
            SD_TRY(sd_pair_tab_upload(c.ctx, c.m, static_cast<const int32_t*>(c.tab), dt));
        }
        SD_TRY(st.alloc(&dp, c.n * c.cols()));
        if (c.chi2) SD_TRY(st.alloc(&db, 1));
        SD_TRY(sd_pairs_dev(PairCall{who_dev.c_str(), c.ctx, c.n, c.s, di, de, c.list, c.m, dt, dp, c.chi2, db}, launch));
        SD_TRY(st.download(c.p, dp, c.n * c.cols()));
        return c.chi2 ? st.download(c.n_bad, db, 1) : SDICE_OK;
    });
}
