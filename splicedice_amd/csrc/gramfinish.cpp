// Host finish of the sample Gram sums (gram.hip, K15): Pearson correlation and root-mean-square PS difference of every
// sample pair from the four integer matrices.  No context and no GPU call.  Every integer is formed exactly in 128 bits
// (N * prod passes 2^63 on large cohorts); the only roundings are the int -> double conversions, one product, the square
// root and the division.
#include <math.h>
#include <stdint.h>
#include "sdice.h"

void sdice_set_error(const char* fmt, ...);

extern "C" int sdice_sample_matrix_finish(int32_t m, const int64_t* shared, const int64_t* sum1, const int64_t* sum2,
                                          const int64_t* prod, int64_t min_shared, double* corr, double* rmsd) {
    if (m < 1 || !shared || !sum1 || !sum2 || !prod || !corr || !rmsd) {
        sdice_set_error("sdice_sample_matrix_finish: bad arguments");
        return SDICE_ERR_ARG;
    }
    if (min_shared < 1) {
        sdice_set_error("sdice_sample_matrix_finish: min_shared must be at least 1 (got %lld)", (long long)min_shared);
        return SDICE_ERR_ARG;
    }
    typedef __int128 i128;
    const double nan = (double)NAN;
    for (int32_t a = 0; a < m; ++a) {
        for (int32_t b = 0; b < m; ++b) {
            const int64_t ab = (int64_t)a * m + b, ba = (int64_t)b * m + a;
            const i128 N = shared[ab];
            double c = nan, d = nan;
            if (N >= min_shared && N > 0) {
                const i128 sa = sum1[ab], sb = sum1[ba];
                const i128 va = N * sum2[ab] - sa * sa, vb = N * sum2[ba] - sb * sb;
                if (va > 0 && vb > 0) {
                    if (a == b) {
                        c = 1.0;
                    } else {
                        const i128 num = N * prod[ab] - sa * sb;
                        c = (double)num / sqrt((double)va * (double)vb);
                        c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
                    }
                }
                const i128 sq = (i128)sum2[ab] + sum2[ba] - 2 * (i128)prod[ab];
                d = sqrt((double)sq / (double)N) / 1000.0;
            }
            corr[ab] = c;
            rmsd[ab] = d;
        }
    }
    return SDICE_OK;
}
