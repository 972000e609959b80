// Host-only: how many columns of a table the column BH corrects at once (bh.h).  No HIP in here: `make asan` builds this
// file as it stands.
#include <algorithm>
#include "bh.h"

int64_t sd_bh_column_group(int64_t budget, int64_t per_column, int64_t fixed, int64_t cols, int64_t max_group) {
    int64_t g = budget > fixed ? (budget - fixed) / per_column : 0;
    g = std::max<int64_t>(1, std::min(g, std::min(cols, max_group)));
    if (g < cols && g > 16) g &= ~(int64_t)15;
    return g;
}
