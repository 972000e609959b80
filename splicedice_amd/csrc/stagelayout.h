// Layout of a host entry point's result fields in one device block (HostStaging, common.h).  No HIP: the sanitizer
// driver calls it.
#pragma once
#include <stdint.h>

constexpr int64_t SD_STAGE_ALIGN = 256;      // hipMalloc's own granularity

// Field i of bytes[i] bytes starts at offsets[i], a multiple of SD_STAGE_ALIGN, the fields one after another; returns the
// size of the block
inline int64_t sd_stage_layout(const int64_t* bytes, int count, int64_t* offsets) {
    int64_t total = 0;
    for (int i = 0; i < count; ++i) {
        offsets[i] = total;
        total += (bytes[i] + SD_STAGE_ALIGN - 1) / SD_STAGE_ALIGN * SD_STAGE_ALIGN;
    }
    return total;
}
