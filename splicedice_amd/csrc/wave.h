// Steps of one 64-lane wave that more than one translation unit needs: 64-bit shuffles, reductions and scans over the
// lanes, and the composite (key, index) compare of the counting sorts.  Device code only; nothing here touches memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- 64-bit shuffles: the two halves travel separately
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffu), mask);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
    const unsigned lo = (unsigned)__shfl_down((int)(unsigned)(v & 0xffffffffu), d);
    const unsigned hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)(v & 0xffffffffu), d);
    const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t bcast_lane0_u64(uint64_t v) {
    return ((uint64_t)(unsigned)__shfl((int)(unsigned)(v >> 32), 0) << 32) | (unsigned)__shfl((int)(unsigned)(v & 0xffffffffu), 0);
}

// ---- over all 64 lanes, the result in every lane
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint64_t y = shfl_xor_u64(v, o); v = y < v ? y : v; }
    return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint64_t y = shfl_xor_u64(v, o); v = y > v ? y : v; }
    return v;
}

// ---- scans (lane = this thread's lane, 0..63)
// inclusive suffix minimum: the minimum over the lanes at or after this one
__device__ __forceinline__ uint64_t wave_suffix_min_u64(uint64_t x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = shfl_down_u64(x, o);
        if (lane + o < 64) x = y < x ? y : x;
    }
    return x;
}
// inclusive prefix sum: the sum over the lanes at or before this one
__device__ __forceinline__ unsigned wave_prefix_sum(unsigned x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

// c += (ka, ia) < (kb, ib) in composite order: the borrow of the 96-bit subtraction, added with carry -- four VALU
// instructions (the compiler turns "ka < kb || (ka == kb && ia < ib)", and __builtin_subc chains too, into five compares
// and their mask arithmetic)
__device__ __forceinline__ void count_less96(unsigned& c, uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    unsigned t;
    asm("v_sub_co_u32 %0, vcc, %2, %3\n\t"
        "v_subb_co_u32 %0, vcc, %4, %5, vcc\n\t"
        "v_subb_co_u32 %0, vcc, %6, %7, vcc\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc"
        : "=&v"(t), "+v"(c)
        : "v"(ia), "v"(ib), "v"((unsigned)ka), "v"((unsigned)kb), "v"((unsigned)(ka >> 32)), "v"((unsigned)(kb >> 32))
        : "vcc");
}
