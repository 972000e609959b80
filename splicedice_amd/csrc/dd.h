// Double-double arithmetic (a value as an unevaluated sum hi + lo of two float64, about 106 bits) for the last step of
// the rank tests whose printed p has to be the correctly rounded float64: signedrank.hip's erfc series, spearman.hip's
// rho and incomplete-beta series.  Built with -ffp-contract=off: every fma here is written out.
#pragma once
#include "common.h"
#include <math.h>

namespace {

struct DD { double hi, lo; };
__host__ __device__ inline DD dd_fast2sum(double a, double b) {            // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
__host__ __device__ inline DD dd_2sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ inline DD dd_add(DD a, DD b) {
    DD s = dd_2sum(a.hi, b.hi);
    const DD t = dd_2sum(a.lo, b.lo);
    s = dd_fast2sum(s.hi, s.lo + t.hi);
    return dd_fast2sum(s.hi, s.lo + t.lo);
}
__host__ __device__ inline DD dd_mul(DD a, DD b) {
    const double p = a.hi * b.hi;
    const double e = __builtin_fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return dd_fast2sum(p, e);
}
__host__ __device__ inline DD dd_mul_d(DD a, double b) {
    const double p = a.hi * b;
    const double e = __builtin_fma(a.hi, b, -p) + a.lo * b;
    return dd_fast2sum(p, e);
}
// a / b for a float64 b, in two roundings that are NOT interchangeable: the tables of `--paired` and `correlate` are
// byte for byte what they are with the form each was written with
__host__ __device__ inline DD dd_div_d(DD a, double b) {                   // two divisions (signedrank.hip)
    const double q1 = a.hi / b;
    const double r = __builtin_fma(-q1, b, a.hi) + a.lo;
    return dd_fast2sum(q1, r / b);
}
__host__ __device__ inline DD dd_div_d_recip(DD a, double b) {             // one: the residual step absorbs q1's error (spearman.hip)
    const double inv = 1.0 / b, q1 = a.hi * inv;
    const double r = __builtin_fma(-q1, b, a.hi) + a.lo;
    return dd_fast2sum(q1, r * inv);
}
__host__ __device__ inline DD dd_div(DD a, DD b) {
    const double q1 = a.hi / b.hi;
    DD r = dd_add(a, dd_mul_d(b, -q1));
    const double q2 = r.hi / b.hi;
    r = dd_add(r, dd_mul_d(b, -q2));
    const double q3 = r.hi / b.hi;
    const DD q = dd_fast2sum(q1, q2);
    return dd_fast2sum(q.hi, q.lo + q3);
}
__host__ __device__ inline DD dd_sqrt(DD a) {                              // a > 0
    const double s = sqrt(a.hi);
    return dd_fast2sum(s, (__builtin_fma(-s, s, a.hi) + a.lo) / (2.0 * s));
}
__host__ __device__ inline DD dd_u128(unsigned __int128 v) {               // exact below 2^106
    const uint64_t lo = (uint64_t)v;
    const DD top = dd_2sum((double)(uint64_t)(v >> 64) * 18446744073709551616.0, (double)(lo >> 32) * 4294967296.0);
    return dd_add(top, {(double)(lo & 0xffffffffull), 0.0});
}
}  // namespace
