// erfc in double-double arithmetic for the rank tests whose printed p has to be the correctly rounded float64:
// signedrank.hip (K13) and jonckheere.hip (K18).
#pragma once
#include "dd.h"

namespace {

// p where most rows of a rank test are (p >= 2.2e-5): erfc(x) from x^2 in double-double arithmetic, so that the float64
// that comes out is the correctly rounded one (the library erfc is an ulp or two off, which shows in the last printed
// digit of the table).  erfc(x) = 1 - 2/sqrt(pi) x sum_n (-x^2)^n / (n! (2n+1)) with x^2 a double-double quotient of the
// test's integers: up to x^2 = 9 the alternating terms grow to 56 and erfc falls to 2.2e-5, about 22 of the 106 bits;
// beyond that the library erfc.
// (This function compiled for the host, against mpmath: 0 of 5048 random (n', W2, T) and break points differ from the correctly
// rounded value.)
constexpr double SR_DD_X2_MAX = 9.0;
// coefficients (-1)^n / (n! (2n+1)) of the series as double-double constants; SR_ERF_TERMS[i] of them leave less than
// 2^-112 behind for x^2 <= SR_ERF_BREAK[i]
__device__ const double SR_ERF_C[70][2] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {-0x1.5555555555555p-2, -0x1.5555555555555p-56},
    {0x1.999999999999ap-4, -0x1.999999999999ap-58},
    {-0x1.8618618618618p-6, -0x1.8618618618618p-60},
    {0x1.2f684bda12f68p-8, 0x1.2f684bda12f68p-62},
    {-0x1.8d3018d3018d3p-11, -0x1.8d3018d3018d3p-71},
    {0x1.c01c01c01c01cp-14, 0x1.c01c01c01c01cp-74},
    {-0x1.bbd779334ef0bp-17, 0x1.4e65f77088199p-71},
    {0x1.87a00187a0018p-20, 0x1.e80061e80061fp-74},
    {-0x1.3777c55568ccdp-23, -0x1.aaabe22270001p-79},
    {0x1.c2e3054870b38p-27, -0x1.d5bceb1cfc09cp-81},
    {-0x1.2b67310aa9f3ap-30, -0x1.0a97d2e29d0a6p-85},
    {0x1.6f448e13e85e1p-34, -0x1.7f9c97a441499p-90},
    {-0x1.a289ee7e40f74p-38, 0x1.d70bcaede276bp-92},
    {0x1.bd577e658d020p-42, 0x1.20ed35aaf6f95p-97},
    {-0x1.bc6250fb14231p-46, 0x1.a5ccd0da99260p-100},
    {0x1.a173a167fba4dp-50, -0x1.4e2d0241b6a79p-104},
    {-0x1.7271cbe5863ecp-54, -0x1.12d42fe81b396p-108},
    {0x1.377c2110f2083p-58, 0x1.98394fbf35b19p-117},
    {-0x1.f1b4073b34a68p-63, 0x1.84a9e0b9a5e9bp-117},
    {0x1.7abd72258fb6ep-67, 0x1.2780872890580p-123},
    {-0x1.13246abce1bddp-71, -0x1.b85c8446def6cp-125},
    {0x1.7e6b81382cd42p-76, 0x1.f8367249eb893p-131},
    {-0x1.fd6bebd65107ap-81, -0x1.64abb94b856f1p-135},
    {0x1.45c0a838efe59p-85, -0x1.423cdb5cc4cc3p-139},
    {-0x1.909c9de3a31c5p-90, 0x1.889db7273c973p-145},
    {0x1.da7460554e5dbp-95, 0x1.59a4d60d2d7dap-149},
    {-0x1.0eef30fa10d2cp-99, 0x1.28594b7fcd32dp-153},
    {0x1.2ac65385f79acp-104, 0x1.03fafe0077abep-161},
    {-0x1.3e81bb5701ac5p-109, 0x1.209a8bade2337p-164},
    {0x1.4899fcdef0a8dp-114, -0x1.aec1a99185f98p-173},
    {-0x1.486eea20c2656p-119, 0x1.9ae3d63d0a79fp-173},
    {0x1.3e53defc4e233p-124, 0x1.d436dda5545e7p-178},
    {-0x1.2b778acc3dedfp-129, -0x1.f264aece2ab96p-184},
    {0x1.11ae81077a49ep-134, -0x1.f8cb0d503e384p-189},
    {-0x1.e6597092ccbf0p-140, -0x1.d930aabd4497fp-197},
    {0x1.a47767f2a3c32p-145, 0x1.eb53c552fbc05p-201},
    {-0x1.61f30bc3acd1ap-150, -0x1.a9e9f60cd9edap-204},
    {0x1.22521d98f98a9p-155, -0x1.637b9778df025p-209},
    {-0x1.d05cc9e3507c9p-161, 0x1.29b6f9c13f797p-215},
    {0x1.6a513f56f8a2fp-166, -0x1.8794747d7f461p-220},
    {-0x1.13f85fc9e143ep-171, -0x1.27bd43d20fbfcp-225},
    {0x1.9aa19d4d16643p-177, -0x1.ad0ff92af832dp-231},
    {-0x1.2a8fa59ffec31p-182, 0x1.44478f2f75d87p-236},
    {0x1.a8830736a5123p-188, -0x1.1af9ae0a12e66p-245},
    {-0x1.273d8edcec957p-193, 0x1.ab7b8539d42f6p-249},
    {0x1.91ef82b367a95p-199, 0x1.690b4eaa147d4p-254},
    {-0x1.0be5a4cd94283p-204, 0x1.fbd6d97519e8fp-258},
    {0x1.5dd4c9219115ap-210, 0x1.73661ef9ff986p-264},
    {-0x1.bfb10e0f68c50p-216, 0x1.159dc3de3de07p-273},
    {0x1.18d952ef00889p-221, -0x1.8e04468edd83dp-278},
    {-0x1.59982b2e94840p-227, 0x1.68a4cb414cb71p-281},
    {0x1.a13ec00b39f6fp-233, -0x1.af38c63806b25p-288},
    {-0x1.ee6cefaa5a158p-239, 0x1.7a47a5ca12246p-293},
    {0x1.1f9dec94da5f8p-244, -0x1.6472662f16fe2p-298},
    {-0x1.48a6b3820b441p-250, 0x1.df79984d16d0dp-305},
    {0x1.70f41ac13e2a1p-256, 0x1.8af98ff8f9fd6p-310},
    {-0x1.970f1cb2ad53fp-262, -0x1.b7fc559391cc2p-316},
    {0x1.b97d90d3e603bp-268, 0x1.1965394a5d61cp-323},
    {-0x1.d6db2a7c68dcbp-274, 0x1.f1ad59160452ep-329},
    {0x1.edf1e6e4658a9p-280, -0x1.3aa36c1523b23p-334},
    {-0x1.fdcf88bbf71dbp-286, 0x1.6f1a1abfe27e7p-342},
    {0x1.02eb04e5f82f5p-291, 0x1.98847a7286982p-349},
    {-0x1.02e2bc1b5790ep-297, 0x1.6a12f5351a054p-352},
    {0x1.fdbe706576d5dp-304, -0x1.2ce505402f725p-358},
    {-0x1.ee3d33862f55bp-310, 0x1.f1da0c3f22056p-366},
    {0x1.d80e20102c46ep-316, -0x1.a560ae14c0c74p-372},
    {-0x1.bc3cf47bca3afp-322, 0x1.82f01ff45da58p-385},
    {0x1.9c00b17fe33c8p-328, -0x1.bc97c630526bcp-383},
    {-0x1.78a61f51a767fp-334, -0x1.1fcc8fc30c961p-388},
};
__device__ const double SR_ERF_BREAK[8] = {0.25, 0.5, 1, 2, 3, 4.5, 6, 9};
__device__ const int SR_ERF_TERMS[8] = {21, 25, 30, 37, 43, 50, 57, 69};

__device__ double erfc_dd_x2(const DD x2) {                                 // 0 < x2 <= SR_DD_X2_MAX
    // (dd_sqrt written out: called, it swaps the operands of one v_add_f64 in the lane and group kernels)
    const double s = sqrt(x2.hi);
    const DD x = dd_fast2sum(s, (__builtin_fma(-s, s, x2.hi) + x2.lo) / (2.0 * s));
    int last = SR_ERF_TERMS[7];
#pragma unroll
    for (int i = 6; i >= 0; --i)
        if (x2.hi <= SR_ERF_BREAK[i]) last = SR_ERF_TERMS[i];
    DD sum = {SR_ERF_C[last][0], SR_ERF_C[last][1]};                     // Horner in x^2, no division
    for (int n = last - 1; n >= 0; --n) sum = dd_add(dd_mul(sum, x2), {SR_ERF_C[n][0], SR_ERF_C[n][1]});
    const DD two_over_sqrt_pi = {0x1.20dd750429b6dp+0, 0x1.1ae3a914fed80p-56};
    const DD erf = dd_mul(dd_mul(two_over_sqrt_pi, x), sum);
    const DD r = dd_add({1.0, 0.0}, {-erf.hi, -erf.lo});
    return r.hi + r.lo;
}

}  // namespace
