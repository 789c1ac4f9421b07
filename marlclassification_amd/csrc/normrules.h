// What the normalisation kernels and the colour kernel share (normalize.hip, color.hip; internal): the statistics
// record as a type, the check of the user pairs on the host, their derivation on the device, and the barrier that keeps
// a product rounded.  MARL_COLOR_OUT_NORM is defined as the colour launch followed by the user normalisation, bit for
// bit, so the two launches may not derive the pair in two places.  Both translation units are built with
// -ffp-contract=off (Makefile): the fp64 chain below rounds every operation.
#pragma once

#include "common.h"

#include "../../include/marl_hip_normalize.h"

namespace marl {
namespace {

// ---- the record: (S1, S2, min, max) of one plane, int64 for uint8 sources and double for fp32 sources ----------------
template <int ELT>
struct RecOf;
template <>
struct RecOf<1> {
    using T = int64_t;
};
template <>
struct RecOf<4> {
    using T = double;
};
template <class T>
struct Rec {
    T s1, s2, mn, mx;
};
static_assert(sizeof(Rec<int64_t>) == MARL_NORM_RECORD_BYTES && sizeof(Rec<double>) == MARL_NORM_RECORD_BYTES,
              "record layout");

// ---- host: the user pairs of a user mode, checked and copied into the argument struct ---------------------------------
// (m, s) or (lo, hi) per channel: finite, and a width (s, or hi - lo) that is finite and not 0
inline int user_pairs(const char* who, int mode, const double* user, int c, double (*pairs)[2]) {
    for (int ch = 0; ch < c; ++ch) {
        const double u0 = user[2 * ch], u1 = user[2 * ch + 1];
        const double width = mode == MARL_NORM_USER_NORMAL ? u1 : u1 - u0;
        if (!(u0 - u0 == 0.0) || !(u1 - u1 == 0.0) || !(width - width == 0.0) || width == 0.0) {  // (NaN, inf, 0)
            set_error("%s: user[%d] = (%g, %g): %s", who, ch, u0, u1,
                      mode == MARL_NORM_USER_NORMAL ? "s must be finite and not 0" : "hi - lo must be finite and not 0");
            return MARL_EINVAL;
        }
        pairs[ch][0] = u0, pairs[ch][1] = u1;
    }
    return MARL_OK;
}

// ---- device -----------------------------------------------------------------------------------------------------------
// (scale64, offset64) of channel ch under user mode `mode` (USER_NORMAL, else USER_MINMAX), from a.user; ELT == 1 folds
// ToTensor's / 255 in.  The caller rounds both once to fp32.
template <int ELT, class Args>
__device__ __forceinline__ void user_coef(const Args& a, int mode, int ch, double& sc, double& of) {
    constexpr double k255 = ELT == 1 ? 255.0 : 1.0;
    if (mode == MARL_NORM_USER_NORMAL) {
        const double m = a.user[ch][0], s = a.user[ch][1];
        sc = 1.0 / (k255 * s);
        of = -m / s;
    } else {
        const double lo = a.user[ch][0], d = a.user[ch][1] - lo;
        sc = 1.0 / (k255 * d);
        of = -lo / d;
    }
}

__device__ __forceinline__ float rounded(float v) {
    asm volatile("" : "+v"(v));  // (a sum sees a rounded product whatever the contraction setting)
    return v;
}

}  // namespace
}  // namespace marl
