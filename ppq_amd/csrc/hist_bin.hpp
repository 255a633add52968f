// hist_bin.hpp -- the bin rule of the calibration histograms, shared by every kernel that counts values into them: hist.hip's
// kernels and the histogram sinks of the convolution epilogues (epilogue.hip).  One definition, so that a value lands in the
// same bin whoever bins it: b = floor(|x| / hist_scale) [sym] or floor((x - min) / hist_scale) [asym] with the IEEE
// quotient and a saturating float->int conversion (NaN -> bin 0); clipping / clamping and the hot bin are WaveBinCounter's
// (common.hpp).
#pragma once
#include "common.hpp"

namespace ppqhip {

typedef float v2f __attribute__((ext_vector_type(2)));

// floor(RN(a / hs)) without the 11-instruction IEEE division on the common path.
//   t = RN(a * RN(1/hs)) differs from q = RN(a / hs) by less than |t| * 0.8 * 2^-22 (two roundings of
//   2^-24 relative for t, one for q), so floor(t) != floor(q) requires an integer within that distance
//   of t -- necessarily rint(t).  When |t - rint(t)| >= |t| * 2^-22 (an exact float test: the
//   difference is exact and the bound is a power-of-two scaling) the floors are provably equal;
//   otherwise (a few lanes in 10^4, plus every inf / NaN / huge outlier / degenerate hs) the lane
//   takes the true division.  The result is therefore ALWAYS the reference's floor(a / hs).
//   (The test is sign symmetric, so the symmetric rule may run it on x * rcp and use |t| afterwards.)
__device__ __forceinline__ bool quotient_is_safe(float t) {
    return __builtin_fabsf(t - __builtin_rintf(t)) >= __builtin_fabsf(t) * 0x1p-22f;
}

// truncation of |t|: == floor for the symmetric rule's non-negative quotient (saturating, NaN -> 0)
__device__ __forceinline__ int f2i_abs(float t) {
    int r;
    asm("v_cvt_i32_f32_e64 %0, |%1|" : "=v"(r) : "v"(t));
    return r;
}
// floor + convert in one instruction; only ever sees finite |t| < 2^23 (everything else took the
// true-division path, which converts with floorf + v_cvt_i32_f32 like round 1)
__device__ __forceinline__ int f2i_floor(float t) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(t));
    return r;
}

// Per-wavefront accumulator over one LDS histogram copy.  ASYM / CLIP specialise the bin rule, HOT
// enables the hot-bin register.
template <bool ASYM, bool CLIP, bool HOT>
struct Binner : WaveBinCounter<ASYM, CLIP, HOT> {
    using Base = WaveBinCounter<ASYM, CLIP, HOT>;
    using Base::h; using Base::last; using Base::hot_bin; using Base::hot_cnt;
    float a0, hs, rcp;

    __device__ __forceinline__ void set_rule(float a, float scale) { a0 = a; hs = scale; rcp = 1.0f / scale; }

    // slots of four values.  Returns bins with the reference's conversion semantics; `exact` lanes
    // (special values) already went through floorf + saturating convert.
    __device__ __forceinline__ void bins4(const float4& v, int (&b)[4]) const {
        v2f x01 = {v.x, v.y}, x23 = {v.z, v.w};
        if (ASYM) { x01 = x01 - a0; x23 = x23 - a0; }
        const v2f t01 = x01 * rcp, t23 = x23 * rcp;
        const v2f r01 = {__builtin_rintf(t01.x), __builtin_rintf(t01.y)};
        const v2f r23 = {__builtin_rintf(t23.x), __builtin_rintf(t23.y)};
        const v2f d01 = t01 - r01, d23 = t23 - r23;
        const v2f e01 = t01 * 0x1p-22f, e23 = t23 * 0x1p-22f;
        // u_k: lane k is NOT provably safe (also true for NaN: the comparison is unordered)
        const bool u0 = !(__builtin_fabsf(d01.x) >= __builtin_fabsf(e01.x));
        const bool u1 = !(__builtin_fabsf(d01.y) >= __builtin_fabsf(e01.y));
        const bool u2 = !(__builtin_fabsf(d23.x) >= __builtin_fabsf(e23.x));
        const bool u3 = !(__builtin_fabsf(d23.y) >= __builtin_fabsf(e23.y));
        b[0] = ASYM ? f2i_floor(t01.x) : f2i_abs(t01.x);
        b[1] = ASYM ? f2i_floor(t01.y) : f2i_abs(t01.y);
        b[2] = ASYM ? f2i_floor(t23.x) : f2i_abs(t23.x);
        b[3] = ASYM ? f2i_floor(t23.y) : f2i_abs(t23.y);
        if (u0 | u1 | u2 | u3) {                // rare: some lane sits next to a bin boundary
            if (u0) b[0] = exact_bin(ASYM ? x01.x : __builtin_fabsf(v.x));
            if (u1) b[1] = exact_bin(ASYM ? x01.y : __builtin_fabsf(v.y));
            if (u2) b[2] = exact_bin(ASYM ? x23.x : __builtin_fabsf(v.z));
            if (u3) b[3] = exact_bin(ASYM ? x23.y : __builtin_fabsf(v.w));
        }
    }
    __device__ __forceinline__ int exact_bin(float a) const { return f2i_sat(__builtin_floorf(a / hs)); }

    __device__ __forceinline__ int bin1(float v) const {
        const float a = ASYM ? (v - a0) : __builtin_fabsf(v);
        const float t = a * rcp;
        if (quotient_is_safe(t)) return ASYM ? f2i_floor(t) : f2i_abs(t);
        return exact_bin(a);
    }

};

}  // namespace ppqhip
