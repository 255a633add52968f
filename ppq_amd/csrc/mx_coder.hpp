// mx_coder.hpp -- THE element coder of the packed MX export: block maximum, E8M0 scale code and element code,
// moved out of mx_pack.hip verbatim so that the fused epilogue of the block-scaled MFMA kernels (mx_mfma.hpp, section 9.16) packs
// with the code mx_pack.hip packs with.  One coder: the bytes of a fused launch are those of ppqhip_mx_pack by construction.
#pragma once

#include "common.hpp"
#include "mx_common.hpp"

namespace ppqhip {

__host__ __device__ constexpr uint32_t mx_elem_bits(uint32_t format) {            // width of an element code
    return format == PPQHIP_MXFP4_E2M1 ? 4u : (format == PPQHIP_MXFP6_E3M2 || format == PPQHIP_MXFP6_E2M3) ? 6u : 8u;
}

#if defined(__HIPCC__)

// what the element coder needs beyond MxFmt, all derived from it (wave-uniform)
struct MxCoder {
    uint32_t bits;             // 8, 6, 4
    uint32_t code_bias;        // (127 - bias) << m: a normal's code is (pattern >> shift) - code_bias
    bool is_int, has_nan;
};
__device__ __forceinline__ MxCoder make_coder(uint32_t format, const MxFmt& fmt) {
    MxCoder c;
    c.bits = mx_elem_bits(format);
    c.code_bias = ((fmt.sub_limit >> 23) - 1u) << (23u - fmt.shift);              // emin + 127 = 128 - bias
    c.is_int = format == PPQHIP_MXINT8;
    c.has_nan = format == PPQHIP_MXFP8_E4M3 || format == PPQHIP_MXFP8_E5M2;
    return c;
}

// the magnitude that takes part in the block maximum; in a format without a NaN encoding a NaN marks the whole block (kMxNaNBlock)
__device__ __forceinline__ uint32_t mxp_mag(float v, const MxCoder& c) {
    const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
    return m < 0x7f800000u ? m : (m > 0x7f800000u && !c.has_nan ? kMxNaNBlock : 0u);
}
// scale code and 1 / X of a block from the reduced mxp_mag
__device__ __forceinline__ uint32_t mxp_scale(uint32_t m, const MxFmt& f, float& inv, bool& dead) {
    dead = m == kMxNaNBlock;
    const uint32_t code = mx_code(dead ? 0u : m, f);
    inv = mx_pow2(254u - code);
    return dead ? 0xffu : code;
}
// the code of cast(v / X): read off the rounded pattern r.  On the fixed-point grid the code is the grid index r / quantum (exact);
// a normal's exponent and mantissa fields are the pattern's own, rebiased.  The sign comes from v (1 / X > 0).
__device__ __forceinline__ uint32_t mxp_code(float v, float inv, const MxFmt& f, const MxCoder& c) {
    const uint32_t vb = __float_as_uint(v), sign = vb >> 31;
    const uint32_t mag = __float_as_uint(v * inv) & 0x7fffffffu;
    const uint32_t r = mx_round(mag, f);
    const uint32_t k = (uint32_t)(__uint_as_float(r) * f.sub_scale);              // used below sub_limit only: 0 .. 127
    if (c.is_int) return (sign ? 0u - k : k) & 0xffu;
    uint32_t code = r < f.sub_limit ? k : (r >> f.shift) - c.code_bias;
    if ((vb & 0x7fffffffu) > 0x7f800000u) code = 0x7fu;                          // reached by MXFP8 only
    return code | (sign << (c.bits - 1u));
}

#endif  // __HIPCC__

}  // namespace ppqhip
