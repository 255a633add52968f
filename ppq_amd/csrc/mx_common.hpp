// mx_common.hpp -- what the MX fake-quant kernels (mx.hip) and the packed MX export (mx_pack.hip) share: the description of an
// element format, the E8M0 code of a block and THE rounding of an element.  Both paths take the rounded float32 pattern from
// mx_round, so the packed codes can never disagree with the fake-quantised values on a rounding.
// Round tuning on the element grid (mx_roundtune.hip) takes the block's code from the same functions and the two neighbours of an
// element from mx_floor / mx_up below.
#pragma once

#include "common.hpp"

namespace ppqhip {

struct MxFmt {                 // 28 B
    uint32_t emax;             // the element format's largest exponent: the shared exponent is exponent(amax) - emax
    uint32_t shift;            // 23 - mantissa bits: float32 mantissa bits a normal element drops
    uint32_t half_m1;          // (1 << (shift - 1)) - 1: with the kept LSB added, a carry out of the dropped bits <=> round up (RNE)
    uint32_t sub_limit;        // |u| patterns below this are on the format's fixed-point grid (its subnormals; all of MXINT8)
    float sub_scale;           // 1 / that grid's spacing
    float sub_quantum;         // the grid's spacing
    uint32_t max_bits;         // pattern of the largest normal
};

constexpr uint32_t f32_bits(int exponent) { return (uint32_t)(exponent + 127) << 23; }      // 2^exponent, -126 <= exponent <= 127

// float formats: mantissa bits m, smallest normal exponent emin = 1 - bias, largest normal (2 - 2^-m) 2^emax -- E4M3 gives its
// all-ones mantissa at emax to NaN, so its largest normal is 1.75 * 2^8
inline bool make_mx_fmt(int format, MxFmt* f) {
    int m, emin, emax;
    uint32_t top_mantissa;     // mantissa field of the largest normal, in m bits
    switch (format) {
        case PPQHIP_MXFP8_E4M3: m = 3; emin = -6; emax = 8; top_mantissa = 6; break;
        case PPQHIP_MXFP8_E5M2: m = 2; emin = -14; emax = 15; top_mantissa = 3; break;
        case PPQHIP_MXFP6_E3M2: m = 2; emin = -2; emax = 4; top_mantissa = 3; break;
        case PPQHIP_MXFP6_E2M3: m = 3; emin = 0; emax = 2; top_mantissa = 7; break;
        case PPQHIP_MXFP4_E2M1: m = 1; emin = 0; emax = 2; top_mantissa = 1; break;
        case PPQHIP_MXINT8:                                                      // k / 64, |k| <= 127: one fixed-point grid
            f->emax = 0; f->shift = 17; f->half_m1 = (1u << 16) - 1u; f->sub_limit = 0x7f800000u;
            f->sub_scale = 64.0f; f->sub_quantum = 0.015625f; f->max_bits = f32_bits(0) | (63u << 17);      // 127 / 64
            return true;
        default: return false;
    }
    f->emax = (uint32_t)emax; f->shift = (uint32_t)(23 - m); f->half_m1 = (1u << (22 - m)) - 1u;
    f->sub_limit = f32_bits(emin);
    union { uint32_t d; float v; } s, q;
    s.d = f32_bits(m - emin); q.d = f32_bits(emin - m);
    f->sub_scale = s.v; f->sub_quantum = q.v;
    f->max_bits = f32_bits(emax) | (top_mantissa << (23 - m));
    return true;
}

// `format` as the scale-making entry points take it: the format in the low byte, the scale rule (PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE,
// DESIGN.md section 9.17) above it.  False: a negative value or a rule nobody knows.
inline bool split_mx_format(int format, int* fmt, uint32_t* rule) {
    if (format < 0 || (format >> PPQHIP_MX_RULE_SHIFT) > PPQHIP_MX_MSE) return false;
    *fmt = format & ((1 << PPQHIP_MX_RULE_SHIFT) - 1);
    *rule = (uint32_t)(format >> PPQHIP_MX_RULE_SHIFT);
    return true;
}

// The instantiation a launch of the scale-making kernels needs: the floor rule's own code, the rules that read nothing but the amax
// (CEIL, EVEN) added, or the MSE search as well -- the search keeps two float64 sums and a second cast in registers, which the other
// rules should not pay for.  A launch of many jobs takes the largest class among them.
enum : int { MX_PLAIN = 0, MX_AMAX_RULES = 1, MX_SEARCH = 2 };
inline int mx_rule_class(uint32_t rule) { return rule == PPQHIP_MX_MSE ? MX_SEARCH : rule != PPQHIP_MX_FLOOR ? MX_AMAX_RULES : MX_PLAIN; }

constexpr uint32_t kMxBlock = 32;                 // elements per MX block
constexpr int kMxMaxJobs = 40;                    // jobs of one launch (the table travels in the kernel arguments)
constexpr int64_t kMxMax = 0x7fffffffLL;          // elements of one tensor
constexpr uint32_t kMxNaNBlock = 0xffffffffu;     // a block maximum above every magnitude: the block is NaN as a whole (mx_coder.hpp)

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t mx_finite_mag(float v) {                     // |v|'s pattern; NaN and Inf do not take part
    const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
    return m < 0x7f800000u ? m : 0u;
}
// E8M0 code of a block from the pattern of its amax: a subnormal or zero amax has exponent field 0 and clamps to code 0 (2^-127)
__device__ __forceinline__ uint32_t mx_code(uint32_t amax_bits, const MxFmt& f) {
    const uint32_t e = amax_bits >> 23;
    return e > f.emax ? e - f.emax : 0u;
}
__device__ __forceinline__ float mx_pow2(uint32_t biased) {                      // 2^(biased - 127), 0 <= biased <= 254
    return __uint_as_float(biased ? biased << 23 : 0x00400000u);
}
// The cast of |u| = |v / X| on its float32 pattern.  Normal elements: round the mantissa to nearest even with one integer add (the
// carry runs into the exponent as it should); the fixed-point grid: rint() of the scaled magnitude (round half to even = the even
// encoding); both saturate at the largest normal, which also takes Inf.  (A NaN pattern gives a pattern nobody may use.)
__device__ __forceinline__ uint32_t mx_round(uint32_t mag, const MxFmt& f) {
    const uint32_t rn = (mag + f.half_m1 + ((mag >> f.shift) & 1u)) & ~((1u << f.shift) - 1u);
    const uint32_t rs = __float_as_uint(__builtin_rintf(__uint_as_float(mag) * f.sub_scale) * f.sub_quantum);
    return min(mag < f.sub_limit ? rs : rn, f.max_bits);
}
// The two element values that enclose |u|, on float32 patterns as mx_round works.  mx_floor: the largest
// element magnitude <= mag -- normal elements drop the mantissa bits below the format's, the fixed-point grid takes floorf() of the
// scaled magnitude; Inf and anything above the largest normal give the largest normal.  mx_up: the element magnitude above the
// element magnitude `lo` -- one quantum on the fixed-point grid (its last step lands on the smallest normal), one mantissa step
// above it (the carry runs into the exponent as it should); the largest normal stays where it is.
__device__ __forceinline__ uint32_t mx_floor(uint32_t mag, const MxFmt& f) {
    const uint32_t fn = mag & ~((1u << f.shift) - 1u);
    const uint32_t fs = __float_as_uint(__builtin_floorf(__uint_as_float(mag) * f.sub_scale) * f.sub_quantum);
    return min(mag < f.sub_limit ? fs : fn, f.max_bits);
}
__device__ __forceinline__ uint32_t mx_up(uint32_t lo, const MxFmt& f) {
    const uint32_t un = lo + (1u << f.shift);
    const uint32_t us = __float_as_uint(__uint_as_float(lo) + f.sub_quantum);
    return min(lo < f.sub_limit ? us : un, f.max_bits);
}
// cast(v / X) * X
__device__ __forceinline__ float mx_elem(float v, float inv, float X, const MxFmt& f) {
    const float u = v * inv;
    const uint32_t bits = __float_as_uint(u), sign = bits & 0x80000000u, mag = bits & 0x7fffffffu;
    const float q = __uint_as_float(mx_round(mag, f) | sign) * X;
    return mag > 0x7f800000u ? v : q;
}

// THE scale rule: the block's code from the pattern of its amax under the three rules that need nothing
// but the amax -- for PPQHIP_MX_MSE this is its first candidate, the floor code.  Every result is in 0 .. 254.
//   CEIL  the floor code, one more when amax / X lies above the largest normal (the product is exact: X is a power of two)
//   EVEN  the floor code of amax rounded to the element's precision: half an element ULP added to the pattern
__device__ __forceinline__ uint32_t mx_rule_code(uint32_t amax_bits, const MxFmt& f, uint32_t rule) {
    const uint32_t floor_code = mx_code(amax_bits, f);
    if (rule == PPQHIP_MX_CEIL) {
        const uint32_t scaled = __float_as_uint(__uint_as_float(amax_bits) * mx_pow2(254u - floor_code));
        return min(floor_code + (scaled > f.max_bits ? 1u : 0u), 254u);
    }
    if (rule == PPQHIP_MX_EVEN) return min(mx_code(amax_bits + f.half_m1 + 1u, f), 254u);
    return floor_code;
}

// PPQHIP_MX_MSE: the squared error of a block under the floor code c0 and under c1 = min(c0 + 1, 254), over its finite elements.
// d = cast(v / X) * X - v is exact in float32 (section 9.17), its square exact in float64; the two sums run through the same adds in
// the same order, so two candidates that quantise alike give equal sums, and the strict comparison keeps c0.
struct MxMse {
    uint32_t c0, c1;
    float X0, inv0, X1, inv1;
    double e0, e1;
    __device__ __forceinline__ explicit MxMse(uint32_t floor_code)
        : c0(floor_code), c1(min(floor_code + 1u, 254u)), X0(mx_pow2(c0)), inv0(mx_pow2(254u - c0)), X1(mx_pow2(c1)),
          inv1(mx_pow2(254u - c1)), e0(0.0), e1(0.0) {}
    __device__ __forceinline__ void add(float v, bool counts, const MxFmt& f) {
        const bool finite = counts && (__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u;
        const float d0 = mx_elem(v, inv0, X0, f) - v, d1 = mx_elem(v, inv1, X1, f) - v;
        e0 += finite ? (double)d0 * (double)d0 : 0.0;
        e1 += finite ? (double)d1 * (double)d1 : 0.0;
    }
    // the sums of the LANES lanes that share the block (a butterfly: every lane ends with the same bits, an add commutes)
    template <int LANES>
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int s = LANES / 2; s > 0; s >>= 1) { e0 += __shfl_xor(e0, s, 64); e1 += __shfl_xor(e1, s, 64); }
    }
    __device__ __forceinline__ uint32_t code() const { return e1 < e0 ? c1 : c0; }
};

#endif  // __HIPCC__

}  // namespace ppqhip
