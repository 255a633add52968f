// to_int.hpp -- one value to its integer code, PPQLinearQuant_toInt's arithmetic: shared by the export kernels of linear.hip
// (ppqhip_to_int_t / _c) and the re-quantising epilogue of the linear INT8 kernels (int8_tile.hpp), which must
// give the same bits.
#pragma once

#include "common.hpp"

namespace ppqhip {

#if defined(__HIPCC__)

// PPQLinearQuant_toInt, ppq/quantization/qfunction/linear.py:218-238 (the reference does this with torch ops; it
// has no kernel for it): q = clamp(ppq_tensor_round(x / s) + o, qmin, qmax) in FLOAT32 -- the RAW offset, not the
// rounded one the fake-quant kernels use -- then .type(int8 | uint8 | int32), i.e. truncation towards zero.
// ppq_tensor_round (utils/round.py:9-49) is a float32 formula per policy, not common.cuh's _round2int.
__device__ __forceinline__ float tensor_round_f32(float v, int rounding) {
    const float sgn = v > 0.f ? 1.f : (v < 0.f ? -1.f : v);           // torch.sign: 0 -> 0, NaN -> NaN
    switch (rounding) {
        case ROUND_HALF_EVEN: return __builtin_rintf(v);
        case ROUND_UP: return __builtin_ceilf(v);
        case ROUND_HALF_TOWARDS_ZERO: return sgn * __builtin_ceilf(__builtin_fabsf(v) - 0.5f);
        case ROUND_HALF_FAR_FORM_ZERO: return sgn * __builtin_floorf(__builtin_fabsf(v) + 0.5f);
        case ROUND_HALF_DOWN: return __builtin_ceilf(v - 0.5f);
        default: return __builtin_floorf(v + 0.5f);                    // ROUND_HALF_UP
    }
}
__device__ __forceinline__ int to_int_scalar(float x, float s, float o, float qmin, float qmax, int rounding) {
    float t = tensor_round_f32(x / s, rounding) + o;
    t = t < qmin ? qmin : t;            // torch.clamp: NaN stays NaN (both compares false)
    t = t > qmax ? qmax : t;
    return f2i_sat(t);                  // truncates; NaN -> 0
}

#endif  // __HIPCC__

}  // namespace ppqhip
