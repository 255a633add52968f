// int4_conv.hip -- a linear INT8 convolution with an INT4 weight (W4A8) that stays 4 bits wide up to the matrix unit: the instance of
// int8_conv.hpp on the B codec Q8B4 (int8_tile.hpp).  w [O, kh, kw, Cp / 2] holds two codes (-8 .. 7) per byte, the channels of a tap
// packed in the layout of DESIGN.md section 9.23; A is gathered exactly as for an int8 weight, the zero point's fill included, and the
// arithmetic is that of int4_gemm.hip.
#include "int8_conv.hpp"

using namespace ppqhip;

extern "C" int ppqhip_int4_conv2d(const int8_t* x, const uint8_t* w, const int32_t* w_sums, int zx, const float* mul, const float* bias,
                                  const float* residual, int relu, float* y, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding,
                                  int q_nan, int64_t n, int64_t c, int64_t h, int64_t wd, int64_t o, int64_t kh, int64_t kw,
                                  int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream) {
    const Int8TailHost t = {w_sums, zx, mul, bias, residual, relu, y, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_conv<Q8B4>("int4_conv2d", K_INT4_CONV, x, w, t, n, c, h, wd, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, stream);
}
