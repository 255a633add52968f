// int4_gemm.hip -- a linear INT8 layer with an INT4 weight (W4A8) that stays 4 bits wide up to the matrix unit: the instance of
// int8_gemm.hpp on the B codec Q8B4 (int8_tile.hpp).  B [N, Kp / 2] holds two codes (-8 .. 7) per byte in the layout of DESIGN.md
// section 9.23; the MFMAs multiply 16 w, the accumulators start at -16 zx sums[n] (sums of the TRUE codes) and are shifted right by 4,
// exactly, before the epilogue of the int8 layer runs on them unchanged.
#include "int8_gemm.hpp"

using namespace ppqhip;

extern "C" int ppqhip_int4_gemm(const int8_t* a, const uint8_t* b, const int32_t* b_sums, int zx, const float* mul, const float* bias,
                                const float* residual, int relu, float* c, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding,
                                int q_nan, int64_t m, int64_t n, int64_t k, void* stream) {
    const Int8TailHost h = {b_sums, zx, mul, bias, residual, relu, c, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_gemm<Q8B4>("int4_gemm", K_INT4_GEMM, a, b, h, m, n, k, stream);
}
