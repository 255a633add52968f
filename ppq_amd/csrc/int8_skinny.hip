// int8_skinny.hip -- the linear INT8 GEMM for 1 <= M <= 64 rows, with an int8 weight or a packed int4 one: the two instances of
// int8_skinny.hpp, where the kernel is described.  Operands, contract and bits are those of ppqhip_int8_gemm / ppqhip_int4_gemm.
// DESIGN.md section 9.26.
#include "int8_skinny.hpp"

using namespace ppqhip;

extern "C" int ppqhip_int8_gemm_skinny(const int8_t* a, const int8_t* b, const int32_t* b_sums, int zx, const float* mul, const float* bias,
                                       const float* residual, int relu, float* c, int8_t* q, float sy, int zy, int qmin, int qmax,
                                       int rounding, int q_nan, int64_t m, int64_t n, int64_t k, void* stream) {
    const Int8TailHost h = {b_sums, zx, mul, bias, residual, relu, c, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_skinny<SkB8>("int8_gemm_skinny", K_INT8_SKINNY, a, b, h, m, n, k, stream);
}

extern "C" int ppqhip_int4_gemm_skinny(const int8_t* a, const uint8_t* b, const int32_t* b_sums, int zx, const float* mul, const float* bias,
                                       const float* residual, int relu, float* c, int8_t* q, float sy, int zy, int qmin, int qmax,
                                       int rounding, int q_nan, int64_t m, int64_t n, int64_t k, void* stream) {
    const Int8TailHost h = {b_sums, zx, mul, bias, residual, relu, c, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_skinny<SkB4>("int4_gemm_skinny", K_INT4_SKINNY, a, b, h, m, n, k, stream);
}
