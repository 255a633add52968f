// int8_gemm.hip -- a linear INT8 layer as an integer backend runs it, with an int8 weight: the instance of int8_gemm.hpp on the B codec
// Q8B8 (int8_tile.hpp), where the kernel, its operands and the entry point's checks are described.  DESIGN.md section 9.22.
#include "int8_gemm.hpp"

using namespace ppqhip;

extern "C" int ppqhip_int8_gemm(const int8_t* a, const int8_t* b, const int32_t* b_sums, int zx, const float* mul, const float* bias,
                                const float* residual, int relu, float* c, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding,
                                int q_nan, int64_t m, int64_t n, int64_t k, void* stream) {
    const Int8TailHost h = {b_sums, zx, mul, bias, residual, relu, c, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_gemm<Q8B8>("int8_gemm", K_INT8_GEMM, a, b, h, m, n, k, stream);
}
