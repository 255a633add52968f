// int8_bmm.hip -- the batched matmul of two INT8 activations on the int8 MFMA (attention's Q.K^T and P.V): the entry point of
// int8_bmm.hpp, where the kernel is described.  DESIGN.md section 9.27.
#include "int8_bmm.hpp"

using namespace ppqhip;

extern "C" int ppqhip_int8_bmm(const int8_t* a, const int8_t* b, int transpose_b, int za, int zb, const float* mul, const float* residual,
                               int relu, float* c, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding, int q_nan,
                               int64_t batch, int64_t m, int64_t n, int64_t k, void* stream) {
    const Int8TailHost h = {nullptr, 0, mul, nullptr, residual, relu, c, q, sy, zy, qmin, qmax, rounding, q_nan};
    return q8_bmm(a, b, transpose_b, za, zb, h, batch, m, n, k, stream);
}
