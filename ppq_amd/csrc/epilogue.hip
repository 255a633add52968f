// epilogue.hip -- the elementwise tail of a convolution in ONE pass over HBM: per-channel bias, optional residual Add,
// optional ReLU.  PyTorch's MIOpen path runs a convolution without bias and then `output.add_(bias)`; the graph then runs
// `Add` and `Relu` as two more elementwise kernels.  Per ResNet-50 forward at batch 32 those three ops are 118 launches that
// move 7.4 GB; fused they are 49 launches and 4.1 GB.
//
// Bitwise the PyTorch sequence:
//   * every add is one rounded fp32 `x + y` in the operand order of the op it replaces (-ffp-contract=off, Makefile);
//   * ReLU is clamp_min's lambda, `isnan(v) ? v : ::max(v, 0.f)` (HIP's float ::max is __builtin_fmaxf): NaN keeps its
//     payload, and -0.0 / +0.0 come out as the same instruction makes them there.
//
// Geometry: channel(i) = (i / elem_per_channel) % num_channel (NCHW: C, H*W; channels-last: C, 1), computed with the
// invariant-divisor multiply of common.hpp (FastDiv), never a 64-bit divide.  When elem_per_channel % 4 == 0 (every NCHW
// plane except 7x7 / odd ones) a float4 never straddles a channel: one channel index per 16-B access.  Otherwise each of
// the four lanes of the float4 finds its own channel (stage-4 7x7 planes, channels-last).
//
// Streaming: 16-B loads and stores, U float4 per lane in flight (clamped, branch-free loads; predicated stores, as in
// linear.hip's tile kernels), one workgroup per tile, grid sized to the tensor.  No atomics, no inter-workgroup sync: the
// launch only enqueues on `stream` and is capturable into a HIP graph.  n % 4 trailing elements (odd tensors) are done by
// workgroup 0; a tensor with a pointer that is not 16-B aligned takes the element-wise kernel.
#include "common.hpp"

namespace ppqhip {
namespace {

constexpr int kEpTileU = 2;                        // HBM-bound tensors (3 .. 103 MB here): two float4 per lane in flight
constexpr int kEpSmallU = 1;                       // small ones are one latency chain: more waves, less work behind each load
constexpr long long kEpSmallElems = 1ll << 20;     // <= 4 MB per operand

struct EpArgs {
    float* a;              // bias_act: y
    const float* bias_a;
    float* b;              // residual operand (nullptr for bias_act)
    const float* bias_b;   // nullptr: b is read as is
    float* out;            // bias_add_act only
    uint32_t nvec;         // float4 count of the vector part
    uint32_t tail;         // first element of the scalar tail (== 4 * nvec)
    int ntail;             // n % 4 (vector kernel) or n (element-wise kernel)
    FastDiv epc;           // elem_per_channel (per-element channel) or elem_per_channel / 4 (per-float4 channel)
    FastDiv nc;            // num_channel
};

__device__ __forceinline__ uint32_t channel_of(uint32_t i, const FastDiv& epc, const FastDiv& nc) {
    const uint32_t row = fdiv(i, epc);
    return row - fdiv(row, nc) * nc.d;
}

__device__ __forceinline__ float act(float v, bool relu) {
    return (relu && !__builtin_isnan(v)) ? __builtin_fmaxf(v, 0.f) : v;
}

__device__ __forceinline__ float4 add4(const float4& x, const float4& y) {
    return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

template <bool RELU>
__device__ __forceinline__ float4 act4(const float4& v) {
    return make_float4(act(v.x, RELU), act(v.y, RELU), act(v.z, RELU), act(v.w, RELU));
}

// bias of the four elements of float4 number v
template <bool PLANE>
__device__ __forceinline__ float4 bias4(const float* __restrict__ bias, uint32_t v, const FastDiv& epc, const FastDiv& nc) {
    if (PLANE) {
        const float t = bias[channel_of(v, epc, nc)];
        return make_float4(t, t, t, t);
    }
    const uint32_t i = v * 4u;
    return make_float4(bias[channel_of(i, epc, nc)], bias[channel_of(i + 1, epc, nc)], bias[channel_of(i + 2, epc, nc)],
                       bias[channel_of(i + 3, epc, nc)]);
}

// one element i (channel from the per-element geometry `epc`)
template <bool RESID, bool BIAS_B, bool RELU>
__device__ __forceinline__ void epilogue_elem(const EpArgs& p, uint32_t i, const FastDiv& epc) {
    const uint32_t c = channel_of(i, epc, p.nc);
    const float x = p.a[i] + p.bias_a[c];
    if (!RESID) { p.a[i] = act(x, RELU); return; }
    p.a[i] = x;
    float y = p.b[i];
    if (BIAS_B) { y = y + p.bias_b[c]; p.b[i] = y; }
    p.out[i] = act(x + y, RELU);
}

// RESID = false: a = act(a + bias_a[c]).  RESID = true: a += bias_a[c]; (BIAS_B) b += bias_b[c]; out = act(a + b).
// PLANE: elem_per_channel % 4 == 0 and p.epc holds elem_per_channel / 4.  The tail (n % 4 != 0) implies !PLANE.
template <int U, bool RESID, bool BIAS_B, bool RELU, bool PLANE>
__global__ __launch_bounds__(kBlock) void epilogue_kernel(EpArgs p) {
    const uint32_t base = blockIdx.x * (kBlock * U) + threadIdx.x;
    float4* a4 = reinterpret_cast<float4*>(p.a);
    float4* b4 = reinterpret_cast<float4*>(p.b);
    float4* o4 = reinterpret_cast<float4*>(p.out);
    float4 a[U], ba[U], b[U], bb[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
        const uint32_t vv = min(base + k * kBlock, p.nvec - 1);      // clamped: all loads issue back to back
        a[k] = a4[vv];
        ba[k] = bias4<PLANE>(p.bias_a, vv, p.epc, p.nc);
        if (RESID) b[k] = b4[vv];
        if (BIAS_B) bb[k] = bias4<PLANE>(p.bias_b, vv, p.epc, p.nc);
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
        const uint32_t vv = base + k * kBlock;
        if (vv >= p.nvec) continue;
        const float4 x = add4(a[k], ba[k]);
        if (!RESID) { a4[vv] = act4<RELU>(x); continue; }
        a4[vv] = x;
        float4 y = b[k];
        if (BIAS_B) { y = add4(y, bb[k]); b4[vv] = y; }
        o4[vv] = act4<RELU>(add4(x, y));
    }
    if (!PLANE && blockIdx.x == 0 && (int)threadIdx.x < p.ntail)
        epilogue_elem<RESID, BIAS_B, RELU>(p, p.tail + threadIdx.x, p.epc);
}

// unaligned pointers: element-wise, grid-strided over [0, n = p.ntail)
template <bool RESID, bool BIAS_B, bool RELU>
__global__ __launch_bounds__(kBlock) void epilogue_scalar_kernel(EpArgs p) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < (uint32_t)p.ntail; i += stride)
        epilogue_elem<RESID, BIAS_B, RELU>(p, i, p.epc);
}

template <bool RESID, bool BIAS_B, bool RELU>
void launch_epilogue(EpArgs p, int64_t n, int64_t C, int64_t epc, bool aligned, hipStream_t st) {
    p.nc = make_fastdiv((uint32_t)C);
    if (!aligned || n < 4) {
        p.nvec = 0; p.tail = 0; p.ntail = (int)n;
        p.epc = make_fastdiv((uint32_t)epc);
        hipLaunchKernelGGL((epilogue_scalar_kernel<RESID, BIAS_B, RELU>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, p);
        return;
    }
    p.nvec = (uint32_t)(n >> 2);
    p.tail = p.nvec * 4u;
    p.ntail = (int)(n & 3);
    const bool plane = (epc % 4 == 0);
    p.epc = make_fastdiv((uint32_t)(plane ? epc / 4 : epc));
#define PPQ_LAUNCH_EP(U, PLANE)                                                                                          \
    hipLaunchKernelGGL((epilogue_kernel<U, RESID, BIAS_B, RELU, PLANE>), dim3((p.nvec + kBlock * U - 1) / (kBlock * U)),   \
                       dim3(kBlock), 0, st, p)
    if (n <= kEpSmallElems) {
        if (plane) PPQ_LAUNCH_EP(kEpSmallU, true); else PPQ_LAUNCH_EP(kEpSmallU, false);
    } else {
        if (plane) PPQ_LAUNCH_EP(kEpTileU, true); else PPQ_LAUNCH_EP(kEpTileU, false);
    }
#undef PPQ_LAUNCH_EP
}

int validate(int64_t n, int64_t C, int64_t epc, const char* what) {
    if (n <= 0 || n > 0x7fffffffLL) {
        set_error("%s: n=%lld is empty or has more than 2^31 - 1 elements", what, (long long)n);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    if (C <= 0 || epc <= 0 || C > 0x7fffffffLL || epc > 0x7fffffffLL || n % (C * epc) != 0) {
        set_error("%s: n=%lld is not [outer, %lld channels, %lld elem/channel]", what, (long long)n, (long long)C,
                  (long long)epc);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_bias_act(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                    void* stream) {
    if (int st = validate(n, num_channel, elem_per_channel, "bias_act")) return st;
    if (!y || !bias) { set_error("bias_act: null pointer"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    EpArgs p{};
    p.a = y; p.bias_a = bias;
    const bool aligned = aligned16(y);
    if (relu) launch_epilogue<false, false, true>(p, n, num_channel, elem_per_channel, aligned, s);
    else launch_epilogue<false, false, false>(p, n, num_channel, elem_per_channel, aligned, s);
    return finish_launch("bias_act");
}

int ppqhip_bias_add_act(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                        int64_t num_channel, int64_t elem_per_channel, int relu, void* stream) {
    if (int st = validate(n, num_channel, elem_per_channel, "bias_add_act")) return st;
    if (!a || !bias_a || !b || !out) { set_error("bias_add_act: null pointer"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    EpArgs p{};
    p.a = a; p.bias_a = bias_a; p.b = b; p.bias_b = bias_b; p.out = out;
    const bool aligned = aligned16(a) && aligned16(b) && aligned16(out);
    if (bias_b) {
        if (relu) launch_epilogue<true, true, true>(p, n, num_channel, elem_per_channel, aligned, s);
        else launch_epilogue<true, true, false>(p, n, num_channel, elem_per_channel, aligned, s);
    } else {
        if (relu) launch_epilogue<true, false, true>(p, n, num_channel, elem_per_channel, aligned, s);
        else launch_epilogue<true, false, false>(p, n, num_channel, elem_per_channel, aligned, s);
    }
    return finish_launch("bias_add_act");
}

}  // extern "C"
