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
//
// Statistics variant (ppqhip_bias_act_stats / ppqhip_bias_add_act_stats): during calibration every tensor these launches store
// is observed, and the observers' end-of-forward launch would read it back from HBM although the epilogue held every value
// in registers a moment earlier.  epilogue_stats_kernel runs the same per-float4 code (epilogue_vec / epilogue_elem: same
// operand order, so the stored tensors are bit for bit the plain kernels') and hands what it stores to one SINK per
// tensor -- the observer's own accumulator of the running range, float[minmax_slots][2], folded with the functions of
// minmax_fold.hpp that reduce.hip's kernels use.  Its shape is that of the slot-owning statistics kernels instead of one
// workgroup per tile: min(tiles, 2 per CU) workgroups of kEpStatBlock lanes, each walking a contiguous tile range with two
// ping-pong register tiles and folding ONCE, at its end, into slot blockIdx.x -- a plain read-modify-write with one owner
// per launch, stream ordered across launches.  No atomics on global memory, nothing synchronises: capturable into a HIP
// graph like the plain launches.  (Histogram sinks for phase 2 of KL / MSE were measured and left out: DESIGN.md section 6.)
#include "channel_axis.hpp"
#include "common.hpp"
#include "minmax_fold.hpp"

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

// What one position stores (for the statistics variant): a (bias_act: y), b (BIAS_B only), out (RESID only).
template <typename T>
struct EpStored { T a, b, out; };

// one element i (channel from the per-element geometry `epc`)
template <bool RESID, bool BIAS_B, bool RELU>
__device__ __forceinline__ EpStored<float> epilogue_elem(const EpArgs& p, uint32_t i, const FastDiv& epc) {
    EpStored<float> s{};
    const uint32_t c = channel_of(i, epc, p.nc);
    const float x = p.a[i] + p.bias_a[c];
    if (!RESID) { p.a[i] = s.a = act(x, RELU); return s; }
    p.a[i] = s.a = x;
    float y = p.b[i];
    if (BIAS_B) { y = y + p.bias_b[c]; p.b[i] = s.b = y; }
    p.out[i] = s.out = act(x + y, RELU);
    return s;
}

// float4 number vv from its loaded operands (a, b) and biases (ba, bb)
template <bool RESID, bool BIAS_B, bool RELU>
__device__ __forceinline__ EpStored<float4> epilogue_vec(float4* a4, float4* b4, float4* o4, uint32_t vv, const float4& a,
                                                         const float4& ba, const float4& b, const float4& bb) {
    EpStored<float4> s{};
    const float4 x = add4(a, ba);
    if (!RESID) { a4[vv] = s.a = act4<RELU>(x); return s; }
    a4[vv] = s.a = x;
    float4 y = b;
    if (BIAS_B) { y = add4(y, bb); b4[vv] = s.b = y; }
    o4[vv] = s.out = act4<RELU>(add4(x, y));
    return s;
}

// RESID = false: a = act(a + bias_a[c]).  RESID = true: a += bias_a[c]; (BIAS_B) b += bias_b[c]; out = act(a + b).
// PLANE: elem_per_channel % 4 == 0 and p.epc holds elem_per_channel / 4.  The tail (n % 4 != 0) implies !PLANE.
template <int U, bool RESID, bool BIAS_B, bool RELU, bool PLANE>
__global__ __launch_bounds__(kBlock) void epilogue_kernel(EpArgs p) {
    const uint32_t base = blockIdx.x * (kBlock * U) + threadIdx.x;
    float4* a4 = reinterpret_cast<float4*>(p.a);
    float4* b4 = reinterpret_cast<float4*>(p.b);
    float4* o4 = reinterpret_cast<float4*>(p.out);
    float4 a[U], ba[U], b[U]{}, bb[U]{};
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
        epilogue_vec<RESID, BIAS_B, RELU>(a4, b4, o4, vv, a[k], ba[k], b[k], bb[k]);
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

// the geometry of the vector kernels (16-B aligned pointers, n >= 4); returns PLANE
bool fill_vector_geometry(EpArgs& p, int64_t n, int64_t C, int64_t epc) {
    const ChannelAxisMap g = pack_channel_axis(true, n, C, epc);
    p.nc = g.nc; p.epc = g.epc;
    p.nvec = g.nvec;
    p.tail = g.nvec * 4u;
    p.ntail = (int)(n & 3);
    return g.plane != 0;
}

template <bool RESID, bool BIAS_B, bool RELU>
void launch_epilogue(EpArgs p, int64_t n, int64_t C, int64_t epc, bool aligned, hipStream_t st) {
    if (!aligned || n < 4) {
        p.nvec = 0; p.tail = 0; p.ntail = (int)n;
        p.epc = make_fastdiv((uint32_t)epc); p.nc = make_fastdiv((uint32_t)C);
        hipLaunchKernelGGL((epilogue_scalar_kernel<RESID, BIAS_B, RELU>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, p);
        return;
    }
    const bool plane = fill_vector_geometry(p, n, C, epc);
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

// ---- the statistics variant ------------------------------------------------------------------------------------------
// One min/max sink per stored tensor: index 0 = a (bias_act: y), 1 = b (BIAS_B only), 2 = out (RESID only);
// nullptr: absent.  slots[k] is the observer's float[minmax_slots][2].
struct EpSinks { float* slots[3]; };
constexpr int kEpStatBlock = 512;              // lanes per workgroup
constexpr int kEpStatWgPerCu = 2;              // co-resident workgroups per CU: the grid cap (2 * CUs <= minmax slots)

// Same arithmetic as epilogue_kernel / its scalar tail; tiles of kEpStatBlock * U float4.  The host guarantees
// gridDim.x <= tiles (every workgroup owns at least one tile), 16-B aligned pointers and nvec >= 1.
template <int U, bool RESID, bool BIAS_B, bool RELU, bool PLANE>
__global__ __launch_bounds__(kEpStatBlock, (kEpStatBlock * kEpStatWgPerCu + 255) / 256)
void epilogue_stats_kernel(EpArgs p, EpSinks sk) {
    __shared__ float lds[32];
    constexpr int NS = RESID ? 3 : 1;
    constexpr uint32_t kTile = (uint32_t)kEpStatBlock * U;
    const uint32_t G = gridDim.x, g = blockIdx.x;
    const uint32_t full = p.nvec / kTile, tiles = full + (p.nvec > full * kTile ? 1u : 0u);
    uint32_t t, t_end;
    even_split(tiles, G, g, t, t_end);
    float4* a4 = reinterpret_cast<float4*>(p.a);
    float4* b4 = reinterpret_cast<float4*>(p.b);
    float4* o4 = reinterpret_cast<float4*>(p.out);

    // sink k is live when the kernel stores its tensor and the caller gave it a destination (workgroup uniform)
    bool live[NS];
    float mn[NS], mx[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        live[k] = sk.slots[k] != nullptr && (k != 1 || BIAS_B);
        mn[k] = INFINITY; mx[k] = -INFINITY;
    }
    auto feed4 = [&](const EpStored<float4>& s) {
        if (live[0]) minmax_fold4(mn[0], mx[0], s.a);
        if (RESID) {
            if (BIAS_B && live[1]) minmax_fold4(mn[1], mx[1], s.b);
            if (live[NS - 1]) minmax_fold4(mn[NS - 1], mx[NS - 1], s.out);
        }
    };
    auto feed1 = [&](const EpStored<float>& s) {
        if (live[0]) minmax_fold1(mn[0], mx[0], s.a);
        if (RESID) {
            if (BIAS_B && live[1]) minmax_fold1(mn[1], mx[1], s.b);
            if (live[NS - 1]) minmax_fold1(mn[NS - 1], mx[NS - 1], s.out);
        }
    };

    struct Tile { float4 a[U], ba[U], b[U], bb[U]; };
    auto fetch = [&](Tile& T, uint32_t tile) {                         // a full tile: no bounds logic
        const uint32_t base = tile * kTile + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t vv = base + u * kEpStatBlock;
            T.a[u] = a4[vv];
            T.ba[u] = bias4<PLANE>(p.bias_a, vv, p.epc, p.nc);
            if (RESID) T.b[u] = b4[vv];
            if (BIAS_B) T.bb[u] = bias4<PLANE>(p.bias_b, vv, p.epc, p.nc);
        }
    };
    auto consume = [&](const Tile& T, uint32_t tile) {
        const uint32_t base = tile * kTile + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; u++)
            feed4(epilogue_vec<RESID, BIAS_B, RELU>(a4, b4, o4, base + u * kEpStatBlock, T.a[u], T.ba[u], T.b[u], T.bb[u]));
    };
    const uint32_t tf = min(t_end, full);                              // full tiles [t, tf)
    if (t < tf) {
        // ping-pong between two register tiles; the prefetch index is clamped (the last tile of the range is loaded twice,
        // before anything is stored to it), so the loads stay unconditional straight-line code
        Tile ta{}, tb{};
        fetch(ta, t);
        for (;;) {
            fetch(tb, min(t + 1, tf - 1));
            consume(ta, t);
            if (++t >= tf) break;
            fetch(ta, min(t + 1, tf - 1));
            consume(tb, t);
            if (++t >= tf) break;
        }
    }
    if (t < t_end) {                                                    // the ragged last tile: clamped loads, predicated stores
        const uint32_t base = t * kTile + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t vv = base + u * kEpStatBlock;
            const uint32_t vc = min(vv, p.nvec - 1);
            const float4 a = a4[vc], ba = bias4<PLANE>(p.bias_a, vc, p.epc, p.nc);
            float4 b{}, bb{};
            if (RESID) b = b4[vc];
            if (BIAS_B) bb = bias4<PLANE>(p.bias_b, vc, p.epc, p.nc);
            if (vv < p.nvec) feed4(epilogue_vec<RESID, BIAS_B, RELU>(a4, b4, o4, vv, a, ba, b, bb));
        }
    }
    if (!PLANE && g == G - 1 && (int)threadIdx.x < p.ntail)             // n % 4 trailing elements: the owner of the last tile
        feed1(epilogue_elem<RESID, BIAS_B, RELU>(p, p.tail + threadIdx.x, p.epc));
#pragma unroll
    for (int k = 0; k < NS; k++) {
        if (!live[k]) continue;
        minmax_block_fold(mn[k], mx[k], lds);
        if (threadIdx.x == 0) minmax_slot_fold(sk.slots[k] + 2 * g, mn[k], mx[k]);
        __syncthreads();                                                // lds is reused by the next sink
    }
}

// The statistics launch, or the reason there is none: PPQHIP_NOT_FUSED (nothing was launched, nothing is wrong: the caller
// runs the plain epilogue and leaves the statistic to the observers' own launch) for what the kernel has no path for.
template <bool RESID, bool BIAS_B>
int launch_epilogue_stats(EpArgs p, int64_t n, int64_t C, int64_t epc, int relu, bool aligned, EpSinks sk, const char* what,
                          hipStream_t st) {
    if ((!sk.slots[0] && !sk.slots[1] && !sk.slots[2]) || !aligned || n < 4) return PPQHIP_NOT_FUSED;
    const bool plane = fill_vector_geometry(p, n, C, epc);
    const bool small = n <= kEpSmallElems;                               // the plain launch's rule
    const uint32_t tile = (uint32_t)kEpStatBlock * (small ? kEpSmallU : kEpTileU), tiles = (p.nvec + tile - 1) / tile;
    const uint32_t cap = (uint32_t)(num_cu() * kEpStatWgPerCu);          // one slot per workgroup
    const uint32_t grid = tiles < cap ? tiles : cap;
#define PPQ_LAUNCH_EPS(U, RELU, PLANE)                                                                                    \
    hipLaunchKernelGGL((epilogue_stats_kernel<U, RESID, BIAS_B, RELU, PLANE>), dim3(grid), dim3(kEpStatBlock), 0, st, p, sk)
    switch ((small ? 0 : 4) | (relu ? 2 : 0) | (plane ? 1 : 0)) {
        case 0: PPQ_LAUNCH_EPS(kEpSmallU, false, false); break;
        case 1: PPQ_LAUNCH_EPS(kEpSmallU, false, true); break;
        case 2: PPQ_LAUNCH_EPS(kEpSmallU, true, false); break;
        case 3: PPQ_LAUNCH_EPS(kEpSmallU, true, true); break;
        case 4: PPQ_LAUNCH_EPS(kEpTileU, false, false); break;
        case 5: PPQ_LAUNCH_EPS(kEpTileU, false, true); break;
        case 6: PPQ_LAUNCH_EPS(kEpTileU, true, false); break;
        default: PPQ_LAUNCH_EPS(kEpTileU, true, true); break;
    }
#undef PPQ_LAUNCH_EPS
    return finish_launch(what);
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_bias_act(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                    void* stream) {
    if (int st = validate_channel_axis("bias_act", n, num_channel, elem_per_channel)) return st;
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
    if (int st = validate_channel_axis("bias_add_act", n, num_channel, elem_per_channel)) return st;
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

int ppqhip_bias_act_stats(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                          float* slots_y, void* stream) {
    if (int st = validate_channel_axis("bias_act_stats", n, num_channel, elem_per_channel)) return st;
    if (!y || !bias) { set_error("bias_act_stats: null pointer"); return PPQHIP_ERR_INVALID_VALUE; }
    EpArgs p{};
    p.a = y; p.bias_a = bias;
    return launch_epilogue_stats<false, false>(p, n, num_channel, elem_per_channel, relu, aligned16(y), EpSinks{{slots_y, nullptr, nullptr}},
                                               "bias_act_stats", (hipStream_t)stream);
}

int ppqhip_bias_add_act_stats(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                              int64_t num_channel, int64_t elem_per_channel, int relu, float* slots_a, float* slots_b,
                              float* slots_out, void* stream) {
    if (int st = validate_channel_axis("bias_add_act_stats", n, num_channel, elem_per_channel)) return st;
    if (!a || !bias_a || !b || !out) { set_error("bias_add_act_stats: null pointer"); return PPQHIP_ERR_INVALID_VALUE; }
    if (!bias_b && slots_b) { set_error("bias_add_act_stats: without bias_b, b is only read: it has no sink"); return PPQHIP_ERR_INVALID_VALUE; }
    EpArgs p{};
    p.a = a; p.bias_a = bias_a; p.b = b; p.bias_b = bias_b; p.out = out;
    const bool aligned = aligned16(a) && aligned16(b) && aligned16(out);
    const EpSinks sk{{slots_a, slots_b, slots_out}};
    hipStream_t s = (hipStream_t)stream;
    if (bias_b) return launch_epilogue_stats<true, true>(p, n, num_channel, elem_per_channel, relu, aligned, sk, "bias_add_act_stats", s);
    return launch_epilogue_stats<true, false>(p, n, num_channel, elem_per_channel, relu, aligned, sk, "bias_add_act_stats", s);
}

}  // extern "C"
