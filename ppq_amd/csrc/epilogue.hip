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
// Statistics variants (ppqhip_bias_act_stats / ppqhip_bias_add_act_stats[2], ppqhip_bias_act_hist / ppqhip_bias_add_act_hist):
// during calibration every tensor these launches store is observed, and the observers' end-of-forward launch would read it
// back from HBM although the epilogue held every value in registers a moment earlier.  epilogue_stats_kernel runs the same
// per-float4 code (epilogue_vec / epilogue_elem: same operand order, so the stored tensors are bit for bit the plain
// kernels') and hands what it computed to one SINK per tensor -- the observer's own accumulator: the running range
// float[minmax_slots][2] in the min/max phase (EpMinMaxSet: the fold of minmax_fold.hpp that reduce.hip's kernels use), the
// histogram rows int32[hist_rows][bins] in the histogram phase of KL / MSE (EpHistSet: hist.hip's Binner from hist_bin.hpp
// over counters in LDS).  Its shape is that of the slot-owning statistics kernels instead of one workgroup per tile: at most
// 2 workgroups per CU of kEpStatBlock lanes, each walking a contiguous tile range with two ping-pong register tiles and
// folding ONCE, at its end, into slot / row blockIdx.x -- a plain read-modify-write with one owner per launch, stream
// ordered across launches.  No atomics on global memory, nothing synchronises: capturable into a HIP graph like the plain
// launches.  A tile is stored BEFORE it is handed to the sinks, with the next tile's loads in flight.
// Store elision (EpArgs::elide): `a` / `b` of a residual launch have two readers in a calibration forward, the addition
// inside the launch and their observer; with a sink the observer is served inside the launch too, and the store -- 0.9 GB
// of the 4.1 GB per ResNet-50 forward -- has no reader left.  The value is computed and fed all the same.
// Measurements, and what the histogram sinks achieve of the streaming rate: DESIGN.md section 6, profiles/r15_epilogue_hist.txt.
// The pooled form (ppqhip_bias_act_pool / _pool_stats / _pool_hist): Conv(bias) -> Relu -> MaxPool, the stem of ResNet-50, as
// one launch.  The Relu tensor there is the largest activation of the network (103 MB at batch 32) and the MaxPool read it
// back from HBM in a launch of its own.  epilogue_pool_kernel has the statistics kernels' shape and sinks (EpMinMaxSet /
// EpHistSet as they are, or none) but walks (n, c) planes: it stages each activated plane in LDS, feeds the sink from
// registers, pools from LDS by at::native::max_pool_forward_nchw's own rule and stores the pooled plane.  With a sink the
// Relu store can be left out too (store_relu = 0): its readers, the observer and the pool, are both inside the launch.
// Contiguous NCHW, H * W % 4 == 0, a plane that fits the LDS, kernel <= 3, dilation 1, floor mode; PPQHIP_NOT_FUSED otherwise.
// Measurements: DESIGN.md section 6, profiles/r17_stem_pool.txt.
// Host side: the eleven entry points at the end of this file keep their C signatures, and each only fills one call record
// (EpCall: form, operands, geometry, relu, elide, the kind of sink with its destinations, the pool window) for run_epilogue.
// That one function holds every check, in the order that decides which message wins, every PPQHIP_NOT_FUSED decision, the
// filling of EpArgs / EpPoolArgs / the sinks and the choice of the launch.  A new sink adds fields to the record and a branch
// in run_epilogue, not a new family of entry points.
#include "channel_axis.hpp"
#include "common.hpp"
#include "epilogue_sinks.hpp"

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
    uint32_t elide;        // statistics variants: kElideA | kElideB, the stores left out (0: every tensor is stored)
};

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

// EpArgs::elide / the `elide` of the two functions below: the stores of a calibration forward that nothing reads (the
// statistics variants with a sink for that tensor; 0 everywhere else).  The VALUE is computed and returned all the same.
constexpr uint32_t kElideA = 1u, kElideB = 2u;

// one element i (channel from the per-element geometry `epc`)
template <bool RESID, bool BIAS_B, bool RELU>
__device__ __forceinline__ EpStored<float> epilogue_elem(const EpArgs& p, uint32_t i, const FastDiv& epc, uint32_t elide = 0) {
    EpStored<float> s{};
    const uint32_t c = channel_of(i, epc, p.nc);
    const float x = p.a[i] + p.bias_a[c];
    if (!RESID) { p.a[i] = s.a = act(x, RELU); return s; }
    s.a = x;
    if (!(elide & kElideA)) p.a[i] = x;
    float y = p.b[i];
    if (BIAS_B) {
        y = y + p.bias_b[c];
        s.b = y;
        if (!(elide & kElideB)) p.b[i] = y;
    }
    p.out[i] = s.out = act(x + y, RELU);
    return s;
}

// float4 number vv from its loaded operands (a, b) and biases (ba, bb)
template <bool RESID, bool BIAS_B, bool RELU>
__device__ __forceinline__ EpStored<float4> epilogue_vec(float4* a4, float4* b4, float4* o4, uint32_t vv, const float4& a,
                                                         const float4& ba, const float4& b, const float4& bb,
                                                         uint32_t elide = 0) {
    EpStored<float4> s{};
    const float4 x = add4(a, ba);
    if (!RESID) { a4[vv] = s.a = act4<RELU>(x); return s; }
    s.a = x;
    if (!(elide & kElideA)) a4[vv] = x;
    float4 y = b;
    if (BIAS_B) {
        y = add4(y, bb);
        s.b = y;
        if (!(elide & kElideB)) b4[vv] = y;
    }
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

// The call record: everything any of the entry points at the end of this file can say, for run_epilogue (zero: not given).
enum EpForm { kEpSingle, kEpResidual, kEpPooled };      // bias_act, bias_add_act, bias_act_pool (and their _stats / _hist)
enum EpSinkKind { kEpNoSink, kEpMinMaxSink, kEpHistSink };
struct EpCall {
    const char* what;                  // the entry point's name, in front of its messages
    EpForm form;
    float* a;                          // kEpSingle, kEpPooled: y
    const float* bias_a;
    float* b;                          // b, bias_b, out: kEpResidual only
    const float* bias_b;
    float* out;
    int64_t n, num_channel, elem_per_channel;
    int relu, elide;
    EpSinkKind sink;
    void* dst[3];                      // per stored tensor (a, b, out): float slots (min/max) or int32_t rows (histogram)
    float p0[3], p1[3];                // histogram: the bin rule's parameters of each sink ...
    int64_t num_bins;                  // ... and what the sinks of one launch share
    int asymmetric, clip_outliers;
    float* pool;                       // kEpPooled only, from here on: height * width stands for elem_per_channel (not read)
    int64_t height, width;
    int kernel, stride, pad, dilation, ceil_mode, store_relu;

    bool aligned() const { return aligned16(a) && (form != kEpResidual || (aligned16(b) && aligned16(out))); }
};

template <bool RESID, bool BIAS_B, bool RELU>
void launch_epilogue(EpArgs p, const EpCall& c, hipStream_t st) {
    const int64_t n = c.n, C = c.num_channel, epc = c.elem_per_channel;
    if (!c.aligned() || n < 4) {
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
// The sinks (EpMinMaxSet / EpHistSet, one per stored tensor), the workgroup shape kEpStatBlock x kEpStatWgPerCu and the LDS
// budget kEpHistLdsInts of the histogram counters: epilogue_sinks.hpp, shared with pointwise_conv.hip's fused launch.

// Same arithmetic as epilogue_kernel / its scalar tail; tiles of kEpStatBlock * U float4.  The host guarantees
// gridDim.x <= tiles (every workgroup owns at least one tile), 16-B aligned pointers and nvec >= 1.  A tile's stores are
// issued before it is handed to the sinks, with the next tile's loads already in flight: the memory pipe has work while
// the sinks' VALU / LDS work drains.  `lds`: 32 floats (min/max sinks) or the histogram counters.
template <int U, bool RESID, bool BIAS_B, bool RELU, bool PLANE, class SINKS>
__global__ __launch_bounds__(kEpStatBlock, (kEpStatBlock * kEpStatWgPerCu + 255) / 256)
void epilogue_stats_kernel(EpArgs p, typename SINKS::Args sk) {
    extern __shared__ int lds[];
    constexpr uint32_t kTile = (uint32_t)kEpStatBlock * U;
    const uint32_t G = gridDim.x, g = blockIdx.x;
    const uint32_t full = p.nvec / kTile, tiles = full + (p.nvec > full * kTile ? 1u : 0u);
    uint32_t t, t_end;
    even_split(tiles, G, g, t, t_end);
    float4* a4 = reinterpret_cast<float4*>(p.a);
    float4* b4 = reinterpret_cast<float4*>(p.b);
    float4* o4 = reinterpret_cast<float4*>(p.out);
    const uint32_t elide = p.elide;
    SINKS sinks;
    sinks.init(sk, lds);

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
        EpStored<float4> s[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            s[u] = epilogue_vec<RESID, BIAS_B, RELU>(a4, b4, o4, base + u * kEpStatBlock, T.a[u], T.ba[u], T.b[u], T.bb[u], elide);
#pragma unroll
        for (int u = 0; u < U; u++) sinks.template feed4<true>(s[u], true, u == 0);
    };
    const uint32_t tf = min(t_end, full);                              // full tiles [t, tf)
    // ping-pong between two register tiles; the prefetch index is clamped (the last tile of the range is loaded twice,
    // before anything is stored to it), so the loads stay unconditional straight-line code
    Tile ta{}, tb{};
    if (t < tf) fetch(ta, t);
    sinks.begin();
    if (t < tf) {
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
            const bool in = vv < p.nvec;
            EpStored<float4> s{};
            if (in) s = epilogue_vec<RESID, BIAS_B, RELU>(a4, b4, o4, vv, a, ba, b, bb, elide);
            sinks.template feed4<false>(s, in, true);
        }
    }
    if (!PLANE && g == G - 1 && p.ntail > 0) {                          // n % 4 trailing elements: the owner of the last tile
        const bool in = (int)threadIdx.x < p.ntail;
        EpStored<float> s{};
        if (in) s = epilogue_elem<RESID, BIAS_B, RELU>(p, p.tail + threadIdx.x, p.epc, elide);
        sinks.feed1(s, in);
    }
    sinks.finish(sk, g, lds);
}

// No epilogue launch, plain or with sinks, is booked under a profiling id (LaunchScope, ppqhip_prof_*): bench.py's roofline leg
// takes the booked kernel with the most device time as THE kernel of the calibration pass -- the end-of-forward statistics
// launch -- and an epilogue id would take that place (tests/test_gpu_calibration.py pins the three names it may be).  The
// launches are timed from kernel traces instead (profiles/r15_epilogue_hist.txt).
// The statistics launch (run_epilogue has seen to it that the kernel has a path: a sink, aligned pointers, n >= 4).
template <bool RESID, bool BIAS_B>
int launch_epilogue_stats(EpArgs p, const EpCall& c, EpMinMaxSinks sk, hipStream_t st) {
    const bool plane = fill_vector_geometry(p, c.n, c.num_channel, c.elem_per_channel);
    const bool small = c.n <= kEpSmallElems;                             // the plain launch's rule
    const uint32_t tile = (uint32_t)kEpStatBlock * (small ? kEpSmallU : kEpTileU), tiles = (p.nvec + tile - 1) / tile;
    const uint32_t cap = (uint32_t)(num_cu() * kEpStatWgPerCu);          // one slot per workgroup
    const uint32_t grid = tiles < cap ? tiles : cap;
    using Set = EpMinMaxSet<RESID, BIAS_B>;
#define PPQ_LAUNCH_EPS(U, RELU, PLANE)                                                                                    \
    hipLaunchKernelGGL((epilogue_stats_kernel<U, RESID, BIAS_B, RELU, PLANE, Set>), dim3(grid), dim3(kEpStatBlock),         \
                       32 * sizeof(float), st, p, sk)
    switch ((small ? 0 : 4) | (c.relu ? 2 : 0) | (plane ? 1 : 0)) {
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
    return finish_launch(c.what);
}

// The histogram sinks' launch.  Instantiated: the two-float4 tile with ReLU only (3 operand forms x PLANE x ASYM x CLIP =
// 24 kernels) -- every group the planner forms ends in a ReLU, and a tensor of kEpSmallElems or less (4 MB: a latency
// chain of a few us) would pay as much for zeroing and flushing its counters as for its tile, so it is NOT fused and
// stays in the observers' end-of-forward launch, which bins all such tensors of a forward behind one flush.
constexpr uint32_t kEpHistMinTiles = 2;            // tiles (32 KB per operand) a workgroup has at least behind one row flush.
                                                   // Headline ms / step, MI355X, interleaved x 3 (profiles/r15_epilogue_hist.txt):
                                                   // 1 tile 8.765, 2 tiles 8.780, 4 tiles 8.783; binning a float4 before storing
                                                   // it instead of after 8.753 -- all inside the 0.2-0.8 % run-to-run spread;
                                                   // reading the row at the start of the launch instead of at its end: 8.750 -> 8.665.
                                                   // NOT swept: the workgroup shape and the co-resident count.  kEpStatBlock x
                                                   // kEpStatWgPerCu = 512 lanes x 2 per CU is inherited from the min/max sinks,
                                                   // because the observers' rows / slots accumulators have one row per workgroup
                                                   // of exactly that grid (hist_rows = 2 per CU); the histogram sinks reach
                                                   // 0.62 of 8 TB/s with it, and another shape may do better

// The histogram sinks of a call (1 <= num_bins < 2^31), pooled or not: (p0, p1) of a sink as the observers' own launches take
// them, sym -> (0, hist_scale), asym -> (min, (max - min) / bins), and the counters' places in LDS.  lds_ints == 0: the call
// has no sink, or its counters do not fit kEpHistLdsInts -- there is no launch for it.
EpHistSinks hist_sinks(const EpCall& c) {
    EpHistSinks sk{};
    sk.bins = (int)c.num_bins;
    uint64_t ints = 0;
    for (int k = 0; k < 3; k++) {
        sk.rows[k] = static_cast<int*>(c.dst[k]);
        if (c.asymmetric) { sk.a0[k] = c.p0[k]; sk.hs[k] = (c.p1[k] - c.p0[k]) / (float)sk.bins; }       // sort.cu:123
        else { sk.a0[k] = 0.f; sk.hs[k] = c.p0[k]; }
        sk.lds_off[k] = (uint32_t)ints;
        if (sk.rows[k]) ints += (uint64_t)c.num_bins;
    }
    sk.lds_ints = ints > kEpHistLdsInts ? 0u : (uint32_t)ints;
    return sk;
}

// (run_epilogue has seen to it that the kernel has a path: counters that fit, aligned pointers, n > kEpSmallElems, ReLU)
template <bool RESID, bool BIAS_B>
int launch_epilogue_hist(EpArgs p, const EpCall& c, EpHistSinks sk, hipStream_t st) {
    const uint32_t ints = sk.lds_ints;
    const bool plane = fill_vector_geometry(p, c.n, c.num_channel, c.elem_per_channel);
    const uint32_t tile = (uint32_t)kEpStatBlock * kEpTileU, tiles = (p.nvec + tile - 1) / tile;
    const uint32_t cap = (uint32_t)(num_cu() * kEpStatWgPerCu);          // one row per workgroup
    uint32_t grid = tiles / kEpHistMinTiles;                             // (n > kEpSmallElems: at least 128)
    if (grid > cap) grid = cap;
#define PPQ_LAUNCH_EPH(PLANE, ASYM, CLIP)                                                                                 \
    hipLaunchKernelGGL((epilogue_stats_kernel<kEpTileU, RESID, BIAS_B, true, PLANE, EpHistSet<RESID, BIAS_B, ASYM, CLIP>>),  \
                       dim3(grid), dim3(kEpStatBlock), ints * sizeof(int), st, p, sk)
    switch ((plane ? 4 : 0) | (c.asymmetric ? 2 : 0) | (c.clip_outliers ? 1 : 0)) {
        case 0: PPQ_LAUNCH_EPH(false, false, false); break;
        case 1: PPQ_LAUNCH_EPH(false, false, true); break;
        case 2: PPQ_LAUNCH_EPH(false, true, false); break;
        case 3: PPQ_LAUNCH_EPH(false, true, true); break;
        case 4: PPQ_LAUNCH_EPH(true, false, false); break;
        case 5: PPQ_LAUNCH_EPH(true, false, true); break;
        case 6: PPQ_LAUNCH_EPH(true, true, false); break;
        default: PPQ_LAUNCH_EPH(true, true, true); break;
    }
#undef PPQ_LAUNCH_EPH
    return finish_launch(c.what);
}

// The operand forms <RESID, BIAS_B> the three launches are instantiated for, as run_epilogue picks them:
// [0] <0, 0> the single tensor, [1] <1, 1> the residual with bias_b, [2] <1, 0> without; plain launches also by [!relu].
constexpr void (*kEpLaunch[3][2])(EpArgs, const EpCall&, hipStream_t) = {
    {launch_epilogue<false, false, true>, launch_epilogue<false, false, false>},
    {launch_epilogue<true, true, true>, launch_epilogue<true, true, false>},
    {launch_epilogue<true, false, true>, launch_epilogue<true, false, false>}};
constexpr int (*kEpStatsLaunch[3])(EpArgs, const EpCall&, EpMinMaxSinks, hipStream_t) = {
    launch_epilogue_stats<false, false>, launch_epilogue_stats<true, true>, launch_epilogue_stats<true, false>};
constexpr int (*kEpHistLaunch[3])(EpArgs, const EpCall&, EpHistSinks, hipStream_t) = {
    launch_epilogue_hist<false, false>, launch_epilogue_hist<true, true>, launch_epilogue_hist<true, false>};

// ---- the pooled form: Conv(bias) -> Relu -> MaxPool in one launch ------------------------------------------------------
// pool = MaxPool_{k,s,p}(act(y + bias[c])) over contiguous NCHW.  The launch has the statistics kernels' shape (at most
// kEpStatWgPerCu workgroups of kEpStatBlock lanes per CU, one fold into slot / row blockIdx.x at the end), but its unit of
// work is the (n, c) PLANE: a workgroup walks a contiguous range of planes in steps of kEpStatBlock * kEpTileU float4 with
// the same ping-pong register tiles, and every step puts what it computed (a) back into y unless the store is elided, (b) into
// the plane's image in LDS, (c) into the sink, from registers, once.  After a plane's last step the workgroup pools from LDS --
// with the first step of the NEXT plane already in flight -- and stores the pooled plane.
// The pool is at::native::max_pool_forward_nchw's rule, literally: start from -inf, scan the window row by row and left to
// right, skip the padding taps, take val when `val > maxval || isnan(val)` (which of +0.0 / -0.0 wins, and which NaN payload
// comes out, follow from that order).
// LDS: [sink: histogram counters or 32 floats] [plane: H * W floats] [staging: 128 floats per wave].  One lane pools ONE
// output at a time and consecutive lanes take consecutive outputs, so a stride-2 window reads LDS with a two-way bank
// conflict at worst (four consecutive outputs per lane would be an eight-way one); each wave then turns its 128 pooled
// values into 16-B stores through its own staging lines (no workgroup barrier: LDS operations of one wave complete in
// order).  A pooled plane whose size is no multiple of 4 is stored element by element.
struct EpNoSinks {
    struct Args {};
    __device__ __forceinline__ void init(const Args&, int*) {}
    __device__ __forceinline__ void begin() {}
    template <bool FULL>
    __device__ __forceinline__ void feed4(const EpStored<float4>&, bool, bool) {}
    __device__ __forceinline__ void finish(const Args&, uint32_t, int*) {}
};

constexpr uint32_t kEpPoolStage = 2 * kWave;                                   // pooled values a wave stages per trip
constexpr uint32_t kEpPoolStageBytes = (kEpStatBlock / kWave) * kEpPoolStage * sizeof(float);
constexpr uint32_t kEpPoolMaxLds = 64u * 1024u;                                // per workgroup (two per CU: 128 of 160 KB)
constexpr int kEpPoolMaxKernel = 3;

struct EpPoolArgs {
    float* y;
    const float* bias;
    float* pool;
    uint32_t planes;       // N * C
    uint32_t hw4;          // H * W / 4
    uint32_t H, W, ohw;    // ohw: OH * OW
    int k, s, pad;
    FastDiv nc;            // num_channel: channel = plane % C
    FastDiv ow;            // OW: (oh, ow) of a pooled index
    uint32_t store;        // 0: y keeps the convolution output (the elided store)
    uint32_t vec;          // ohw % 4 == 0: 16-B stores of pool
    uint32_t sink_ints;    // LDS ints in front of the plane
};

__device__ __forceinline__ void lds_barrier() {       // LDS traffic only: __syncthreads() would also wait for the loads in flight
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// pooled value o of the plane held in LDS.  Every tap is read from an index clamped into the plane, so that the nine LDS reads
// issue back to back with no branch between them; a tap in the padding, or beyond a window smaller than 3 x 3, then counts as
// -inf, which the rule never takes (`-inf > maxval` is false for every maxval, -inf is no NaN): exactly as if it were skipped.
__device__ __forceinline__ float pool_at(const float* plane, const EpPoolArgs& p, uint32_t o) {
    const uint32_t oh = fdiv(o, p.ow), ow = o - oh * p.ow.d;
    const int h0 = (int)oh * p.s - p.pad, w0 = (int)ow * p.s - p.pad;
    float v[kEpPoolMaxKernel][kEpPoolMaxKernel];
#pragma unroll
    for (int kh = 0; kh < kEpPoolMaxKernel; kh++) {
        const int ih = h0 + kh;
        const bool row = kh < p.k && (uint32_t)ih < p.H;
        const uint32_t first = (uint32_t)min(max(ih, 0), (int)p.H - 1) * p.W;
#pragma unroll
        for (int kw = 0; kw < kEpPoolMaxKernel; kw++) {
            const int iw = w0 + kw;
            const float t = plane[first + (uint32_t)min(max(iw, 0), (int)p.W - 1)];
            v[kh][kw] = (row && kw < p.k && (uint32_t)iw < p.W) ? t : -INFINITY;
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int kh = 0; kh < kEpPoolMaxKernel; kh++)
#pragma unroll
        for (int kw = 0; kw < kEpPoolMaxKernel; kw++)
            if (v[kh][kw] > m || __builtin_isnan(v[kh][kw])) m = v[kh][kw];
    return m;
}

// The host guarantees gridDim.x <= planes, 16-B aligned pointers, hw4 >= 1 and that the LDS layout fits.
template <int U, bool RELU, class SINKS>
__global__ __launch_bounds__(kEpStatBlock, (kEpStatBlock * kEpStatWgPerCu + 255) / 256)
void epilogue_pool_kernel(EpPoolArgs p, typename SINKS::Args sk) {
    extern __shared__ int lds[];
    constexpr uint32_t kTile = (uint32_t)kEpStatBlock * U;
    float* plane = reinterpret_cast<float*>(lds + p.sink_ints);
    float4* plane4 = reinterpret_cast<float4*>(plane);
    float* stage = plane + p.hw4 * 4u + (threadIdx.x >> 6) * kEpPoolStage;     // this wave's staging lines
    float4* y4 = reinterpret_cast<float4*>(p.y);
    uint32_t pl, pl_end;
    even_split(p.planes, gridDim.x, blockIdx.x, pl, pl_end);
    const uint32_t steps = (p.hw4 + kTile - 1) / kTile;                        // per plane
    SINKS sinks;
    sinks.init(sk, lds);

    struct Tile { float4 a[U]; float bias; };
    auto fetch = [&](Tile& T, uint32_t pi, uint32_t step) {                    // clamped inside the plane: straight-line loads
        const uint32_t first = pi * p.hw4, base = step * kTile + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; u++) T.a[u] = y4[first + min(base + u * kEpStatBlock, p.hw4 - 1)];
        T.bias = p.bias[pi - fdiv(pi, p.nc) * p.nc.d];
    };
    auto pool_plane = [&](uint32_t pi) {
        float* dst = p.pool + (size_t)pi * p.ohw;
        const uint32_t lane = threadIdx.x & 63, wave_first = (threadIdx.x >> 6) * kEpPoolStage;
        for (uint32_t base = 0; base < p.ohw; base += (kEpStatBlock / kWave) * kEpPoolStage) {
            const uint32_t o0 = base + wave_first + lane, o1 = o0 + kWave;
            const float m0 = o0 < p.ohw ? pool_at(plane, p, o0) : 0.f;
            const float m1 = o1 < p.ohw ? pool_at(plane, p, o1) : 0.f;
            if (p.vec) {
                stage[lane] = m0;
                stage[kWave + lane] = m1;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t o4 = base + wave_first + 4u * lane;             // (ohw % 4 == 0: a float4 in range is whole)
                if (lane < kEpPoolStage / 4 && o4 < p.ohw)
                    *reinterpret_cast<float4*>(dst + o4) = *reinterpret_cast<const float4*>(stage + 4u * lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            } else {
                if (o0 < p.ohw) dst[o0] = m0;
                if (o1 < p.ohw) dst[o1] = m1;
            }
        }
    };
    auto consume = [&](const Tile& T, uint32_t pi, uint32_t step) {
        const uint32_t first = pi * p.hw4, base = step * kTile + threadIdx.x;
        const float4 bias = make_float4(T.bias, T.bias, T.bias, T.bias);
        const bool full = (step + 1) * kTile <= p.hw4;                         // workgroup uniform
        EpStored<float4> s[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t vv = base + u * kEpStatBlock;
            in[u] = vv < p.hw4;
            s[u] = EpStored<float4>{};
            s[u].a = act4<RELU>(add4(T.a[u], bias));
            if (in[u]) {
                if (p.store) y4[first + vv] = s[u].a;
                plane4[vv] = s[u].a;
            }
        }
        if (full) {
#pragma unroll
            for (int u = 0; u < U; u++) sinks.template feed4<true>(s[u], true, u == 0);
        } else {
#pragma unroll
            for (int u = 0; u < U; u++)                                         // a wave with nothing in range has nothing to feed
                if (__builtin_amdgcn_ballot_w64(in[u]) != 0ull) sinks.template feed4<false>(s[u], in[u], true);
        }
        if (step + 1 == steps) {                                                // the plane is complete
            lds_barrier();
            pool_plane(pi);
            lds_barrier();                                                      // before the next plane overwrites it
        }
    };
    // (plane, step) pairs in order; the prefetch of the pair behind the last one re-reads the last (before anything of it is stored)
    uint32_t cp = pl, cs = 0;
    Tile ta{}, tb{};
    fetch(ta, cp, cs);
    sinks.begin();
    for (;;) {
        uint32_t np = cp, ns = cs + 1;
        if (ns == steps) { ns = 0; np++; }
        bool last = np >= pl_end;
        fetch(tb, last ? cp : np, last ? cs : ns);
        consume(ta, cp, cs);
        if (last) break;
        cp = np; cs = ns;
        ns = cs + 1;
        if (ns == steps) { ns = 0; np++; }
        last = np >= pl_end;
        fetch(ta, last ? cp : np, last ? cs : ns);
        consume(tb, cp, cs);
        if (last) break;
        cp = np; cs = ns;
    }
    sinks.finish(sk, blockIdx.x, lds);
}

// The shape checks of the pooled form: the dynamic LDS size, with `p` filled, or 0 for what the kernel has no exact path for.
// On entry p.sink_ints holds the LDS ints the sinks own in front of the plane.
uint32_t fill_pool_geometry(EpPoolArgs& p, const EpCall& c) {
    const int64_t H = c.height, W = c.width;
    const int kernel = c.kernel, stride = c.stride, pad = c.pad;
    if (kernel < 1 || kernel > kEpPoolMaxKernel || stride < 1 || pad < 0 || 2 * pad > kernel || c.dilation != 1 || c.ceil_mode != 0)
        return 0;                                                                // (PyTorch refuses a pad above kernel / 2 itself)
    const int64_t hw = H * W;
    if (hw % 4 != 0 || H + 2 * pad < kernel || W + 2 * pad < kernel || !aligned16(p.y) || !aligned16(p.pool)) return 0;
    const int64_t OH = (H + 2 * pad - kernel) / stride + 1, OW = (W + 2 * pad - kernel) / stride + 1, planes = c.n / hw;
    if (planes * OH * OW > 0x7fffffffLL) return 0;
    p.sink_ints = (p.sink_ints + 3u) & ~3u;                                      // the plane starts on a 16-B boundary
    const int64_t bytes = (int64_t)p.sink_ints * 4 + hw * 4 + kEpPoolStageBytes;
    if (bytes > (int64_t)kEpPoolMaxLds) return 0;
    p.planes = (uint32_t)planes; p.hw4 = (uint32_t)(hw / 4);
    p.H = (uint32_t)H; p.W = (uint32_t)W; p.ohw = (uint32_t)(OH * OW);
    p.k = kernel; p.s = stride; p.pad = pad;
    p.nc = make_fastdiv((uint32_t)c.num_channel); p.ow = make_fastdiv((uint32_t)OW);
    p.vec = p.ohw % 4u == 0 ? 1u : 0u;
    return (uint32_t)bytes;
}

// The pooled launch with the sinks of c.sink, or PPQHIP_NOT_FUSED for a window or plane without a path: the one such decision
// outside run_epilogue, because it falls out of the LDS layout that only this launch has.
int launch_epilogue_pool(EpPoolArgs p, const EpCall& c, const EpMinMaxSinks& mm, const EpHistSinks& hs, hipStream_t st) {
    const uint32_t lds_bytes = fill_pool_geometry(p, c);
    if (lds_bytes == 0) return PPQHIP_NOT_FUSED;
    const uint32_t cap = (uint32_t)(num_cu() * kEpStatWgPerCu);                  // one slot / row per workgroup
    const uint32_t grid = p.planes < cap ? p.planes : cap;
#define PPQ_LAUNCH_POOL(RELU, SET, SK)                                                                                    \
    hipLaunchKernelGGL((epilogue_pool_kernel<kEpTileU, RELU, SET>), dim3(grid), dim3(kEpStatBlock), lds_bytes, st, p, SK)
#define PPQ_LAUNCH_POOLH(ASYM, CLIP) { using Set = EpHistSet<false, false, ASYM, CLIP>; PPQ_LAUNCH_POOL(true, Set, hs); }
    if (c.sink == kEpNoSink) {
        const EpNoSinks::Args none{};
        if (c.relu) PPQ_LAUNCH_POOL(true, EpNoSinks, none); else PPQ_LAUNCH_POOL(false, EpNoSinks, none);
    } else if (c.sink == kEpMinMaxSink) {
        using Set = EpMinMaxSet<false, false>;
        if (c.relu) PPQ_LAUNCH_POOL(true, Set, mm); else PPQ_LAUNCH_POOL(false, Set, mm);
    } else {
        switch ((c.asymmetric ? 2 : 0) | (c.clip_outliers ? 1 : 0)) {            // (ReLU only, like the unpooled histogram launch)
            case 0: PPQ_LAUNCH_POOLH(false, false); break;
            case 1: PPQ_LAUNCH_POOLH(false, true); break;
            case 2: PPQ_LAUNCH_POOLH(true, false); break;
            default: PPQ_LAUNCH_POOLH(true, true); break;
        }
    }
#undef PPQ_LAUNCH_POOLH
#undef PPQ_LAUNCH_POOL
    return finish_launch(c.what);
}

int refuse(const char* what, const char* why) {
    set_error("%s: %s", what, why);
    return PPQHIP_ERR_INVALID_VALUE;
}

// Every entry point below: validation (the order is the precedence of the messages, pinned by
// tests/test_host_epilogue_refusals.py), then the reasons to launch nothing -- PPQHIP_NOT_FUSED: nothing is wrong, the caller runs
// the plain epilogue and leaves the statistic to the observers' own launch -- then the kernels' structs and the launch.
int run_epilogue(const EpCall& c, hipStream_t st) {
    const bool resid = c.form == kEpResidual, pooled = c.form == kEpPooled;
    const bool minmax = c.sink == kEpMinMaxSink, hist = c.sink == kEpHistSink;
    int64_t epc = c.elem_per_channel;
    if (pooled) {
        // The plane comes before the channel axis, unlike every other check of a shape here: height * width IS the axis'
        // elem_per_channel, and the product must be known not to overflow before the axis is checked with it.
        if (c.height <= 0 || c.width <= 0 || c.height > 0x7fffffffLL || c.width > 0x7fffffffLL || c.height * c.width > 0x7fffffffLL) {
            set_error("%s: the plane %lld x %lld is empty or too large", c.what, (long long)c.height, (long long)c.width);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        epc = c.height * c.width;
    }
    if (int s = validate_channel_axis(c.what, c.n, c.num_channel, epc)) return s;
    if (!c.a || !c.bias_a || (resid && (!c.b || !c.out)) || (pooled && !c.pool)) return refuse(c.what, "null pointer");
    if (!c.bias_b && c.dst[1]) return refuse(c.what, "without bias_b, b is only read: it has no sink");
    if (hist && (c.num_bins <= 0 || c.num_bins > 0x7fffffffLL)) return refuse(c.what, "histogram is empty or too large");
    // An elided tensor must be one the launch computes AND hands to a sink: otherwise its values would be lost.  The pooled
    // form's store_relu == 0 is the elision of its one tensor: its readers, the observer and the pool, are inside the launch.
    const int elide = pooled ? (c.store_relu ? 0 : (int)kElideA) : c.elide;
    if (elide & ~(int)(kElideA | kElideB)) return refuse(c.what, "elide has unknown bits");
    if (((elide & (int)kElideA) && !c.dst[0]) || ((elide & (int)kElideB) && !(c.dst[1] && c.bias_b)))
        return refuse(c.what, "a tensor that is not stored needs a sink");
    // a workgroup reads its row of every sink ahead and writes it back at the end: two sinks on one accumulator would lose counts
    if (hist && ((c.dst[0] && (c.dst[0] == c.dst[1] || c.dst[0] == c.dst[2])) || (c.dst[1] && c.dst[1] == c.dst[2])))
        return refuse(c.what, "two sinks share one rows accumulator");

    EpMinMaxSinks mm{};
    EpHistSinks hs{};
    if (minmax) {
        for (int k = 0; k < 3; k++) mm.slots[k] = static_cast<float*>(c.dst[k]);
        if (!mm.slots[0] && !mm.slots[1] && !mm.slots[2]) return PPQHIP_NOT_FUSED;
    }
    if (hist) {
        hs = hist_sinks(c);
        if (hs.lds_ints == 0 || !c.relu) return PPQHIP_NOT_FUSED;                // (why ReLU only: above launch_epilogue_hist)
    }
    if (pooled) {
        EpPoolArgs p{};
        p.y = c.a; p.bias = c.bias_a; p.pool = c.pool;
        p.store = (elide & (int)kElideA) ? 0u : 1u;
        p.sink_ints = hist ? hs.lds_ints : minmax ? 32u : 0u;                    // (min/max: the 32 floats of its block fold)
        return launch_epilogue_pool(p, c, mm, hs, st);
    }
    if (minmax && (!c.aligned() || c.n < 4)) return PPQHIP_NOT_FUSED;            // the sinks' kernels are vector kernels only
    if (hist && (!c.aligned() || c.n <= kEpSmallElems)) return PPQHIP_NOT_FUSED; // (small tensors: above launch_epilogue_hist)

    EpArgs p{};
    p.a = c.a; p.bias_a = c.bias_a; p.b = c.b; p.bias_b = c.bias_b; p.out = c.out; p.elide = (uint32_t)elide;
    const int form = !resid ? 0 : c.bias_b ? 1 : 2;
    if (minmax) return kEpStatsLaunch[form](p, c, mm, st);
    if (hist) return kEpHistLaunch[form](p, c, hs, st);
    kEpLaunch[form][c.relu ? 0 : 1](p, c, st);
    return finish_launch(c.what);
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

// Each entry point fills the call record -- its leading fields in the order of EpCall, `what` .. `dst` (.. `clip_outliers` with
// histogram sinks) -- and runs it.
extern "C" {

int ppqhip_bias_act(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                    void* stream) {
    const EpCall c{"bias_act", kEpSingle, y, bias, nullptr, nullptr, nullptr, n, num_channel, elem_per_channel, relu};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_add_act(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                        int64_t num_channel, int64_t elem_per_channel, int relu, void* stream) {
    const EpCall c{"bias_add_act", kEpResidual, a, bias_a, b, bias_b, out, n, num_channel, elem_per_channel, relu};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_act_stats(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                          float* slots_y, void* stream) {
    const EpCall c{"bias_act_stats", kEpSingle, y, bias, nullptr, nullptr, nullptr, n, num_channel, elem_per_channel, relu, 0,
                   kEpMinMaxSink, {slots_y}};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_add_act_stats(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                              int64_t num_channel, int64_t elem_per_channel, int relu, float* slots_a, float* slots_b,
                              float* slots_out, void* stream) {
    const EpCall c{"bias_add_act_stats", kEpResidual, a, bias_a, b, bias_b, out, n, num_channel, elem_per_channel, relu, 0,
                   kEpMinMaxSink, {slots_a, slots_b, slots_out}};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_add_act_stats2(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                               int64_t num_channel, int64_t elem_per_channel, int relu, float* slots_a, float* slots_b,
                               float* slots_out, int elide, void* stream) {
    const EpCall c{"bias_add_act_stats2", kEpResidual, a, bias_a, b, bias_b, out, n, num_channel, elem_per_channel, relu, elide,
                   kEpMinMaxSink, {slots_a, slots_b, slots_out}};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_act_hist(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                         int32_t* rows_y, float p0_y, float p1_y, int64_t num_bins, int asymmetric, int clip_outliers,
                         void* stream) {
    const EpCall c{"bias_act_hist", kEpSingle, y, bias, nullptr, nullptr, nullptr, n, num_channel, elem_per_channel, relu, 0,
                   kEpHistSink, {rows_y}, {p0_y}, {p1_y}, num_bins, asymmetric, clip_outliers};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_add_act_hist(float* a, const float* bias_a, float* b, const float* bias_b, float* out, int64_t n,
                             int64_t num_channel, int64_t elem_per_channel, int relu, int32_t* rows_a, float p0_a, float p1_a,
                             int32_t* rows_b, float p0_b, float p1_b, int32_t* rows_out, float p0_out, float p1_out,
                             int64_t num_bins, int asymmetric, int clip_outliers, int elide, void* stream) {
    const EpCall c{"bias_add_act_hist", kEpResidual, a, bias_a, b, bias_b, out, n, num_channel, elem_per_channel, relu, elide,
                   kEpHistSink, {rows_a, rows_b, rows_out}, {p0_a, p0_b, p0_out}, {p1_a, p1_b, p1_out},
                   num_bins, asymmetric, clip_outliers};
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_act_pool(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height, int64_t width,
                         int relu, int kernel, int stride, int pad, int dilation, int ceil_mode, void* stream) {
    EpCall c{"bias_act_pool", kEpPooled, y, bias, nullptr, nullptr, nullptr, n, num_channel, 0, relu};
    c.pool = pool; c.height = height; c.width = width;
    c.kernel = kernel; c.stride = stride; c.pad = pad; c.dilation = dilation; c.ceil_mode = ceil_mode; c.store_relu = 1;
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_act_pool_stats(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height,
                               int64_t width, int relu, int kernel, int stride, int pad, int dilation, int ceil_mode,
                               float* slots_y, int store_relu, void* stream) {
    EpCall c{"bias_act_pool_stats", kEpPooled, y, bias, nullptr, nullptr, nullptr, n, num_channel, 0, relu, 0, kEpMinMaxSink, {slots_y}};
    c.pool = pool; c.height = height; c.width = width;
    c.kernel = kernel; c.stride = stride; c.pad = pad; c.dilation = dilation; c.ceil_mode = ceil_mode; c.store_relu = store_relu;
    return run_epilogue(c, (hipStream_t)stream);
}

int ppqhip_bias_act_pool_hist(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height,
                              int64_t width, int relu, int kernel, int stride, int pad, int dilation, int ceil_mode,
                              int32_t* rows_y, float p0_y, float p1_y, int64_t num_bins, int asymmetric, int clip_outliers,
                              int store_relu, void* stream) {
    EpCall c{"bias_act_pool_hist", kEpPooled, y, bias, nullptr, nullptr, nullptr, n, num_channel, 0, relu, 0,
             kEpHistSink, {rows_y}, {p0_y}, {p1_y}, num_bins, asymmetric, clip_outliers};
    c.pool = pool; c.height = height; c.width = width;
    c.kernel = kernel; c.stride = stride; c.pad = pad; c.dilation = dilation; c.ceil_mode = ceil_mode; c.store_relu = store_relu;
    return run_epilogue(c, (hipStream_t)stream);
}

}  // extern "C"
