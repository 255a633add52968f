// fq_walk.hpp -- THE walks of the element-wise fake-quant kernels: the forward tile walk, the element-wise
// fallback, the backward row walk, the short-row backward and the fixed-order finish sum, plus the host half of their entry points.
// linear.hip (integer grids) and floating.hip (FP8 and other small floats) bring a quantiser policy and their element functors and
// add nothing else: every __global__ function of the two files is a thin wrapper over a template below.
//
// A quantiser policy Q (LinearQ in linear.hip, FloatQ in floating.hip) supplies
//     Q::State                      what one (scale, offset) pair becomes: s, fq_safe_rcp(s), round_offset(o) / s, o, pow2_reciprocal_bits(s)
//     q.make(scale, offset)         builds it
//     q.quant4(float4, state)       fake-quantises four elements of one channel
//     q.quant1(float, state)        one element, the same arithmetic (results do not depend on the launch shape)
//     q.fast(state)                 FQ_GUARD_SLOW only: the state takes the policy's branch-free path
//
// Why the forward walk looks the way it does (MI355X, rocprofv3 medians, interleaved A/B):
//   * one contiguous tile of kBlock * U float4 per workgroup, no loop: tens of thousands of short-lived workgroups over contiguous
//     tiles stream faster than a chip-sized persistent grid-stride loop (6.8 vs 4.9 TB/s on 205 MB in + 205 MB out), and tiny
//     tensors still spread over every CU;
//   * the U loads are clamped to the last float4 instead of predicated, so that they are branch-free and issue back to back, ahead
//     of the scale read where the scale is uniform;
//   * the arithmetic is unconditional (lanes past the end recompute the clamped element) and only the STORE is predicated: with the
//     whole body under `if (v < nvec)` the compiler sinks the tile's x / scale loads into the branch, BEHIND the wait for the
//     scale and the offsets (two dependent memory round trips on a latency-bound tensor).  Not every kernel has this shape yet:
//     see FqPredication;
//   * NT selects streaming loads for tensors that cannot be cache resident anyway; stores stay cacheable because the next
//     operation of the graph consumes the output.
#pragma once

#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {

// ---- host: checks ---------------------------------------------------------------------------------------------------------------
inline int validate_n(int64_t n, const char* what) {
    if (n <= 0) { set_error("%s: tensor is empty", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (n > 0x7fffffffLL) {
        set_error("%s: there are too many elements in your tensor (more than 2*10^9)", what);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

inline int validate_channels(int64_t n, int64_t C, int64_t epc, const char* what) {
    if (C <= 0 || epc <= 0 || n % (C * epc) != 0) {
        set_error("%s: n=%lld is not [outer, %lld channels, %lld elem/channel]", what, (long long)n,
                  (long long)C, (long long)epc);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

// 16-B accesses need aligned pointers and channel rows of whole float4s (a float4 never straddles channels); per tensor: epc = 4
inline bool fq_vec_ok(const float* x, const float* out, int64_t epc = 4) { return aligned16(x) && aligned16(out) && epc % 4 == 0; }
inline bool fq_bwd_vec_ok(const float* x, const float* dy, const float* gx, int64_t epc = 4) {
    return epc % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(gx);
}

// ---- host: tile shapes ----------------------------------------------------------------------------------------------------------
// Tensors of at least kStreamElems elements (192 MiB) cannot be resident in the 256 MiB Infinity
// Cache together with their output: read them with streaming (nontemporal) loads.
constexpr int64_t kStreamElems = 48ll << 20;
// Tile shape: U 16-B accesses per lane and workgroup.  HBM-bound tensors stream best with U = 2 (half as many workgroups to
// dispatch); a tensor of a few MB is ONE latency chain (dispatch -> loads -> arithmetic -> stores) in which the arithmetic of
// the last-arriving wave is exposed, so U = 1 (twice the waves, half the work behind each load) is 0.2 us faster on
// B = [1,512,56,56]: 4.28 -> 4.08 us per tensor, 4.44 -> 4.24 per channel (rocprofv3 medians, interleaved A/B,
// profiles/r05_floor_table.txt); the copy floor of the same 12.8 MB is 3.88 us.
constexpr int kTileU = 2;
constexpr int kSmallU = 1;
constexpr int64_t kFqSmallElems = 4ll << 20;        // up to 16 MB in + 16 MB out

// launch(std::integral_constant<int, U>, std::bool_constant<NT>) for a tensor of n elements
template <typename Launch>
inline void with_tile_shape(int64_t n, Launch launch) {
    if (n >= kStreamElems) launch(std::integral_constant<int, kTileU>(), std::true_type());
    else if (n <= kFqSmallElems) launch(std::integral_constant<int, kSmallU>(), std::false_type());
    else launch(std::integral_constant<int, kTileU>(), std::false_type());
}
inline dim3 tile_grid(uint32_t nvec, int U) { return dim3((nvec + kBlock * U - 1) / (kBlock * U)); }

// ---- many tensors, one launch ---------------------------------------------------------------------------------------------------
// Every forward of a quantised graph fake-quantises all of its weights again (the reference executor does so until
// ParameterBakingPass; ResNet-50 has 54 of them, 0.01 .. 9 MB each; the TRT_FP8 policy does it per channel for the 50 weights of
// ViT-B/16) -- one launch per weight is pure launch latency.  Here one launch serves them all: the job table lives in device
// memory (it only changes when a weight / scale tensor is replaced), the kernel arguments carry the prefix of workgroup counts so
// a workgroup finds its job without touching memory, and each workgroup quantises one tile of kBlock * kFqMultiU float4 (or the
// same range element-wise when the tensor cannot be vectorised: elem_per_channel % 4 != 0 or unaligned).  Per-tensor jobs are C = 1.
constexpr int kFqMultiMax = 128;
constexpr int kFqMultiU = 2;
template <typename Fmt>
struct FqJobOf {
    const float* x;
    float* out;
    const float* scale;
    const float* offset;
    uint32_t n;
    uint32_t vec_ok;
    FastDiv per;          // vec_ok: float4 per channel row; else elements per channel row
    FastDiv nc;
    Fmt fmt;              // what the quantiser policy needs besides (scale, offset)
};
template <typename DevJob>
struct FqMultiArgsOf {
    uint32_t first_block[kFqMultiMax];
    uint32_t count;
    int rounding;
    const DevJob* jobs;
};

// The body of ppqhip_fq_linear_multi / ppqhip_fq_float_multi.  fill(job, &fmt) checks the format fields of a public job and writes
// them (it is also the probe of the validation loop); launch(workgroups, args) starts the kernel for `rounding`.
template <typename Fmt, typename Job, typename Fill, typename Launch>
inline int fq_multi(const char* what, KernelId id, const Job* jobs, int num_jobs, int rounding, void* device_table, int upload,
                    hipStream_t s, Fill fill, Launch launch) {
    typedef FqJobOf<Fmt> DevJob;
    if (num_jobs <= 0) return PPQHIP_OK;
    if (jobs == nullptr || device_table == nullptr) {
        set_error("%s: jobs / device_table is null", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const Job& j = jobs[k];
        if (int st = validate_n(j.n, what)) return st;
        if (int st = validate_channels(j.n, j.num_channel, j.elem_per_channel, what)) return st;
        if (!j.x || !j.out || !j.scale || !j.offset) {
            set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE;
        }
        Fmt probe;
        if (int st = fill(j, &probe)) return st;
        bytes += 8.0 * (double)j.n;
    }
    LaunchScope scope(id, bytes, s);
    for (int base = 0; base < num_jobs; base += kFqMultiMax) {
        const int count = (num_jobs - base) < kFqMultiMax ? (num_jobs - base) : kFqMultiMax;
        FqMultiArgsOf<DevJob> args;
        args.count = (uint32_t)count; args.rounding = rounding;
        args.jobs = (const DevJob*)device_table + base;
        std::vector<DevJob> table(upload ? count : 0);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const Job& src = jobs[base + k];
            const bool vec = fq_vec_ok(src.x, src.out, src.elem_per_channel);
            args.first_block[k] = blocks;
            const uint64_t quads = ((uint64_t)src.n + 3) / 4;
            blocks += (uint32_t)((quads + kBlock * kFqMultiU - 1) / (kBlock * kFqMultiU));
            if (upload) {
                DevJob& d = table[k];
                d.x = src.x; d.out = src.out; d.scale = src.scale; d.offset = src.offset;
                d.n = (uint32_t)src.n; d.vec_ok = vec ? 1u : 0u;
                d.per = make_fastdiv((uint32_t)(vec ? src.elem_per_channel / 4 : src.elem_per_channel));
                d.nc = make_fastdiv((uint32_t)src.num_channel);
                fill(src, &d.fmt);
            }
        }
        if (upload) {
            // pageable source: the runtime stages the copy before returning, `table` may go out of scope
            if (int st = check_hip(hipMemcpyAsync((DevJob*)device_table + base, table.data(), sizeof(DevJob) * count,
                                                  hipMemcpyHostToDevice, s), (std::string(what) + " table upload").c_str()))
                return st;
        }
        launch(blocks, args);
    }
    return finish_launch(what);
}

#if defined(__HIPCC__)

// ---- device: forward ------------------------------------------------------------------------------------------------------------
// What runs under the bounds test of a float4.  FQ_STORE_ONLY is the tuned shape (header).  The other two exist ONLY because the
// FP8 kernels had drifted to them before the walk was shared and unifying them is a tuning change of its own: they keep every
// kernel's code as it was.
enum FqPredication {
    FQ_STORE_ONLY = 0,    // unconditional arithmetic, predicated store
    FQ_GUARD_SLOW = 1,    // the same where q.fast(state); arithmetic and store under the test elsewhere (FP8 tile kernels)
    FQ_GUARD_ALL = 2,     // arithmetic and store under the test (FP8 multi kernel)
};

template <int PRED, typename Q>
__device__ __forceinline__ void fq_emit(const Q& q, const float4& a, const typename Q::State& st, uint32_t vv, uint32_t nvec,
                                        float4* out) {
    bool unconditional = PRED == FQ_STORE_ONLY;
    if constexpr (PRED == FQ_GUARD_SLOW) unconditional = q.fast(st);
    if (unconditional) {
        const float4 r = q.quant4(a, st);
        if (vv < nvec) out[vv] = r;
    } else if (vv < nvec) {
        out[vv] = q.quant4(a, st);
    }
}

// Per tensor: workgroup `blockIdx.x` owns float4s [b * kBlock * U, (b + 1) * kBlock * U); the scale is uniform (SGPRs) and read
// behind the loads; workgroup 0 also quantises the ntail < 4 elements behind the last float4.
template <int U, bool NT, int PRED, typename Q>
__device__ __forceinline__ void fq_tile_t(const Q& q, const float4* x, const float* scale, const float* offset, float4* out,
                                          uint32_t nvec, const float* xtail, float* otail, int ntail) {
    const uint32_t base = blockIdx.x * (kBlock * U) + threadIdx.x;
    float4 a[U];
#pragma unroll
    for (int k = 0; k < U; k++) a[k] = load4<NT>(&x[min(base + k * kBlock, nvec - 1)]);
    const typename Q::State st = q.make(scale[0], offset[0]);
    auto rest = [&](auto pred) {
#pragma unroll
        for (int k = 0; k < U; k++) fq_emit<decltype(pred)::value>(q, a[k], st, base + k * kBlock, nvec, out);
        if (blockIdx.x == 0 && (int)threadIdx.x < ntail) otail[threadIdx.x] = q.quant1(xtail[threadIdx.x], st);
    };
    if constexpr (PRED == FQ_GUARD_SLOW) {                             // kernel-uniform
        if (q.fast(st)) rest(std::integral_constant<int, FQ_STORE_ONLY>());
        else rest(std::integral_constant<int, FQ_GUARD_ALL>());
    } else {
        rest(std::integral_constant<int, PRED>());
    }
}

// Per channel: tile `local` of a tensor of nvec float4; the channel of a float4 is found with two multiply-high divisions by
// invariants (`per` float4 per channel row, `nc` channels), the scale / offset gathers hit L1 / L2.  Callers hand in job fields by
// value: read through a job inside the walk, they are fetched again after every store (1 - 5 % on the MX bodies).
template <int U, bool NT, int PRED, typename Q>
__device__ __forceinline__ void fq_tile_c(const Q& q, const float4* x, const float* scale, const float* offset, float4* out,
                                          uint32_t nvec, uint32_t local, FastDiv per, FastDiv nc) {
    const uint32_t base = local * (kBlock * U) + threadIdx.x;
    float4 a[U];
    typename Q::State st[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
        const uint32_t vv = min(base + k * kBlock, nvec - 1);
        a[k] = load4<NT>(&x[vv]);
        const uint32_t row = fdiv(vv, per);
        const uint32_t c = row - fdiv(row, nc) * nc.d;
        st[k] = q.make(scale[c], offset[c]);
    }
#pragma unroll
    for (int k = 0; k < U; k++) fq_emit<PRED>(q, a[k], st[k], base + k * kBlock, nvec, out);
}

// Element-wise: elements begin, begin + stride, .. below end, through the scalar arithmetic of the policy -- a grid-stride range
// (tensors that cannot be vectorised, n < 4) or the four elements of a lane's float4 (a job of the multi kernels)
template <typename Q>
__device__ __forceinline__ void fq_elems(const Q& q, const float* x, const float* scale, const float* offset, float* out,
                                         uint32_t begin, uint32_t end, uint32_t stride, bool per_channel, FastDiv per, FastDiv nc) {
    for (uint32_t i = begin; i < end; i += stride) {
        uint32_t c = 0;
        if (per_channel) {
            const uint32_t row = fdiv(i, per);
            c = row - fdiv(row, nc) * nc.d;
        }
        out[i] = q.quant1(x[i], q.make(scale[c], offset[c]));
    }
}

// one workgroup of a multi kernel: tile `local` of a job, whose fields arrive by value
template <int U, int PRED, typename Q>
__device__ __forceinline__ void fq_multi_tile(const Q& q, const float* x, float* out, const float* scale, const float* offset, uint32_t n,
                                              uint32_t vec_ok, FastDiv per, FastDiv nc, uint32_t local) {
    if (vec_ok) {
        fq_tile_c<U, false, PRED>(q, reinterpret_cast<const float4*>(x), scale, offset, reinterpret_cast<float4*>(out), n >> 2, local,
                                  per, nc);
    } else {
        const uint32_t base = local * (kBlock * U) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint32_t e0 = (base + k * kBlock) * 4;
            fq_elems(q, x, scale, offset, out, e0, min(e0 + 4u, n), 1u, true, per, nc);
        }
    }
}

// ---- device: backward -----------------------------------------------------------------------------------------------------------
// Elements [lo, hi) of one channel row (x, dy, gx point at the row): elem(x, dy, &gx) returns the element's term of d(loss)/d(scale),
// which is added to the lane's accumulator `acc` in walk order.  vec_ok (row length, lo and chunk size % 4 == 0, 16-B aligned
// rows): U (x, dy) load pairs in flight per lane -- a 56 x 56 row (784 float4) is ONE trip of 4, all 8 loads issued up front (one
// pair per dependent trip kept the row kernel at 0.68 of the roofline on [32, 512, 56, 56]); the loads are clamped so that they
// stay unconditional.
// The pointer parameters of the walks carry NO __restrict__ (the kernels' own parameters do): on an inlined function it becomes
// scoped alias information that lets the backend sink each (x, dy) pair behind the previous store, into its `break` test -- one
// pair per dependent trip again, +2.2 % on lsq_bwd_c at [32, 512, 56, 56] (profiles/fq_walk.txt).
template <int U, bool NT, typename Elem>
__device__ __forceinline__ float fq_bwd_row(const float* x, const float* dy, float* gx, uint32_t lo, uint32_t hi, bool vec_ok,
                                            float acc, const Elem& elem) {
    if (vec_ok) {
        const float4* xv = reinterpret_cast<const float4*>(x);
        const float4* dv = reinterpret_cast<const float4*>(dy);
        float4* gv = reinterpret_cast<float4*>(gx);
        const uint32_t v1 = hi >> 2;
        for (uint32_t v = (lo >> 2) + threadIdx.x; v < v1; v += kBlock * U) {
            float4 a[U], d[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t at = min(v + u * kBlock, v1 - 1);
                a[u] = load4<NT>(&xv[at]); d[u] = load4<NT>(&dv[at]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (v + u * kBlock >= v1) break;
                float4 g;
                acc += elem(a[u].x, d[u].x, &g.x);
                acc += elem(a[u].y, d[u].y, &g.y);
                acc += elem(a[u].z, d[u].z, &g.z);
                acc += elem(a[u].w, d[u].w, &g.w);
                gv[v + u * kBlock] = g;
            }
        }
    } else {
        for (uint32_t j = lo + threadIdx.x; j < hi; j += kBlock) {
            float g;
            acc += elem(x[j], dy[j], &g);
            gx[j] = g;
        }
    }
    return acc;
}

// Short channel rows (channel-last views, [N, C] matrices): grid-stride over elements, per-channel sums through atomics into LDS
// accumulators (use_lds: num_channel floats of dynamic LDS) or straight to global memory, one flush per workgroup.
// elem(c, x, dy, &gx) returns the element's term, fin(sum) scales what is added to gs[c].
template <typename Elem, typename Fin>
__device__ __forceinline__ void fq_bwd_generic(const float* x, const float* dy, float* gx,
                                               float* gs, uint32_t n, FastDiv elem_per_channel, FastDiv num_channel,
                                               int use_lds, Elem elem, Fin fin) {
    extern __shared__ float acc_lds[];
    const uint32_t C = num_channel.d;
    if (use_lds) {
        for (uint32_t c = threadIdx.x; c < C; c += kBlock) acc_lds[c] = 0.f;
        __syncthreads();
    }
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t row = fdiv(i, elem_per_channel);
        const uint32_t c = row - fdiv(row, num_channel) * C;
        float g;
        const float p = elem(c, x[i], dy[i], &g);
        gx[i] = g;
        if (use_lds) atomicAdd(&acc_lds[c], p);
        else atomicAdd(&gs[c], fin(p));
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < C; c += kBlock) {
            const float v = acc_lds[c];
            if (v != 0.f) atomicAdd(&gs[c], fin(v));
        }
    }
}

// The sum of partial(0) .. partial(count - 1) by one workgroup of BLOCK lanes, 8 loads in flight per lane, double accumulation in
// a FIXED order (lane l adds partial(l), partial(l + BLOCK), ..; then lanes, then waves, in index order): the result does not
// depend on timing.  Valid in thread 0.
// (256 lanes adding one partial per dependent trip took 13.8 us for the 12544 partials of a [32, 512, 56, 56] tensor.)
template <int BLOCK, typename Partial>
__device__ __forceinline__ double fq_finish_sum(uint32_t count, Partial partial) {
    __shared__ double lds[BLOCK / kWave];
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < count; i += 8 * BLOCK) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t at = i + u * BLOCK; v[u] = at < count ? partial(at) : 0.f; }
#pragma unroll
        for (int u = 0; u < 8; u++) acc += (double)v[u];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / kWave; w++) t += lds[w];
    return t;
}

#endif  // __HIPCC__

}  // namespace ppqhip
