// ssd.hip -- the three launches of SSD equalization (ppq_amd/ssd.py; mirror of ppq/quantization/optim/ssd.py).
//
// 1. ppqhip_ssd_scales_multi: the four candidate scales of a pair (one_step_equalization, ssd.py:288-320) from the two weight
//    ranges (prepare_weight_for_equalization, :152-210) and the activation range.  Two device kernels behind one entry point:
//    a workgroup per (pair, channel) reduces max |w| of the channel's rows of the first weight and of its slices of the last
//    weight (ppqhip_equalize_segment addressing; max is order independent, a NaN wins as in torch.max), then ONE workgroup per
//    pair does the cross-channel max / min (wave shuffle, then LDS -- exact) and the per-channel arithmetic.  Bitwise the torch
//    sequence, op for op (fp32, -ffp-contract=off, correctly rounded division and square root: common.hpp):
//      algo 0   s = clamp(sqrt(last / (first + 1e-8f)), 0.1f, 10.0f)
//      algo 1-3 first / last are floored at max * channel_ratio, the activation range at 0.01f;
//               ks = max(first) / (first + 1e-8f), nks = the same of last, as = the same of the activation range
//        1      s = min(ks, as)
//        2      s = min(min(ks / nks, as / nks), 8.0f);  s = s / min over the channels;  s = clamp(s, 1.0f, 2.0f)
//        3      s = clamp(sqrt(as * sqrt(ks / nks)), 1.0f, 2.0f)
//    (min / max / clamp keep a NaN as torch's do.)
// 2. ppqhip_ssd_apply_multi: write_back (:212-262) for all four candidates of every tensor of a pair, OUT OF PLACE: one read of
//    x, four writes.  The originals are never written: "recover" costs nothing.
// 3. ppqhip_fq_measure_rows_multi: the loss read.  The row sums of measure.hip between fake_quant(y) and r with the fake-quant
//    (common.hpp: fq_linear4 / fq_linear_scalar, the device functions of linear.hip's kernels) done in registers and the
//    accumulation of measure_rows.hpp -- the same lanes, the same order: bit-identical to ppqhip_fq_linear_{t,c} into a buffer
//    followed by ppqhip_measure_rows_multi on that buffer, with one read of y and r and no write.
//
// Job tables: DESIGN.md, "Job tables".  No synchronisation, no atomics.
#include "channel_scale.hpp"
#include "common.hpp"
#include "equalize_key.hpp"
#include "job_table.hpp"
#include "measure_rows.hpp"

namespace ppqhip {
namespace {

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : __builtin_fminf(a, b)); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : __builtin_fmaxf(a, b)); }

// NaN-propagating max / min of one value per thread over the workgroup; every thread gets the result.  `lds`: kWaves floats.
template <bool MAX>
__device__ __forceinline__ float block_extreme(float v, float* lds) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { const float o = __shfl_xor(v, m, 64); v = MAX ? nan_max(v, o) : nan_min(v, o); }
    __syncthreads();                                                      // the previous use of lds is over
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = lds[0];
    for (int w = 1; w < kWaves; w++) t = MAX ? nan_max(t, lds[w]) : nan_min(t, lds[w]);
    return t;
}

// ------------------------------------------------------------------------------------ scales
constexpr int kSsdMaxJobs = 24;

struct SsdScaleJob {                               // 112 B
    EqSeg seg[2];                                  // [0] first weight, [1] last weight (mult and flags are not read)
    const float* act;
    float* scales;                                 // [4][C]
    float* ranges;                                 // [2][C]
    uint32_t C;
    float ratio;
};
struct SsdScaleArgs {
    SsdScaleJob jobs[kSsdMaxJobs];
    uint32_t first_block[kSsdMaxJobs];
    uint32_t count;
};
static_assert(sizeof(SsdScaleArgs) <= 4096, "kernel arguments are limited to 4 KB");

// one workgroup per (job, channel): ranges[side][c] = max |w| over the channel's elements of the segment
__global__ __launch_bounds__(kBlock) void ssd_ranges_kernel(const SsdScaleArgs args) {
    __shared__ float lds[kWaves];
    uint32_t c;
    const SsdScaleJob& j = args.jobs[job_of(args, c)];
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const EqSeg& g = j.seg[side];
        const uint32_t q = c / g.div;
        const float* p = g.base + (size_t)q * g.a + (size_t)(c - q * g.div) * g.b;
        const uint32_t total = g.outer * g.run;
        float m = 0.f;                                                    // |x| >= 0: 0 is neutral
        for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
            const uint32_t o = (g.outer == 1) ? 0u : (g.run == 1 ? i : i / g.run), e = i - o * g.run;
            m = nan_max(m, __builtin_fabsf(p[(size_t)o * g.stride + e]));
        }
        m = block_extreme<true>(m, lds);
        if (threadIdx.x == 0) j.ranges[(size_t)side * j.C + c] = m;
    }
}

struct SsdPre { float ks, nks, as; };

// one workgroup per job: the cross-channel extremes, then the four scales of every channel
__global__ __launch_bounds__(kBlock) void ssd_scales_kernel(const SsdScaleArgs args) {
    __shared__ float lds[kWaves];
    const SsdScaleJob& j = args.jobs[blockIdx.x];
    const uint32_t C = j.C;
    const float* __restrict__ first = j.ranges;
    const float* __restrict__ last = j.ranges + C;
    const float* __restrict__ act = j.act;
    const float eps = 1e-8f, act_floor = 0.01f;
    float m1 = 0.f, m2 = 0.f, ma = act_floor;                            // ranges are |.| >= 0; the floored activation range >= 0.01
    for (uint32_t c = threadIdx.x; c < C; c += kBlock) {
        m1 = nan_max(m1, first[c]); m2 = nan_max(m2, last[c]);
        const float a = act[c];
        ma = nan_max(ma, a < act_floor ? act_floor : a);
    }
    m1 = block_extreme<true>(m1, lds); m2 = block_extreme<true>(m2, lds); ma = block_extreme<true>(ma, lds);
    const float t1 = m1 * j.ratio, t2 = m2 * j.ratio;
    // the max of the floored ranges: every channel is its own value or the floor, and the largest one is never below the floor
    // unless the ratio exceeds 1 -- then every channel is the floor
    const float f1 = nan_max(m1, t1), f2 = nan_max(m2, t2);
    auto pre = [&](uint32_t c) {
        const float a = first[c], b = last[c], r = act[c];
        const float af = a < t1 ? t1 : a, bf = b < t2 ? t2 : b, rf = r < act_floor ? act_floor : r;
        SsdPre p;
        p.ks = f1 / (af + eps);
        p.nks = f2 / (bf + eps);
        p.as = ma / (rf + eps);
        return p;
    };
    auto algo2 = [&](const SsdPre& p) {
        const float k = p.ks / p.nks, a = p.as / p.nks;
        return nan_min(nan_min(k, a), 8.0f);
    };
    float low = INFINITY;
    for (uint32_t c = threadIdx.x; c < C; c += kBlock) low = nan_min(low, algo2(pre(c)));
    low = block_extreme<false>(low, lds);
    for (uint32_t c = threadIdx.x; c < C; c += kBlock) {
        const float q0 = last[c] / (first[c] + eps);
        j.scales[c] = clamp_nan(__builtin_sqrtf(q0), 0.1f, 10.0f);
        const SsdPre p = pre(c);
        j.scales[(size_t)C + c] = nan_min(p.ks, p.as);
        const float s2 = algo2(p) / low;
        j.scales[(size_t)2 * C + c] = clamp_nan(s2, 1.0f, 2.0f);
        const float k3 = __builtin_sqrtf(p.ks / p.nks);
        const float s3 = __builtin_sqrtf(p.as * k3);
        j.scales[(size_t)3 * C + c] = clamp_nan(s3, 1.0f, 2.0f);
    }
}

// ------------------------------------------------------------------------------------ apply
constexpr int kSsdApMaxJobs = 32;
struct SsdApJob {                                  // 88 B
    const float* x;
    float* out;                                    // [4][n]
    const float* scale;                            // [4][C]
    ChannelScaleMap g;
    uint32_t C;
};
struct SsdApArgs {
    SsdApJob jobs[kSsdApMaxJobs];
    uint32_t first_block[kSsdApMaxJobs];
    uint32_t count;
};
static_assert(sizeof(SsdApArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBlock) void ssd_apply_kernel(const SsdApArgs args) {
    uint32_t local;
    const SsdApJob& j = args.jobs[job_of(args, local)];
    const ChannelScaleMap& g = j.g;
    const uint32_t stride = g.blocks * kBlock;
    const uint32_t first = local * kBlock + threadIdx.x;
    if (g.nvec == 0) {                                                    // unaligned pointer or run % 4 != 0
        for (uint32_t i = first; i < g.n; i += stride) {
            const uint32_t k = channel_scale_index(g, i);
            const float x = j.x[i];
#pragma unroll
            for (uint32_t cand = 0; cand < 4; cand++) {
                const float s = j.scale[(size_t)cand * j.C + k];
                j.out[(size_t)cand * g.n + i] = g.divide ? x / s : x * s;
            }
        }
        return;
    }
    const float4* x4 = reinterpret_cast<const float4*>(j.x);
    for (uint32_t q = first; q < g.nvec; q += stride) {                   // one channel per float4
        const uint32_t k = channel_scale_index(g, q);
        const float4 v = x4[q];
#pragma unroll
        for (uint32_t cand = 0; cand < 4; cand++) {
            const float s = j.scale[(size_t)cand * j.C + k];
            float4 r;
            if (g.divide) { r.x = v.x / s; r.y = v.y / s; r.z = v.z / s; r.w = v.w / s; }
            else { r.x = v.x * s; r.y = v.y * s; r.z = v.z * s; r.w = v.w * s; }
            reinterpret_cast<float4*>(j.out + (size_t)cand * g.n)[q] = r;   // n % 4 == 0 here: every candidate stays 16-B aligned
        }
    }
}

// ------------------------------------------------------------------------------------ fake-quant + row sums
constexpr int kFqMsMaxJobs = 32;

struct FqX {                                       // 48 B: the fake-quant applied to the p slots of measure_rows.hpp
    const float* scale;
    const float* offset;
    FastDiv epc;                                   // elements per channel
    uint32_t C;                                    // 1: per tensor
    int qmin, qmax, rounding;
    uint32_t whole4;                               // the four elements of an aligned slot share a channel

    __device__ __forceinline__ uint32_t channel(uint32_t e) const { return C == 1 ? 0u : min(fdiv(e, epc), C - 1u); }
    __device__ __forceinline__ float one(float x, uint32_t e) const {
        const uint32_t c = channel(e);
        const float s = scale[c];
        const int o = round_offset(offset[c]);
        return rounding == ROUND_HALF_EVEN ? fq_linear_scalar<ROUND_HALF_EVEN>(x, s, o, qmin, qmax, rounding)
                                           : fq_linear_scalar<-1>(x, s, o, qmin, qmax, rounding);
    }
    __device__ __forceinline__ float4 operator()(const float4& a, uint32_t e, int valid) const {
        float4 q;
        if (whole4) {
            const uint32_t c = channel(e);
            const float s = scale[c];
            const int o = round_offset(offset[c]);
            q = rounding == ROUND_HALF_EVEN ? fq_linear4<ROUND_HALF_EVEN>(a, s, fq_safe_rcp(s), o, qmin, qmax, rounding)
                                            : fq_linear4<-1>(a, s, fq_safe_rcp(s), o, qmin, qmax, rounding);
        } else {
            q.x = one(a.x, e); q.y = one(a.y, e + 1); q.z = one(a.z, e + 2); q.w = one(a.w, e + 3);
        }
        // a slot past the end of the row holds 0 in r: it must add nothing, whatever fake_quant(0) is
        if (valid < 4) { q.w = 0.f; if (valid < 3) q.z = 0.f; if (valid < 2) q.y = 0.f; if (valid < 1) q.x = 0.f; }
        return q;
    }
};
struct FqMsArgs {
    MsJob jobs[kFqMsMaxJobs];
    FqX fx[kFqMsMaxJobs];
    uint32_t first_block[kFqMsMaxJobs];
    uint32_t count;
    double* scratch;
};
static_assert(sizeof(FqMsArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBlock) void fq_measure_rows_kernel(const FqMsArgs args) {
    __shared__ double lds[kWaves][4];
    uint32_t local;
    const uint32_t k = job_of(args, local);
    measure_job<false>(args.jobs[k], local, args.scratch, lds, args.fx[k]);
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_ssd_scales_multi(const ppqhip_ssd_scales_job* jobs, int num_jobs, void* stream) {
    const char* what = "ssd_scales_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_ssd_scales_job& j = jobs[k];
        if (j.act_range == nullptr || j.scales == nullptr || j.ranges == nullptr || j.num_channel <= 0) {
            set_error("%s: job %d: null pointer or no channel", what, k); return PPQHIP_ERR_INVALID_VALUE;
        }
        if (int st = validate_segment(what, k, "first", 0, j.first, j.num_channel)) return st;
        if (int st = validate_segment(what, k, "last", 1, j.last, j.num_channel)) return st;
        bytes += 4.0 * (double)j.num_channel * (double)(j.first.outer * j.first.run + j.last.outer * j.last.run + 7);
    }
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_SSD_SCALES, bytes, s);
    for (int base = 0; base < num_jobs; base += kSsdMaxJobs) {
        SsdScaleArgs args;
        const int count = std::min(kSsdMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_ssd_scales_job& src = jobs[base + k];
            SsdScaleJob& d = args.jobs[k];
            d.seg[0] = pack_segment(src.first); d.seg[1] = pack_segment(src.last);
            d.act = src.act_range; d.scales = src.scales; d.ranges = src.ranges;
            d.C = (uint32_t)src.num_channel; d.ratio = src.channel_ratio;
            args.first_block[k] = blocks;
            blocks += d.C;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        hipLaunchKernelGGL(ssd_ranges_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
        hipLaunchKernelGGL(ssd_scales_kernel, dim3((uint32_t)count), dim3(kBlock), 0, s, args);
    }
    return finish_launch(what);
}

int ppqhip_ssd_apply_multi(const ppqhip_ssd_apply_job* jobs, int num_jobs, void* stream) {
    const char* what = "ssd_apply_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    double bytes = 0.0;
    std::vector<Span> ins, outs;                                          // an output over an input (or another output) would race
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_ssd_apply_job& j = jobs[k];
        if (j.x == nullptr || j.out == nullptr || j.scales == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (j.num_channel > kEqMax) { set_error("%s: job %d: more than 2^31 - 1 channels", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (int st = validate_channel_scale(what, k, kEqMax / 4, j.n, j.run, j.inner, j.group_out, j.num_channel)) return st;   // out is [4][n]
        ins.push_back(span_of(j.x, j.n));
        outs.push_back(span_of(j.out, 4 * j.n));
        bytes += 20.0 * (double)j.n;                                      // x in, four candidates out
    }
    if (int st = check_overlap(what, ins, outs)) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_SSD_APPLY, bytes, s);
    for (int base = 0; base < num_jobs; base += kSsdApMaxJobs) {
        SsdApArgs args;
        const int count = std::min(kSsdApMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_ssd_apply_job& src = jobs[base + k];
            SsdApJob& d = args.jobs[k];
            d.x = src.x; d.out = src.out; d.scale = src.scales; d.C = (uint32_t)src.num_channel;
            d.g = pack_channel_scale(aligned16(src.x) && aligned16(src.out), src.n, src.run, src.inner, src.group_out, src.divide);
            args.first_block[k] = blocks;
            blocks += d.g.blocks;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        hipLaunchKernelGGL(ssd_apply_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
    return finish_launch(what);
}

int ppqhip_fq_measure_rows_multi(const ppqhip_fq_measure_rows_job* jobs, int num_jobs, void* stream) {
    const char* what = "fq_measure_rows_multi";
    if (num_jobs <= 0) return PPQHIP_OK;
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_fq_measure_rows_job& j = jobs[k];
        if (int st = validate_rows(j.rows, j.count, j.count, what, k)) return st;
        if (!j.y || !j.r || !j.sums || !j.scale || !j.offset) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (j.num_channel <= 0 || j.elem_per_channel <= 0 || j.num_channel * j.elem_per_channel != j.count) {
            set_error("%s: job %d: a row of %lld is not [%lld channels, %lld elem/channel]", what, k, (long long)j.count,
                      (long long)j.num_channel, (long long)j.elem_per_channel);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        const int64_t chunks = (j.count + kChunk - 1) / kChunk;
        if (j.rows * chunks > 0x3fffffffLL) { set_error("%s: job %d: too many work items", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        bytes += (double)j.rows * (double)j.count * 8.0 + 32.0 * (double)j.rows;
    }
    LaunchScope scope(K_FQ_MEASURE_ROWS, bytes, s);
    for (int base = 0; base < num_jobs; ) {                              // the chunking of ppqhip_measure_rows_multi
        FqMsArgs args;
        FoldArgs fold;
        uint64_t blocks = 0, partials = 0, fold_blocks = 0;
        int count = 0, folds = 0;
        for (; count < kFqMsMaxJobs && base + count < num_jobs; count++) {
            const ppqhip_fq_measure_rows_job& src = jobs[base + count];
            const uint32_t chunks = src.count <= kWaveRow ? 0u : (uint32_t)((src.count + kChunk - 1) / kChunk);
            const uint64_t need = chunks == 0 ? (uint64_t)((src.rows + kWaves - 1) / kWaves) : (uint64_t)src.rows * chunks;
            if (blocks + need > 0x7fffffffULL && count > 0) break;      // the rest goes into the next launch
            MsJob& d = args.jobs[count];
            d.p = src.y; d.r = src.r; d.index = nullptr; d.sums = src.sums;
            d.rows = (uint32_t)src.rows; d.row_len = (uint32_t)src.count; d.count = (uint32_t)src.count; d.chunks = chunks;
            d.partial = (uint32_t)partials;
            d.index_vec = 0; d.pad0 = d.pad1 = 0;
            FqX& f = args.fx[count];
            f.scale = src.scale; f.offset = src.offset; f.epc = make_fastdiv((uint32_t)src.elem_per_channel);
            f.C = (uint32_t)src.num_channel; f.qmin = src.clip_min; f.qmax = src.clip_max; f.rounding = src.rounding;
            f.whole4 = (src.num_channel == 1 || src.elem_per_channel % 4 == 0) ? 1u : 0u;
            args.first_block[count] = (uint32_t)blocks;
            blocks += need;
            if (chunks > 1) {
                FoldJob& g = fold.jobs[folds];
                g.sums = src.sums; g.rows = d.rows; g.chunks = chunks; g.partial = d.partial; g.pad = 0;
                fold.first_block[folds++] = (uint32_t)fold_blocks;
                fold_blocks += ((uint64_t)src.rows + kWaves - 1) / kWaves;
                partials += need;
            }
        }
        for (int k = count; k < kFqMsMaxJobs; k++) args.fx[k] = args.fx[0];
        pad_job_table(args, (uint32_t)count, (uint32_t)blocks);
        args.scratch = nullptr;
        if (folds > 0) {
            args.scratch = (double*)scratch(s, (size_t)partials * 4 * sizeof(double));
            if (!args.scratch) return PPQHIP_ERR_HIP;
        }
        hipLaunchKernelGGL(fq_measure_rows_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
        if (folds > 0) {
            pad_job_table(fold, (uint32_t)folds, (uint32_t)fold_blocks);
            fold.scratch = args.scratch;
            launch_measure_fold(fold, (uint32_t)fold_blocks, s);
        }
        base += count;
    }
    return finish_launch(what);
}

}  // extern "C"
