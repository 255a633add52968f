// equalize.hip -- layerwise equalization: the scales of a group of independent pairs in ONE launch, their application in another.
// Mirror of ppq/quantization/algorithm/equalization.py:27-198 (EqualizationHelper) and :419-436 (calculate_scale over
// reduce_by_axis(ABSOLUTE_MAX)), which the reference runs as ~20 small torch ops per pair and iteration.
//
// Bitwise the torch sequence (fp32, -ffp-contract=off, correctly rounded division and square root: common.hpp), op for op:
//   up = max |x * m| over the upstream rows, down = the same over the downstream slices (max is order independent; a NaN wins as
//   in torch.max)      q = up / down      r = sqrt(q)      s = 1.0f / r      s = clamp(s, 0.1f, 10.0f) (NaN kept)
//   s = 1 where up + down < threshold
//   upstream weight / bias: x = x * s[c]          downstream weight: x = x / s[k]  (IEEE quotient)
//
// Two kernels, not one per channel: for a grouped downstream Conv the reference orders its key rows (cin_local, group) but applies
// the scale in (group, cin_local) order, so the slice a channel READS for its key is not the slice its scale is APPLIED to -- a
// fused reduce-and-apply workgroup would race with its neighbours.
//
// Job tables: DESIGN.md, "Job tables".  No atomics; the reductions are the wave64 shuffle + LDS pattern of reduce.hip.
#include "channel_scale.hpp"
#include "common.hpp"
#include "equalize_key.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

// ------------------------------------------------------------------------------------ scale
constexpr int kEqMaxJobs = 32;                     // pairs per launch
struct EqScaleJob {                                // 24 B
    float* scale;
    uint32_t C;
    float threshold;
    uint32_t seg_begin, seg_count;
};
struct EqScaleArgs {
    EqSeg segs[kEqMaxSegs];
    EqScaleJob jobs[kEqMaxJobs];
    uint32_t first_block[kEqMaxJobs];
    uint32_t count;
};
static_assert(sizeof(EqScaleArgs) <= 4096, "kernel arguments are limited to 4 KB");

// one workgroup per (job, channel): lanes stride over the channel's elements of every segment
__global__ __launch_bounds__(kBlock) void equalize_scale_kernel(const EqScaleArgs args) {
    __shared__ float lds[4 * (kBlock / kWave)];
    uint32_t c;
    const EqScaleJob& j = args.jobs[job_of(args, c)];
    float up, dn;
    eq_channel_keys(args.segs + j.seg_begin, j.seg_count, c, lds, up, dn);
    if (threadIdx.x == 0) {
        const float q = up / dn;
        const float r = __builtin_sqrtf(q);
        float s = 1.0f / r;
        s = clamp_nan(s, 0.1f, 10.0f);
        if (up + dn < j.threshold) s = 1.0f;
        j.scale[c] = s;
    }
}

// ------------------------------------------------------------------------------------ apply
constexpr int kEqApMaxJobs = 32;
struct EqApJob {                                   // 72 B
    float* x;
    const float* scale;
    ChannelScaleMap g;
};
struct EqApArgs {
    EqApJob jobs[kEqApMaxJobs];
    uint32_t first_block[kEqApMaxJobs];
    uint32_t count;
};
static_assert(sizeof(EqApArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBlock) void equalize_apply_kernel(const EqApArgs args) {
    uint32_t local;
    const EqApJob& j = args.jobs[job_of(args, local)];
    const ChannelScaleMap& g = j.g;
    const uint32_t stride = g.blocks * kBlock;
    const uint32_t first = local * kBlock + threadIdx.x;
    if (g.nvec == 0) {                                                    // unaligned pointer or run % 4 != 0
        for (uint32_t i = first; i < g.n; i += stride) {
            const float s = j.scale[channel_scale_index(g, i)];
            const float x = j.x[i];
            j.x[i] = g.divide ? x / s : x * s;
        }
        return;
    }
    float4* x4 = reinterpret_cast<float4*>(j.x);
    for (uint32_t q = first; q < g.nvec; q += stride) {                   // one channel per float4
        const float s = j.scale[channel_scale_index(g, q)];
        float4 v = x4[q];
        if (g.divide) { v.x = v.x / s; v.y = v.y / s; v.z = v.z / s; v.w = v.w / s; }
        else { v.x = v.x * s; v.y = v.y * s; v.z = v.z * s; v.w = v.w * s; }
        x4[q] = v;
    }
}

int validate_scale(const ppqhip_equalize_scale_job* jobs, int num_jobs) {
    const char* what = "equalize_scale_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_equalize_scale_job& j = jobs[k];
        if (j.segments == nullptr || j.scale == nullptr || j.num_channel <= 0 || j.num_segments <= 0) {
            set_error("%s: job %d: null pointer, no channel or no segment", what, k); return PPQHIP_ERR_INVALID_VALUE;
        }
        if (int st = validate_segments(what, k, j.segments, j.num_segments, j.num_channel)) return st;
    }
    return PPQHIP_OK;
}

void launch_scale(const ppqhip_equalize_scale_job* jobs, int num_jobs, hipStream_t s) {
    for (int base = 0; base < num_jobs;) {
        EqScaleArgs args;
        uint32_t count = 0, segs = 0, blocks = 0;
        while (base + (int)count < num_jobs && count < (uint32_t)kEqMaxJobs &&
               segs + (uint32_t)jobs[base + count].num_segments <= (uint32_t)kEqMaxSegs) {
            const ppqhip_equalize_scale_job& src = jobs[base + count];
            EqScaleJob& d = args.jobs[count];
            d.scale = src.scale; d.C = (uint32_t)src.num_channel; d.threshold = src.value_threshold;
            d.seg_begin = segs; d.seg_count = (uint32_t)src.num_segments;
            for (int t = 0; t < src.num_segments; t++) args.segs[segs++] = pack_segment(src.segments[t]);
            args.first_block[count] = blocks;
            blocks += d.C;
            count++;
        }
        for (uint32_t k = segs; k < (uint32_t)kEqMaxSegs; k++) args.segs[k] = args.segs[0];
        pad_job_table(args, count, blocks);
        hipLaunchKernelGGL(equalize_scale_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
        base += (int)count;
    }
}

int validate_apply(const ppqhip_equalize_apply_job* jobs, int num_jobs) {
    const char* what = "equalize_apply_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_equalize_apply_job& j = jobs[k];
        if (j.x == nullptr || j.scale == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (int st = validate_channel_scale(what, k, kEqMax, j.n, j.run, j.inner, j.group_out, j.num_scale)) return st;
    }
    std::vector<Span> ins, outs;                                          // in place: two jobs on one tensor would race
    for (int k = 0; k < num_jobs; k++) outs.push_back(span_of(jobs[k].x, jobs[k].n));
    return check_overlap(what, ins, outs);
}

void launch_apply(const ppqhip_equalize_apply_job* jobs, int num_jobs, hipStream_t s) {
    for (int base = 0; base < num_jobs; base += kEqApMaxJobs) {
        EqApArgs args;
        const int count = std::min(kEqApMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_equalize_apply_job& src = jobs[base + k];
            EqApJob& d = args.jobs[k];
            d.x = src.x; d.scale = src.scale;
            d.g = pack_channel_scale(aligned16(src.x), src.n, src.run, src.inner, src.group_out, src.divide);
            args.first_block[k] = blocks;
            blocks += d.g.blocks;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        hipLaunchKernelGGL(equalize_apply_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_equalize_scale_multi(const ppqhip_equalize_scale_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_scale(jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        for (int t = 0; t < jobs[k].num_segments; t++)
            bytes += 4.0 * (double)jobs[k].num_channel * (double)(jobs[k].segments[t].outer * jobs[k].segments[t].run);
        bytes += 4.0 * (double)jobs[k].num_channel;
    }
    LaunchScope scope(K_EQUALIZE_SCALE, bytes, s);
    launch_scale(jobs, num_jobs, s);
    return finish_launch("equalize_scale_multi");
}

int ppqhip_equalize_apply_multi(const ppqhip_equalize_apply_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_apply(jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) bytes += 8.0 * (double)jobs[k].n;           // x in, x out
    LaunchScope scope(K_EQUALIZE_APPLY, bytes, s);
    launch_apply(jobs, num_jobs, s);
    return finish_launch("equalize_apply_multi");
}

}  // extern "C"
