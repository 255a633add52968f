// roundtune.hip -- the forward of the reference's round-tuning delegator, every round-tuned weight of a block in ONE launch.
// Mirror of ppq/quantization/algorithm/training.py:490-527 (TensorwiseRoundTuningImpl / ChannelwiseRoundTuningImpl.forward).
// There is no backward kernel: the reference's backward is the identity (dR = dy, :502-504 / :524-526).
//
// Bitwise the torch sequence (fp32, -ffp-contract=off, Makefile), op for op:
//   q = w / s  (IEEE quotient; w is the pre-floored weight floor(W / s) * s, so q is only APPROXIMATELY an integer and nothing
//   rounds it: no reciprocal shortcut)      q = q + (r > .5f ? 1.f : 0.f)  (r NaN: + 0)      q = q + o
//   out = (clamp(q, qmin, qmax) - o) * s
// clamp is torch's `isnan(v) ? v : min(max(v, lo), hi)` with the Python ints converted to float: NaN in, NaN out.
//
// Job table: DESIGN.md, "Job tables" (capturable into a HIP graph).  Geometry and walk: channel_axis.hpp (a per-tensor job has
// num_channel = 1); 16-B loads and stores where every pointer of the job is aligned.  No atomics, no reductions.
#include "channel_axis.hpp"
#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

constexpr int kRtMaxJobs = 16;                     // 16 x 88 B of job table: well inside the 4 KB of kernel arguments

struct RtJob {                                     // 88 B
    const float* w;
    const float* r;
    const float* scale;
    const float* offset;
    float* out;
    ChannelAxisMap map;
    float qmin, qmax;
};
struct RtArgs {
    RtJob jobs[kRtMaxJobs];
    uint32_t first_block[kRtMaxJobs];
    uint32_t count;
};
static_assert(sizeof(RtArgs) <= 4096, "kernel arguments are limited to 4 KB");

// the forward chain of one element
__device__ __forceinline__ float rt_forward(float w, float r, float s, float o, float qmin, float qmax) {
    const float q = w / s;
    const float u = q + (r > 0.5f ? 1.0f : 0.0f);
    const float t = u + o;
    const float c = clamp_nan(t, qmin, qmax);
    return (c - o) * s;
}

__device__ __forceinline__ void rt_job(const RtJob& j, uint32_t local) {
    const float4* w4 = reinterpret_cast<const float4*>(j.w);
    const float4* r4 = reinterpret_cast<const float4*>(j.r);
    float4* o4 = reinterpret_cast<float4*>(j.out);
    auto one = [&](float w, float r, uint32_t c) { return rt_forward(w, r, j.scale[c], j.offset[c], j.qmin, j.qmax); };
    walk_channel_axis(j.map, local,
                      [&](uint32_t i, uint32_t c) { j.out[i] = one(j.w[i], j.r[i], c); },
                      [&](uint32_t q) {
                          const float4 w = w4[q], r = r4[q];
                          const Channels4 c = channels_of_float4(j.map, q);             // behind the loads: channel_axis.hpp
                          o4[q] = make_float4(one(w.x, r.x, c.c0), one(w.y, r.y, c.c1), one(w.z, r.z, c.c2), one(w.w, r.w, c.c3));
                      });
}

__global__ __launch_bounds__(kBlock) void roundtune_fwd_kernel(const RtArgs args) {
    uint32_t local;
    const uint32_t k = job_of(args, local);
    rt_job(args.jobs[k], local);
}

int validate_jobs(const ppqhip_roundtune_job* jobs, int num_jobs, const char* what) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_roundtune_job& j = jobs[k];
        if (int st = validate_channel_axis(what, j.n, j.num_channel, j.elem_per_channel, k)) return st;
        if (!j.w || !j.r || !j.scale || !j.offset || !j.out) {
            set_error("%s: job %d has a null pointer", what, k);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        if (j.qmin > j.qmax) { set_error("%s: job %d: quant_min > quant_max", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    }
    return PPQHIP_OK;
}

void launch_roundtune(const ppqhip_roundtune_job* jobs, int num_jobs, hipStream_t s) {
    for (int base = 0; base < num_jobs; base += kRtMaxJobs) {
        RtArgs args;
        const int count = min(kRtMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_roundtune_job& src = jobs[base + k];
            RtJob& d = args.jobs[k];
            d.w = src.w; d.r = src.r; d.scale = src.scale; d.offset = src.offset; d.out = src.out;
            const bool aligned = aligned16(src.w) && aligned16(src.r) && aligned16(src.out);
            d.map = pack_channel_axis(aligned, src.n, src.num_channel, src.elem_per_channel);
            d.qmin = (float)src.qmin; d.qmax = (float)src.qmax;
            args.first_block[k] = blocks;
            blocks += d.map.blocks;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        hipLaunchKernelGGL(roundtune_fwd_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_roundtune_fwd_multi(const ppqhip_roundtune_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_jobs(jobs, num_jobs, "roundtune_fwd_multi")) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) bytes += 12.0 * (double)jobs[k].n;          // w, r in; out
    LaunchScope scope(K_ROUNDTUNE_FWD, bytes, s);
    launch_roundtune(jobs, num_jobs, s);
    return finish_launch("roundtune_fwd_multi");
}

}  // extern "C"
