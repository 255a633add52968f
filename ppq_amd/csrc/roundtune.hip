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
// Job table: DESIGN.md, "Job tables" (capturable into a HIP graph).  channel(i) = (i / elem_per_channel) % num_channel with FastDiv (a per-tensor job has num_channel = 1).  16-B loads and
// stores where every pointer of the job is aligned, the n % 4 tail by the job's first workgroup; element-wise otherwise.  No
// atomics, no reductions.
#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

constexpr int kRtMaxJobs = 16;                     // 16 x 88 B of job table: well inside the 4 KB of kernel arguments
constexpr uint32_t kRtMaxBlocksPerJob = 1024;      // grid-strided beyond: 256 K lanes per job cover the largest weights in ~3 trips

struct RtJob {                                     // 88 B
    const float* w;
    const float* r;
    const float* scale;
    const float* offset;
    float* out;
    uint32_t n, nvec;                              // nvec: float4 count of the vector part (0: element-wise job)
    FastDiv epc, nc;
    float qmin, qmax;
    uint32_t plane;                                // epc % 4 == 0: one channel per float4
    uint32_t blocks;                               // workgroups of this job
};
struct RtArgs {
    RtJob jobs[kRtMaxJobs];
    uint32_t first_block[kRtMaxJobs];
    uint32_t count;
};
static_assert(sizeof(RtArgs) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ uint32_t rt_channel(uint32_t i, const FastDiv& epc, const FastDiv& nc) {
    const uint32_t row = fdiv(i, epc);
    return row - fdiv(row, nc) * nc.d;
}

// the forward chain of one element
__device__ __forceinline__ float rt_forward(float w, float r, float s, float o, float qmin, float qmax) {
    const float q = w / s;
    const float u = q + (r > 0.5f ? 1.0f : 0.0f);
    const float t = u + o;
    const float c = clamp_nan(t, qmin, qmax);
    return (c - o) * s;
}

__device__ __forceinline__ void rt_elem(const RtJob& j, uint32_t i) {
    const uint32_t c = rt_channel(i, j.epc, j.nc);
    j.out[i] = rt_forward(j.w[i], j.r[i], j.scale[c], j.offset[c], j.qmin, j.qmax);
}

__device__ __forceinline__ void rt_job(const RtJob& j, uint32_t local) {
    const uint32_t stride = j.blocks * kBlock;
    const uint32_t first = local * kBlock + threadIdx.x;
    if (j.nvec == 0) {                                               // unaligned pointers or n < 4: element-wise
        for (uint32_t i = first; i < j.n; i += stride) rt_elem(j, i);
        return;
    }
    const float4* w4 = reinterpret_cast<const float4*>(j.w);
    const float4* r4 = reinterpret_cast<const float4*>(j.r);
    float4* o4 = reinterpret_cast<float4*>(j.out);
    for (uint32_t q = first; q < j.nvec; q += stride) {
        const float4 w = w4[q], r = r4[q];
        const uint32_t i = q * 4u;
        uint32_t c0, c1, c2, c3;
        if (j.plane) { c0 = c1 = c2 = c3 = rt_channel(q, j.epc, j.nc); }            // j.epc holds epc / 4
        else {
            c0 = rt_channel(i, j.epc, j.nc); c1 = rt_channel(i + 1, j.epc, j.nc);
            c2 = rt_channel(i + 2, j.epc, j.nc); c3 = rt_channel(i + 3, j.epc, j.nc);
        }
        float4 y;
        y.x = rt_forward(w.x, r.x, j.scale[c0], j.offset[c0], j.qmin, j.qmax);
        y.y = rt_forward(w.y, r.y, j.scale[c1], j.offset[c1], j.qmin, j.qmax);
        y.z = rt_forward(w.z, r.z, j.scale[c2], j.offset[c2], j.qmin, j.qmax);
        y.w = rt_forward(w.w, r.w, j.scale[c3], j.offset[c3], j.qmin, j.qmax);
        o4[q] = y;
    }
    if (local == 0 && threadIdx.x < j.n - j.nvec * 4u) rt_elem(j, j.nvec * 4u + threadIdx.x);   // the n % 4 tail (never in the plane form)
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
        if (j.n <= 0 || j.n > 0x7fffffffLL) {
            set_error("%s: job %d: n=%lld is empty or has more than 2^31 - 1 elements", what, k, (long long)j.n);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        if (j.num_channel <= 0 || j.elem_per_channel <= 0 || j.num_channel > 0x7fffffffLL || j.elem_per_channel > 0x7fffffffLL ||
            j.n % (j.num_channel * j.elem_per_channel) != 0) {
            set_error("%s: job %d: n=%lld is not [outer, %lld channels, %lld elem/channel]", what, k, (long long)j.n,
                      (long long)j.num_channel, (long long)j.elem_per_channel);
            return PPQHIP_ERR_INVALID_VALUE;
        }
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
            d.n = (uint32_t)src.n;
            const bool aligned = aligned16(src.w) && aligned16(src.r) && aligned16(src.out);
            d.nvec = (aligned && src.n >= 4) ? (uint32_t)(src.n >> 2) : 0u;
            d.plane = (d.nvec > 0 && src.elem_per_channel % 4 == 0) ? 1u : 0u;
            d.epc = make_fastdiv((uint32_t)(d.plane ? src.elem_per_channel / 4 : src.elem_per_channel));
            d.nc = make_fastdiv((uint32_t)src.num_channel);
            d.qmin = (float)src.qmin; d.qmax = (float)src.qmax;
            const uint64_t work = d.nvec > 0 ? d.nvec : (uint64_t)src.n;
            d.blocks = (uint32_t)std::min<uint64_t>((work + kBlock - 1) / kBlock, kRtMaxBlocksPerJob);
            args.first_block[k] = blocks;
            blocks += d.blocks;
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
