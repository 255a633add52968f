// split.hip -- channelwise split: the split PLAN of a group of independent pairs, and the gather that applies it.
// Mirror of ppq/quantization/algorithm/equalization.py:200-290 (ChannelSplitHelper) and :361-393 (EqualizationPair.channel_split),
// which the reference runs as mask.tolist() and one torch op per CHANNEL of every tensor of the pair, then one torch.cat.
//
//   up / down = the keys of equalize_key.hpp (the ones equalization uses)        split[c] = up >= t && down >= t  (NaN: never)
//   d[c] = exclusive prefix sum of 1 + split[c]      src_of[d[c]] = c, and src_of[d[c] + 1] = c when split[c], both with bit 31 set
//   out[o, d, e] = x[o, src_of[d] & 0x7fffffff, e] (* 0.70710677f when bit 31 is set: ONE fp32 multiply, as torch's
//   `row * (1 / sqrt(2))` on a float32 tensor; an unsplit channel is copied bit for bit)
//
// The plan is two kernels: keys + mask with one workgroup per (job, channel), then the scan with one workgroup per job.  The mask
// of channel c waits in src_of[2 * c] -- the scan of a chunk of kBlock channels writes no further than src_of[2 * c + 1] of its
// last channel, so it never overwrites a mask it has not read: no scratch buffer, no atomics.
//
// Job tables: DESIGN.md, "Job tables".
#include "common.hpp"
#include "equalize_key.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

constexpr uint32_t kSplitBit = 0x80000000u;
constexpr float kInvSqrt2 = 0.70710677f;           // (float)(1 / sqrt(2)): what torch multiplies a float32 tensor by

// ------------------------------------------------------------------------------------ plan
constexpr int kSpMaxJobs = 32;                     // pairs per launch

struct SpPlanJob {                                 // 32 B
    uint32_t* src_of;
    int32_t* count;
    uint32_t C;
    float threshold;
    uint32_t seg_begin, seg_count;
};
struct SpPlanArgs {
    EqSeg segs[kEqMaxSegs];
    SpPlanJob jobs[kSpMaxJobs];
    uint32_t first_block[kSpMaxJobs];
    uint32_t count;
};
static_assert(sizeof(SpPlanArgs) <= 4096, "kernel arguments are limited to 4 KB");

// one workgroup per (job, channel): src_of[2 * c] = split[c]
__global__ __launch_bounds__(kBlock) void split_mask_kernel(const SpPlanArgs args) {
    __shared__ float lds[4 * (kBlock / kWave)];
    uint32_t c;
    const SpPlanJob& j = args.jobs[job_of(args, c)];
    float up, dn;
    eq_channel_keys(args.segs + j.seg_begin, j.seg_count, c, lds, up, dn);
    if (threadIdx.x == 0) j.src_of[2 * c] = (up >= j.threshold && dn >= j.threshold) ? 1u : 0u;     // a NaN key compares false
}

// one workgroup per job: chunks of kBlock channels in ascending order, the running total carried from chunk to chunk
__global__ __launch_bounds__(kBlock) void split_scan_kernel(const SpPlanArgs args) {
    __shared__ uint32_t wave_total[kBlock / kWave];
    const SpPlanJob& j = args.jobs[blockIdx.x];
    const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < j.C; base += kBlock) {
        const uint32_t c = base + threadIdx.x;
        const bool in = c < j.C;
        const uint32_t split = in ? j.src_of[2 * c] : 0u;
        const uint32_t width = in ? 1u + split : 0u;
        uint32_t incl = width;                                             // inclusive scan inside the wave
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            const uint32_t t = __shfl_up(incl, m, kWave);
            if (lane >= (uint32_t)m) incl += t;
        }
        if (lane == kWave - 1) wave_total[wid] = incl;
        __syncthreads();                                                   // every mask of the chunk is read; the wave totals are there
        uint32_t before = carry, chunk = 0;
        for (uint32_t w = 0; w < kBlock / kWave; w++) {
            const uint32_t t = wave_total[w];
            if (w < wid) before += t;
            chunk += t;
        }
        if (in) {
            const uint32_t d = before + incl - width;                      // <= 2 * c
            const uint32_t v = split ? (c | kSplitBit) : c;
            j.src_of[d] = v;
            if (split) j.src_of[d + 1] = v;
        }
        carry += chunk;
        __syncthreads();                                                   // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *j.count = (int32_t)carry;
}

int validate_plan(const ppqhip_split_plan_job* jobs, int num_jobs) {
    const char* what = "split_plan_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_split_plan_job& j = jobs[k];
        if (j.segments == nullptr || j.src_of == nullptr || j.count == nullptr || j.num_channel <= 0 || j.num_segments <= 0) {
            set_error("%s: job %d: null pointer, no channel or no segment", what, k); return PPQHIP_ERR_INVALID_VALUE;
        }
        if ((int64_t)j.num_channel * 2 > kEqMax) { set_error("%s: job %d: too many channels", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (int st = validate_segments(what, k, j.segments, j.num_segments, j.num_channel)) return st;
    }
    // the plans of one call are written while its segments are read: an output shares memory with nothing else of the call
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        outs.push_back(span_of(jobs[k].src_of, 2 * (int64_t)jobs[k].num_channel));
        outs.push_back(span_of(jobs[k].count, 1));
        for (int t = 0; t < jobs[k].num_segments; t++) ins.push_back(span_of(jobs[k].segments[t].base, jobs[k].segments[t].extent));
    }
    return check_overlap(what, ins, outs);
}

void launch_plan(const ppqhip_split_plan_job* jobs, int num_jobs, hipStream_t s) {
    for (int base = 0; base < num_jobs;) {
        SpPlanArgs args;
        uint32_t count = 0, segs = 0, blocks = 0;
        while (base + (int)count < num_jobs && count < (uint32_t)kSpMaxJobs &&
               segs + (uint32_t)jobs[base + count].num_segments <= (uint32_t)kEqMaxSegs) {
            const ppqhip_split_plan_job& src = jobs[base + count];
            SpPlanJob& d = args.jobs[count];
            d.src_of = reinterpret_cast<uint32_t*>(src.src_of); d.count = src.count;
            d.C = (uint32_t)src.num_channel; d.threshold = src.value_threshold;
            d.seg_begin = segs; d.seg_count = (uint32_t)src.num_segments;
            for (int t = 0; t < src.num_segments; t++) args.segs[segs++] = pack_segment(src.segments[t]);
            args.first_block[count] = blocks;
            blocks += d.C;
            count++;
        }
        for (uint32_t k = segs; k < (uint32_t)kEqMaxSegs; k++) args.segs[k] = args.segs[0];
        pad_job_table(args, count, blocks);
        hipLaunchKernelGGL(split_mask_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
        hipLaunchKernelGGL(split_scan_kernel, dim3(count), dim3(kBlock), 0, s, args);
        base += (int)count;
    }
}

// ------------------------------------------------------------------------------------ apply
constexpr int kSpApMaxJobs = 32;
constexpr uint32_t kSpApMaxBlocksPerJob = 1024;    // grid-strided beyond

struct SpApJob {                                   // 72 B
    const float* x;
    float* out;
    const uint32_t* src_of;
    uint32_t n_out, C;                             // n_out: output units -- float4 when vec, else floats
    FastDiv run, count;                            // run: units per (outer, channel) row
    uint32_t vec, blocks;
};
struct SpApArgs {
    SpApJob jobs[kSpApMaxJobs];
    uint32_t first_block[kSpApMaxJobs];
    uint32_t count;
};
static_assert(sizeof(SpApArgs) <= 4096, "kernel arguments are limited to 4 KB");

// the destination drives the loop: every output unit is written once
__global__ __launch_bounds__(kBlock) void split_apply_kernel(const SpApArgs args) {
    uint32_t local;
    const SpApJob& j = args.jobs[job_of(args, local)];
    const uint32_t stride = j.blocks * kBlock;
    const uint32_t first = local * kBlock + threadIdx.x;
    for (uint32_t i = first; i < j.n_out; i += stride) {
        const uint32_t row = fdiv(i, j.run), e = i - row * j.run.d;
        const uint32_t o = fdiv(row, j.count), d = row - o * j.count.d;    // d < count: inside the plan
        const uint32_t s = j.src_of[d];
        const uint32_t c = s & ~kSplitBit;
        if (c >= j.C) continue;                                            // a plan that is not one of ours reads nothing out of bounds
        const uint32_t from = (o * j.C + c) * j.run.d + e;                 // < the input's units <= 2^31 - 1
        if (j.vec) {
            float4 v = reinterpret_cast<const float4*>(j.x)[from];
            if (s & kSplitBit) { v.x = v.x * kInvSqrt2; v.y = v.y * kInvSqrt2; v.z = v.z * kInvSqrt2; v.w = v.w * kInvSqrt2; }
            reinterpret_cast<float4*>(j.out)[i] = v;
        } else {
            const float v = j.x[from];
            j.out[i] = (s & kSplitBit) ? v * kInvSqrt2 : v;
        }
    }
}

int validate_apply(const ppqhip_split_apply_job* jobs, int num_jobs) {
    const char* what = "split_apply_multi";
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_split_apply_job& j = jobs[k];
        if (j.x == nullptr || j.out == nullptr || j.src_of == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (j.n <= 0 || j.n > kEqMax || j.run <= 0 || j.run > j.n || j.num_channel <= 0 || j.num_channel > j.n ||      // both <= n < 2^31: the product fits
            j.n % ((int64_t)j.num_channel * j.run) != 0) {
            set_error("%s: job %d: bad geometry (n=%lld num_channel=%d run=%lld)", what, k, (long long)j.n, j.num_channel, (long long)j.run);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        if (j.count < j.num_channel || (int64_t)j.count > 2 * (int64_t)j.num_channel) {
            set_error("%s: job %d: count %d is outside [%d, %lld]", what, k, j.count, j.num_channel, 2 * (long long)j.num_channel);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        const int64_t n_out = j.n / j.num_channel * j.count;
        if (n_out > kEqMax) { set_error("%s: job %d writes %lld elements, more than 2^31 - 1", what, k, (long long)n_out); return PPQHIP_ERR_INVALID_VALUE; }
        ins.push_back(span_of(j.x, j.n));
        ins.push_back(span_of(j.src_of, j.count));
        outs.push_back(span_of(j.out, n_out));
    }
    return check_overlap(what, ins, outs);
}

void launch_apply(const ppqhip_split_apply_job* jobs, int num_jobs, hipStream_t s) {
    for (int base = 0; base < num_jobs; base += kSpApMaxJobs) {
        SpApArgs args;
        const int count = std::min(kSpApMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_split_apply_job& src = jobs[base + k];
            SpApJob& d = args.jobs[k];
            d.x = src.x; d.out = src.out; d.src_of = reinterpret_cast<const uint32_t*>(src.src_of);
            const bool vec = aligned16(src.x) && aligned16(src.out) && src.run % 4 == 0;
            const int64_t n_out = src.n / src.num_channel * src.count;
            d.vec = vec ? 1u : 0u;
            d.n_out = (uint32_t)(vec ? n_out >> 2 : n_out);
            d.C = (uint32_t)src.num_channel;
            d.run = make_fastdiv((uint32_t)(vec ? src.run / 4 : src.run));
            d.count = make_fastdiv((uint32_t)src.count);
            d.blocks = (uint32_t)std::min<uint64_t>(((uint64_t)d.n_out + kBlock - 1) / kBlock, kSpApMaxBlocksPerJob);
            args.first_block[k] = blocks;
            blocks += d.blocks;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        hipLaunchKernelGGL(split_apply_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_split_plan_multi(const ppqhip_split_plan_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_plan(jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        for (int t = 0; t < jobs[k].num_segments; t++)
            bytes += 4.0 * (double)jobs[k].num_channel * (double)(jobs[k].segments[t].outer * jobs[k].segments[t].run);
        bytes += 4.0 * (4.0 * (double)jobs[k].num_channel + 1.0);          // mask out and in, at most 2C plan entries, the count
    }
    LaunchScope scope(K_SPLIT_PLAN, bytes, s);
    launch_plan(jobs, num_jobs, s);
    return finish_launch("split_plan_multi");
}

int ppqhip_split_apply_multi(const ppqhip_split_apply_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_apply(jobs, num_jobs)) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++)                                     // every output element: one read, one write; the plan
        bytes += 8.0 * (double)(jobs[k].n / jobs[k].num_channel * jobs[k].count) + 4.0 * (double)jobs[k].count;
    LaunchScope scope(K_SPLIT_APPLY, bytes, s);
    launch_apply(jobs, num_jobs, s);
    return finish_launch("split_apply_multi");
}

}  // extern "C"
