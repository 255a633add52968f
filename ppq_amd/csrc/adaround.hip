// adaround.hip -- AdaRound's soft-rounded fake quant (forward) and its V gradient (backward), every weight of a block in ONE
// launch each.  Mirror of ppq/quantization/optim/legacy.py:122-132 (AdaRoundDelegator.__call__) and of the gradient torch's
// autograd takes through it; the regulariser of legacy.py:58-64 is fused into the backward launch.
//
// Bitwise the torch sequence (fp32, -ffp-contract=off, Makefile), op for op, with the Python scalars as torch casts them
// (zeta - gamma = 1.2000000000000002 -> 1.2f, gamma -> -0.1f):
//   f = floor(w / s)  (IEEE quotient)      sg = 1 / (1 + exp(-v))  (torch.sigmoid)      a = sg * 1.2f + -0.1f  (two roundings)
//   h = clamp(a, 0, 1)      t = (f + h) + o      out = (clamp(t, qmin, qmax) - o) * s
// clamp is torch's `isnan(v) ? v : min(max(v, lo), hi)`: NaN in, NaN out.
// Backward (dV only; W and the scale are in no optimizer, legacy.py:224-236):
//   g = dy * s;  g = qmin <= t <= qmax ? g : +0;  g = 0 <= a <= 1 ? g : +0;  dv = ((g * 1.2f) * (1 - sg)) * sg
// Regulariser (reg = device {k, beta, beta - 1}, k = gamma * alpha as autograd rounds it; k == 0: the term is the integer 0 of
// legacy.py:59-60 and NOTHING is added -- `+ 0.0f` would turn a -0.0 gradient into +0.0):
//   r = -k;  x = |h - 0.5| * 2;  r = r * (beta * pow(x, beta - 1));  r = r * 2;  r = r * sgn(h - 0.5);  mask on a;  r = r * 1.2f;
//   r = (r * (1 - sg)) * sg;  dv = dv + r
//
// Job table: DESIGN.md, "Job tables" (capturable into a HIP graph).  Geometry and walk: channel_axis.hpp (a per-tensor job has
// num_channel = 1); 16-B loads and stores where every pointer of the job is aligned.  No atomics, no reductions.
#include "channel_axis.hpp"
#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

constexpr int kArMaxJobs = 16;                     // 16 x 96 B of job table: well inside the 4 KB of kernel arguments

struct ArJob {                                     // 96 B
    const float* w;
    const float* v;
    const float* scale;
    const float* offset;
    float* out;                                    // forward: fake-quantised weight; backward: dV
    const float* dy;                               // backward only
    ChannelAxisMap map;
    float qmin, qmax;
};
struct ArArgs {
    ArJob jobs[kArMaxJobs];
    uint32_t first_block[kArMaxJobs];
    uint32_t count;
    const float* reg;                              // backward: {k, beta, beta - 1}
};
static_assert(sizeof(ArArgs) <= 4096, "kernel arguments are limited to 4 KB");

struct ArElem {
    float sg, a, t;
};

// the forward chain of one element; returns the fake-quantised value
__device__ __forceinline__ float ar_forward(float w, float v, float s, float o, float qmin, float qmax, ArElem& e) {
    const float f = __builtin_floorf(w / s);
    e.sg = 1.0f / (1.0f + expf(-v));
    const float m = e.sg * 1.2f;
    e.a = m + (-0.1f);
    const float h = clamp_nan(e.a, 0.0f, 1.0f);
    const float u = f + h;
    e.t = u + o;
    const float c = clamp_nan(e.t, qmin, qmax);
    return (c - o) * s;
}

template <bool REG>
__device__ __forceinline__ float ar_backward(float w, float v, float s, float o, float qmin, float qmax, float dy, float k,
                                             float beta, float bm1) {
    ArElem e;
    (void)ar_forward(w, v, s, o, qmin, qmax, e);
    const bool in_a = (e.a >= 0.0f) && (e.a <= 1.0f);
    float g = dy * s;
    g = (e.t >= qmin && e.t <= qmax) ? g : 0.0f;
    g = in_a ? g : 0.0f;
    const float one_m = 1.0f - e.sg;
    float dv = ((g * 1.2f) * one_m) * e.sg;
    if (REG) {
        const float h = clamp_nan(e.a, 0.0f, 1.0f);
        const float d = h - 0.5f;
        const float x = __builtin_fabsf(d) * 2.0f;
        const float p = powf(x, bm1);
        float r = -k;
        r = r * (beta * p);
        r = r * 2.0f;
        r = r * (float)((0.0f < d) - (d < 0.0f));
        r = in_a ? r : 0.0f;
        r = r * 1.2f;
        r = (r * one_m) * e.sg;
        dv = dv + r;
    }
    return dv;
}

template <bool BWD, bool REG>
__device__ __forceinline__ void ar_job(const ArJob& j, uint32_t local, float k, float beta, float bm1) {
    const float4* w4 = reinterpret_cast<const float4*>(j.w);
    const float4* v4 = reinterpret_cast<const float4*>(j.v);
    const float4* d4 = reinterpret_cast<const float4*>(j.dy);
    float4* o4 = reinterpret_cast<float4*>(j.out);
    auto one = [&](float w, float v, float dy, uint32_t c) {
        const float s = j.scale[c], o = j.offset[c];
        if (BWD) return ar_backward<REG>(w, v, s, o, j.qmin, j.qmax, dy, k, beta, bm1);
        ArElem e;
        return ar_forward(w, v, s, o, j.qmin, j.qmax, e);
    };
    walk_channel_axis(j.map, local,
                      [&](uint32_t i, uint32_t c) { j.out[i] = one(j.w[i], j.v[i], BWD ? j.dy[i] : 0.f, c); },
                      [&](uint32_t q) {
                          const float4 w = w4[q], v = v4[q];
                          float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                          if (BWD) dy = d4[q];
                          const Channels4 c = channels_of_float4(j.map, q);             // behind the loads: channel_axis.hpp
                          o4[q] = make_float4(one(w.x, v.x, dy.x, c.c0), one(w.y, v.y, dy.y, c.c1), one(w.z, v.z, dy.z, c.c2),
                                              one(w.w, v.w, dy.w, c.c3));
                      });
}

__global__ __launch_bounds__(kBlock) void adaround_fwd_kernel(const ArArgs args) {
    uint32_t local;
    const uint32_t jk = job_of(args, local);
    ar_job<false, false>(args.jobs[jk], local, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(kBlock) void adaround_bwd_kernel(const ArArgs args) {
    uint32_t local;
    const ArJob& j = args.jobs[job_of(args, local)];
    // every lane reads the same three floats: the branch on k is wave-uniform
    const float k = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, args.reg[0])));
    if (k == 0.0f) { ar_job<true, false>(j, local, 0.f, 0.f, 0.f); return; }
    ar_job<true, true>(j, local, k, args.reg[1], args.reg[2]);
}

int validate_jobs(const ppqhip_adaround_job* jobs, int num_jobs, bool bwd, const char* what) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_adaround_job& j = jobs[k];
        if (int st = validate_channel_axis(what, j.n, j.num_channel, j.elem_per_channel, k)) return st;
        if (!j.w || !j.v || !j.scale || !j.offset || !j.out || (bwd && !j.dy)) {
            set_error("%s: job %d has a null pointer", what, k);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        if (j.qmin > j.qmax) { set_error("%s: job %d: quant_min > quant_max", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    }
    return PPQHIP_OK;
}

int launch_adaround(const ppqhip_adaround_job* jobs, int num_jobs, bool bwd, const float* reg, hipStream_t s) {
    for (int base = 0; base < num_jobs; base += kArMaxJobs) {
        ArArgs args;
        const int count = min(kArMaxJobs, num_jobs - base);
        uint32_t blocks = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_adaround_job& src = jobs[base + k];
            ArJob& d = args.jobs[k];
            d.w = src.w; d.v = src.v; d.scale = src.scale; d.offset = src.offset; d.out = src.out; d.dy = src.dy;
            const bool aligned = aligned16(src.w) && aligned16(src.v) && aligned16(src.out) && (!bwd || aligned16(src.dy));
            d.map = pack_channel_axis(aligned, src.n, src.num_channel, src.elem_per_channel);
            d.qmin = (float)src.qmin; d.qmax = (float)src.qmax;
            args.first_block[k] = blocks;
            blocks += d.map.blocks;
        }
        pad_job_table(args, (uint32_t)count, blocks);
        args.reg = reg;
        if (bwd) hipLaunchKernelGGL(adaround_bwd_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
        else hipLaunchKernelGGL(adaround_fwd_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
    return PPQHIP_OK;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_adaround_fwd_multi(const ppqhip_adaround_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_jobs(jobs, num_jobs, false, "adaround_fwd_multi")) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) bytes += 12.0 * (double)jobs[k].n;          // w, v in; out
    LaunchScope scope(K_ADAROUND_FWD, bytes, s);
    launch_adaround(jobs, num_jobs, false, nullptr, s);
    return finish_launch("adaround_fwd_multi");
}

int ppqhip_adaround_bwd_multi(const ppqhip_adaround_job* jobs, int num_jobs, const float* reg, void* stream) {
    if (int st = validate_jobs(jobs, num_jobs, true, "adaround_bwd_multi")) return st;
    if (num_jobs == 0) return PPQHIP_OK;
    if (!reg) { set_error("adaround_bwd_multi: reg is null"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) bytes += 16.0 * (double)jobs[k].n;          // w, v, dy in; dv
    LaunchScope scope(K_ADAROUND_BWD, bytes, s);
    launch_adaround(jobs, num_jobs, true, reg, s);
    return finish_launch("adaround_bwd_multi");
}

}  // extern "C"
