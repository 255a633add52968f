// mx_roundtune.hip -- round tuning on the MX element grid for gfx950 (ppq_amd/mx_roundtune.py): per element
// the learned choice between the element value just below and just above the weight on its block's own grid, the block scale fixed.
//
//   split    once per weight: the block's code exactly as mx.hip makes it under the job's scale rule, then per element
//            u = v * 2^(127 - c), lo = mx_floor(|u|), hi = mx_up(lo); floored = (sign | lo) * X, rounding = (|u| - lo) / (hi - lo)
//            (0 where hi == lo: saturated), a NaN keeps its bits and gets rounding 0.  One read of w, one write of each output.
//   forward  once per training step: out = rounding > .5 ? (sign | mx_up(|floored / X|)) * X : floored -- element-wise, 8 B + 1/32 B
//            read and 4 B written per element, no cross-lane work.  Its backward is the identity (dy for floored, dy for rounding),
//            as for roundtune.hip: there is no backward kernel.
// Every step is exact in float32 (X and hi - lo are powers of two), so the torch restatement gives the same bits.
//
// The split needs the block amax (and the MSE sums): it walks through mx_walk.hpp as mx.hip does, so its codes are mx.hip's by
// construction; what is written here is rs_elem and the stores.  Weights are small, so a rows4 lane owns one float4 and nothing
// streams.  Job tables: DESIGN.md, "Job tables".
#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"
#include "mx_walk.hpp"

namespace ppqhip {
namespace {

constexpr int kMxRoundMaxJobs = 32;               // jobs of one launch of either kernel

struct RsJob {                                    // 104 B
    const float* w;
    float* floored;
    float* rounding;
    uint8_t* codes;
    MxWalk walk;
};
struct RsArgs {
    RsJob jobs[kMxRoundMaxJobs];
    uint32_t first_block[kMxRoundMaxJobs];
    uint32_t count;
};
static_assert(sizeof(RsArgs) <= 4096, "kernel arguments are limited to 4 KB");

struct RfJob {                                    // 96 B
    const float* floored;
    const float* rounding;
    const uint8_t* codes;
    float* out;
    uint32_t units;                               // lanes: float4 (vec) or elements
    uint32_t vec;                                 // inner == 1, axis_len % 4 == 0, all three float pointers 16-B aligned
    FastDiv plane;                                // axis_len * inner
    FastDiv inner;
    uint32_t nb;                                  // blocks per row
    MxFmt fmt;
};
struct RfArgs {
    RfJob jobs[kMxRoundMaxJobs];
    uint32_t first_block[kMxRoundMaxJobs];
    uint32_t count;
};
static_assert(sizeof(RfArgs) <= 4096, "kernel arguments are limited to 4 KB");

// ---- split ----------------------------------------------------------------------------------------------------------------------
struct RsElem { float floored, rounding; };
__device__ __forceinline__ RsElem rs_elem(float v, float inv, float X, const MxFmt& f) {
    const uint32_t bits = __float_as_uint(v * inv), sign = bits & 0x80000000u, mag = bits & 0x7fffffffu;
    const uint32_t lo = mx_floor(mag, f), hi = mx_up(lo, f);
    const bool nan = mag > 0x7f800000u, open = hi > lo && !nan;
    const float flo = __uint_as_float(lo);
    const float step = open ? __uint_as_float(hi) - flo : 1.0f;                 // a power of two
    RsElem r;
    r.floored = nan ? v : __uint_as_float(lo | sign) * X;
    r.rounding = open ? (__uint_as_float(mag) - flo) * (1.0f / step) : 0.0f;    // both exact; Inf has lo == hi
    return r;
}

template <int RULED>
__global__ __launch_bounds__(kBlock) void mx_round_split_kernel(const RsArgs args) {
    uint32_t local;
    const RsJob& j = args.jobs[job_of(args, local)];
    const MxWalk& walk = j.walk;
    const MxFmt f = walk.fmt;                                                    // by value, like the pointers: read once, ahead of every store
    float* const floored = j.floored;
    float* const rounding = j.rounding;
    uint8_t* const codes = j.codes;
    const auto mag = [](float v) { return mx_finite_mag(v); };
    if (walk.path == MX_ROWS4) {                                                 // workgroup-uniform
        mx_rows4<1, false, RULED>(walk, j.w, local, mag, [&](const MxRowPos& p, const float (&v)[4], uint32_t code) {
            const float X = mx_pow2(code), inv = mx_pow2(254u - code);
            const RsElem r0 = rs_elem(v[0], inv, X, f), r1 = rs_elem(v[1], inv, X, f), r2 = rs_elem(v[2], inv, X, f), r3 = rs_elem(v[3], inv, X, f);
            if (p.ok) {
                *reinterpret_cast<float4*>(floored + p.at) = make_float4(r0.floored, r1.floored, r2.floored, r3.floored);
                *reinterpret_cast<float4*>(rounding + p.at) = make_float4(r0.rounding, r1.rounding, r2.rounding, r3.rounding);
            }
            if (p.in && p.q == 0) codes[p.g] = (uint8_t)code;
        });
    } else if (walk.path == MX_ROWS1) {
        mx_rows1<RULED>(walk, j.w, local, mag, [&](const MxRowPos& p, const float (&v)[1], uint32_t code) {
            const RsElem r = rs_elem(v[0], mx_pow2(254u - code), mx_pow2(code), f);
            if (p.ok) { floored[p.at] = r.floored; rounding[p.at] = r.rounding; }
            if (p.in && p.q == 0) codes[p.g] = (uint8_t)code;
        });
    } else {
        mx_strided<RULED>(walk, j.w, local, mag, [&](const MxStridedPos& p, const float (&v)[kMxBlock], uint32_t code) {
            const float X = mx_pow2(code), inv = mx_pow2(254u - code);
#pragma unroll
            for (uint32_t t = 0; t < kMxBlock; t++) {
                if (t < p.blen) {
                    const RsElem r = rs_elem(v[t], inv, X, f);
                    floored[p.base + t * p.step] = r.floored;
                    rounding[p.base + t * p.step] = r.rounding;
                }
            }
            codes[p.w] = (uint8_t)code;
        });
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rf_elem(float fl, float r, uint32_t code, const MxFmt& f) {
    const uint32_t c = min(code, 254u);
    const float X = mx_pow2(c), inv = mx_pow2(254u - c);
    const uint32_t bits = __float_as_uint(fl * inv), sign = bits & 0x80000000u, mag = bits & 0x7fffffffu;
    const float up = __uint_as_float(mx_up(mag, f) | sign) * X;
    return (r > 0.5f && mag <= 0x7f800000u && code != 0xffu) ? up : fl;         // r NaN compares false
}

__global__ __launch_bounds__(kBlock) void mx_round_fwd_kernel(const RfArgs args) {
    uint32_t local;
    const RfJob& j = args.jobs[job_of(args, local)];
    const uint32_t t = local * kBlock + threadIdx.x;
    if (t >= j.units) return;
    const uint32_t e = j.vec ? t * 4u : t;                                       // first element of this lane
    const uint32_t o = fdiv(e, j.plane), rem = e - o * j.plane.d;
    const uint32_t a = fdiv(rem, j.inner), i = rem - a * j.inner.d;
    const uint8_t* cp = j.codes + ((size_t)o * j.nb + (a >> 5)) * j.inner.d + i;
    if (j.vec) {                                                                 // workgroup-uniform; a float4 lies inside one block
        const float4 fl = reinterpret_cast<const float4*>(j.floored)[t], r = reinterpret_cast<const float4*>(j.rounding)[t];
        const uint32_t code = *cp;
        reinterpret_cast<float4*>(j.out)[t] = make_float4(rf_elem(fl.x, r.x, code, j.fmt), rf_elem(fl.y, r.y, code, j.fmt),
                                                          rf_elem(fl.z, r.z, code, j.fmt), rf_elem(fl.w, r.w, code, j.fmt));
    } else {
        const float fl = j.floored[t], r = j.rounding[t];
        const uint32_t code = *cp;
        j.out[t] = rf_elem(fl, r, code, j.fmt);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int validate_split(const char* what, const ppqhip_mx_round_split_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_mx_round_split_job& j = jobs[k];
        const MxGeometry g = mx_geometry_of(j);
        if (int st = check_mx_job(what, k, j.format, true, g)) return st;
        if (g.empty()) continue;
        if (!j.w || !j.floored || !j.rounding || !j.scale_codes) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!aligned4(j.w) || !aligned4(j.floored) || !aligned4(j.rounding)) { set_error("%s: job %d: a float pointer is not 4-byte aligned", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        ins.push_back(span_of(j.w, g.elems()));
        outs.push_back(span_of(j.floored, g.elems()));
        outs.push_back(span_of(j.rounding, g.elems()));
        outs.push_back(span_of(j.scale_codes, g.codes()));
    }
    return check_overlap(what, ins, outs);
}

int validate_fwd(const char* what, const ppqhip_mx_round_fwd_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_mx_round_fwd_job& j = jobs[k];
        if (j.format < 0 || (j.format >> PPQHIP_MX_RULE_SHIFT) != 0) { set_error("%s: job %d: format %d carries a scale rule, but the codes are given", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
        const MxGeometry g = mx_geometry_of(j);
        if (int st = check_mx_job(what, k, j.format, false, g)) return st;
        if (g.empty()) continue;
        if (!j.floored || !j.rounding || !j.scale_codes || !j.out) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!aligned4(j.floored) || !aligned4(j.rounding) || !aligned4(j.out)) { set_error("%s: job %d: a float pointer is not 4-byte aligned", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        ins.push_back(span_of(j.floored, g.elems()));
        ins.push_back(span_of(j.rounding, g.elems()));
        ins.push_back(span_of(j.scale_codes, g.codes()));
        outs.push_back(span_of(j.out, g.elems()));
    }
    return check_overlap(what, ins, outs);
}

// the device job and its workgroups
uint32_t split_job(const ppqhip_mx_round_split_job& src, RsJob* d, int* ruled) {
    d->w = src.w; d->floored = src.floored; d->rounding = src.rounding; d->codes = src.scale_codes;
    return fill_mx_walk(&d->walk, mx_geometry_of(src), src.format, aligned16(src.w) && aligned16(src.floored) && aligned16(src.rounding), 1, ruled);
}

uint32_t fwd_job(const ppqhip_mx_round_fwd_job& src, RfJob* d, int*) {
    d->floored = src.floored; d->rounding = src.rounding; d->codes = src.scale_codes; d->out = src.out;
    const MxGeometry g = mx_geometry_of(src);
    d->vec = (src.inner == 1 && src.axis_len % 4 == 0 && aligned16(src.floored) && aligned16(src.rounding) && aligned16(src.out)) ? 1u : 0u;
    d->units = (uint32_t)(d->vec ? g.elems() / 4 : g.elems());
    d->plane = make_fastdiv((uint32_t)(src.axis_len * src.inner));
    d->inner = make_fastdiv((uint32_t)src.inner);
    d->nb = (uint32_t)g.nb();
    make_mx_fmt(src.format, &d->fmt);
    return (uint32_t)(((int64_t)d->units + kBlock - 1) / kBlock);
}

// both directions move 12 B per element and one code per block: w in and floored, rounding, codes out; floored, rounding, codes in and out
template <typename Job>
double live_bytes(const std::vector<const Job*>& live) {
    double bytes = 0.0;
    for (const Job* j : live) bytes += 12.0 * (double)mx_geometry_of(*j).elems() + (double)mx_geometry_of(*j).codes();
    return bytes;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_mx_round_split_multi(const ppqhip_mx_round_split_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_split("mx_round_split_multi", jobs, num_jobs)) return st;
    const auto live = live_mx_jobs(jobs, num_jobs);
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_ROUND_SPLIT, live_bytes(live), s);
    return launch_mx_jobs<RsArgs>("mx_round_split_multi", live, split_job, [&](int ruled, uint32_t blocks, const RsArgs& args) {
        with_mx_ruled(ruled, [&](auto R) { hipLaunchKernelGGL(mx_round_split_kernel<decltype(R)::value>, dim3(blocks), dim3(kBlock), 0, s, args); });
    });
}

int ppqhip_mx_round_fwd_multi(const ppqhip_mx_round_fwd_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_fwd("mx_round_fwd_multi", jobs, num_jobs)) return st;
    const auto live = live_mx_jobs(jobs, num_jobs);
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_ROUND_FWD, live_bytes(live), s);
    return launch_mx_jobs<RfArgs>("mx_round_fwd_multi", live, fwd_job, [&](int, uint32_t blocks, const RfArgs& args) {
        hipLaunchKernelGGL(mx_round_fwd_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    });
}

}  // extern "C"
