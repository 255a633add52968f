// mx.hip -- OCP Microscaling (MX) block-scaled fake-quant for gfx950: MXFP8 (E4M3 / E5M2), MXFP6 (E3M2 / E2M3), MXFP4 (E2M1), MXINT8.
//
// The reference has no MX; the contract is DESIGN.md section 9 and tests/mx_reference.py.  A tensor is addressed as
// [outer, axis_len, inner]; a block is up to 32 consecutive elements along the middle axis (the last block of an axis may be short):
//   amax = max |v| over the block's FINITE elements          code = max(biased_exponent(amax) - emax, 0)      X = 2^(code - 127)
//   y = cast(v / X) * X      cast: nearest representable element value, ties to the even encoding, saturating at the largest normal
//   NaN passes through bit for bit; +-Inf saturates; zero keeps its sign; float32 subnormals are inputs and outputs like any other.
// X and 1 / X are powers of two inside float32's range (2^-127 is a subnormal), so v / X is v * (1 / X), exact whenever the product is
// a normal number -- a product that lands among float32's subnormals is far below half the smallest element value and casts to zero
// whichever way it was rounded -- and cast(u) * X is always representable: every step is exact, the function is deterministic.
//
// ONE kernel (job table in the kernel arguments, DESIGN.md "Job tables"; the single-tensor entry point is a table of one job) over
// the three addressings of mx_walk.hpp, which loads the block, reduces its amax and takes its code; what is written here is the
// cast of the elements and the stores.  Each element is read once and written once; the block's values wait in registers between
// the max and the cast.  The description of a format, the scale code and the rounding of an element live in mx_common.hpp.
// The code above is the floor rule's; a job may ask for another scale rule (CEIL, EVEN, MSE: DESIGN.md section 9.17), which travels
// above the format id and is a workgroup-uniform choice in instantiations of their own -- still one launch, one read and one write
// per element: under MSE the block's values wait in registers through two more casts and two float64 sums.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"
#include "mx_walk.hpp"

namespace ppqhip {
namespace {

struct MxJob {                                    // 96 B
    const float* x;
    float* y;
    uint8_t* codes;                               // E8M0 scale codes, one per block, or null
    MxWalk walk;
};
template <int CAP>
struct MxArgs {
    MxJob jobs[CAP];
    uint32_t first_block[CAP];
    uint32_t count;
};
static_assert(sizeof(MxArgs<kMxMaxJobs>) <= 4096, "kernel arguments are limited to 4 KB");

// RULED (MX_PLAIN / MX_AMAX_RULES / MX_SEARCH, mx_common.hpp): the instantiations above MX_PLAIN take the block's code from the job's
// scale rule.  The plain ones are the floor rule's and keep their code; a launch whose jobs are all FLOOR
// runs those.
template <int CAP, int U, bool NT, int RULED>
__global__ __launch_bounds__(kBlock) void mx_fq_kernel(const MxArgs<CAP> args) {
    uint32_t local;
    const MxJob& j = args.jobs[job_of(args, local)];
    const MxWalk& walk = j.walk;
    const MxFmt f = walk.fmt;                                                    // by value, like the pointers: read once, ahead of every store
    float* const y = j.y;
    uint8_t* const codes = j.codes;
    const auto mag = [](float v) { return mx_finite_mag(v); };
    if (walk.path == MX_ROWS4) {                                                 // workgroup-uniform
        mx_rows4<U, NT, RULED>(walk, j.x, local, mag, [&](const MxRowPos& p, const float (&v)[4], uint32_t code) {
            const float X = mx_pow2(code), inv = mx_pow2(254u - code);
            const float4 r = make_float4(mx_elem(v[0], inv, X, f), mx_elem(v[1], inv, X, f), mx_elem(v[2], inv, X, f), mx_elem(v[3], inv, X, f));
            if (p.ok) *reinterpret_cast<float4*>(y + p.at) = r;
            if (p.in && p.q == 0 && codes != nullptr) codes[p.g] = (uint8_t)code;
        });
    } else if (walk.path == MX_ROWS1) {
        mx_rows1<RULED>(walk, j.x, local, mag, [&](const MxRowPos& p, const float (&v)[1], uint32_t code) {
            const float r = mx_elem(v[0], mx_pow2(254u - code), mx_pow2(code), f);
            if (p.ok) y[p.at] = r;
            if (p.in && p.q == 0 && codes != nullptr) codes[p.g] = (uint8_t)code;
        });
    } else {
        mx_strided<RULED>(walk, j.x, local, mag, [&](const MxStridedPos& p, const float (&v)[kMxBlock], uint32_t code) {
            const float X = mx_pow2(code), inv = mx_pow2(254u - code);
#pragma unroll
            for (uint32_t t = 0; t < kMxBlock; t++)
                if (t < p.blen) y[p.base + t * p.step] = mx_elem(v[t], inv, X, f);
            if (codes != nullptr) codes[p.w] = (uint8_t)code;
        });
    }
}

template <int CAP, int U, bool NT>
void launch_fq(int ruled, uint32_t blocks, hipStream_t s, const MxArgs<CAP>& args) {
    with_mx_ruled(ruled, [&](auto R) { hipLaunchKernelGGL((mx_fq_kernel<CAP, U, NT, decltype(R)::value>), dim3(blocks), dim3(kBlock), 0, s, args); });
}

// An output shares memory with no other tensor of the call, with one exception: y == x, a tensor quantised in place (a block is read
// whole before any of it is written, and blocks are disjoint).
int validate(const char* what, const ppqhip_mx_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_mx_job& j = jobs[k];
        const MxGeometry g = mx_geometry_of(j);
        if (int st = check_mx_job(what, k, j.format, true, g)) return st;
        if (g.empty()) continue;
        if (j.x == nullptr || j.y == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if ((const float*)j.y != j.x) ins.push_back(span_of(j.x, g.elems()));
        outs.push_back(span_of(j.y, g.elems()));
        if (j.scale_codes != nullptr) outs.push_back(span_of(j.scale_codes, g.codes()));
    }
    return check_overlap(what, ins, outs);
}

// the device job and the workgroups it takes when a rows4 lane owns U float4
uint32_t device_job(const ppqhip_mx_job& src, int U, MxJob* d, int* ruled) {
    d->x = src.x; d->y = src.y; d->codes = src.scale_codes;
    return fill_mx_walk(&d->walk, mx_geometry_of(src), src.format, aligned16(src.x) && aligned16(src.y), U, ruled);
}

constexpr int64_t kMxStreamElems = 48ll << 20;    // >= 192 MiB: streaming loads (see fq_walk.hpp)
constexpr int64_t kMxSmallElems = 4ll << 20;      // latency-bound tensors: one float4 per lane (see fq_walk.hpp)

double job_bytes(const ppqhip_mx_job& j) {
    const MxGeometry g = mx_geometry_of(j);
    return 8.0 * (double)g.outer * (double)g.axis_len * (double)g.inner + (j.scale_codes != nullptr ? (double)g.codes() : 0.0);
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_mx_fq(const float* x, float* y, uint8_t* scale_codes, int64_t outer, int64_t axis_len, int64_t inner, int format,
                 void* stream) {
    ppqhip_mx_job job;
    job.x = x; job.y = y; job.scale_codes = scale_codes;
    job.outer = outer; job.axis_len = axis_len; job.inner = inner; job.format = format; job.reserved = 0;
    if (int st = validate("mx_fq", &job, 1)) return st;
    const auto live = live_mx_jobs(&job, 1);
    if (live.empty()) return PPQHIP_OK;
    const int64_t n = outer * axis_len * inner;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_FQ, job_bytes(job), s);
    const int U = n <= kMxSmallElems ? 1 : 2;
    return launch_mx_jobs<MxArgs<1>>("mx_fq", live,
        [&](const ppqhip_mx_job& src, MxJob* d, int* ruled) { return device_job(src, U, d, ruled); },
        [&](int ruled, uint32_t blocks, const MxArgs<1>& args) {
            if (n >= kMxStreamElems) launch_fq<1, 2, true>(ruled, blocks, s, args);
            else if (U == 2) launch_fq<1, 2, false>(ruled, blocks, s, args);
            else launch_fq<1, 1, false>(ruled, blocks, s, args);
        });
}

int ppqhip_mx_fq_multi(const ppqhip_mx_job* jobs, int num_jobs, void* stream) {
    if (int st = validate("mx_fq_multi", jobs, num_jobs)) return st;
    const auto live = live_mx_jobs(jobs, num_jobs);
    if (live.empty()) return PPQHIP_OK;
    double bytes = 0.0;
    for (const ppqhip_mx_job* j : live) bytes += job_bytes(*j);
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_FQ, bytes, s);
    return launch_mx_jobs<MxArgs<kMxMaxJobs>>("mx_fq_multi", live,
        [](const ppqhip_mx_job& src, MxJob* d, int* ruled) { return device_job(src, 1, d, ruled); },
        [&](int ruled, uint32_t blocks, const MxArgs<kMxMaxJobs>& args) { launch_fq<kMxMaxJobs, 1, false>(ruled, blocks, s, args); });
}

}  // extern "C"
