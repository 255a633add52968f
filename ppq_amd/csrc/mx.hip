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
// (The split of round tuning, mx_roundtune.hip, repeats these three bodies with its own stores: its codes must stay these bit for
// bit, so a change to the addressing, the reductions or the order of the MSE adds here is made there too.)
// Three bodies behind ONE kernel (job table in the kernel arguments, DESIGN.md "Job tables"; the single-tensor entry point is a table
// of one job).  Each reads every element once and writes it once; the block's values wait in registers between the max and the cast:
//   rows4   inner == 1, 16-B aligned, axis_len % 4 == 0: a block is 128 B, eight lanes load one float4 each (a short last block
//           switches whole lanes off), integer max over the magnitudes with three shuffles inside the eight lanes
//   rows1   inner == 1 otherwise: one element per lane, 32 lanes per block, five shuffles -- the same arithmetic
//   strided inner > 1: one lane per (outer, block, inner) triple, numbered with inner fastest, so that each of the 32 loads of a
//           wave is coalesced along inner and a wave stays full when inner is small (9 for a 3x3 weight)
// The description of a format, the scale code and the rounding of an element live in mx_common.hpp, shared with mx_pack.hip.
// The code above is the floor rule's; a job may ask for another scale rule (CEIL, EVEN, MSE: DESIGN.md section 9.17), which travels
// above the format id and is a workgroup-uniform choice in instantiations of their own -- still one launch, one read and one write
// per element: under MSE the block's values wait in registers through two more casts and two float64 sums.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"

namespace ppqhip {
namespace {

enum : uint32_t { MX_ROWS4 = 0, MX_ROWS1 = 1, MX_STRIDED = 2 };

struct MxJob {                                    // 96 B
    const float* x;
    float* y;
    uint8_t* codes;                               // E8M0 scale codes, one per block, or null
    uint32_t len;                                 // axis_len
    uint32_t units;                               // rows4 / rows1: outer * blocks per row; strided: outer * blocks per row * inner
    FastDiv nb;                                   // blocks per row
    FastDiv inner;
    uint32_t path;
    MxFmt fmt;
    uint32_t rule;                                // PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE: read by the RULED instantiations only
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
template <int U, bool NT, int RULED>
__device__ __forceinline__ void mx_rows4(const MxJob& j, uint32_t local) {
    constexpr uint32_t kGroups = kBlock / 8;                                     // blocks per workgroup and step
    const uint32_t q = threadIdx.x & 7u;
    float4 a[U];
    uint32_t g[U];
    size_t at[U];
    bool in[U], ok[U];
#pragma unroll
    for (int k = 0; k < U; k++) {                                                // clamped, branch-free: all U loads issue back to back
        const uint32_t want = (local * U + k) * kGroups + (threadIdx.x >> 3);
        in[k] = want < j.units;
        g[k] = min(want, j.units - 1);
        const uint32_t row = fdiv(g[k], j.nb), b = g[k] - row * j.nb.d;
        const uint32_t e = b * kMxBlock + q * 4;
        ok[k] = in[k] && e < j.len;                                              // len % 4 == 0: a float4 is inside the row or outside
        at[k] = (size_t)row * j.len + (e < j.len ? e : b * kMxBlock);
        a[k] = load4<NT>(reinterpret_cast<const float4*>(j.x + at[k]));
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
        uint32_t m = max(max(mx_finite_mag(a[k].x), mx_finite_mag(a[k].y)), max(mx_finite_mag(a[k].z), mx_finite_mag(a[k].w)));
        m = ok[k] ? m : 0u;
        m = max(m, (uint32_t)__shfl_xor((int)m, 4, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
        uint32_t code = mx_code(m, j.fmt);
        if constexpr (RULED != MX_PLAIN) {
            code = mx_rule_code(m, j.fmt, j.rule);
            if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {              // workgroup-uniform
                MxMse s(code);
                s.add(a[k].x, ok[k], j.fmt); s.add(a[k].y, ok[k], j.fmt); s.add(a[k].z, ok[k], j.fmt); s.add(a[k].w, ok[k], j.fmt);
                s.reduce<8>();
                code = s.code();
            }
        }
        const float X = mx_pow2(code), inv = mx_pow2(254u - code);
        float4 r;
        r.x = mx_elem(a[k].x, inv, X, j.fmt); r.y = mx_elem(a[k].y, inv, X, j.fmt);
        r.z = mx_elem(a[k].z, inv, X, j.fmt); r.w = mx_elem(a[k].w, inv, X, j.fmt);
        if (ok[k]) *reinterpret_cast<float4*>(j.y + at[k]) = r;
        if (in[k] && q == 0 && j.codes != nullptr) j.codes[g[k]] = (uint8_t)code;
    }
}

template <int RULED>
__device__ __forceinline__ void mx_rows1(const MxJob& j, uint32_t local) {
    const uint32_t q = threadIdx.x & 31u;
    const uint32_t want = local * (kBlock / kMxBlock) + (threadIdx.x >> 5);
    const bool in = want < j.units;
    const uint32_t g = min(want, j.units - 1);
    const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + q;
    const bool ok = in && e < j.len;
    const size_t at = (size_t)row * j.len + (e < j.len ? e : b * kMxBlock);
    const float v = j.x[at];
    uint32_t m = ok ? mx_finite_mag(v) : 0u;
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    uint32_t code = mx_code(m, j.fmt);
    if constexpr (RULED != MX_PLAIN) {
        code = mx_rule_code(m, j.fmt, j.rule);
        if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {
            MxMse s(code);
            s.add(v, ok, j.fmt);
            s.reduce<32>();
            code = s.code();
        }
    }
    const float r = mx_elem(v, mx_pow2(254u - code), mx_pow2(code), j.fmt);
    if (ok) j.y[at] = r;
    if (in && q == 0 && j.codes != nullptr) j.codes[g] = (uint8_t)code;
}

template <int RULED>
__device__ __forceinline__ void mx_strided(const MxJob& j, uint32_t local) {
    const uint32_t want = local * kBlock + threadIdx.x;
    const bool in = want < j.units;
    const uint32_t w = min(want, j.units - 1);
    const uint32_t blk = fdiv(w, j.inner), i = w - blk * j.inner.d;
    const uint32_t o = fdiv(blk, j.nb), b = blk - o * j.nb.d;
    const uint32_t blen = min(kMxBlock, j.len - b * kMxBlock);                   // >= 1
    const size_t base = ((size_t)o * j.len + (size_t)b * kMxBlock) * j.inner.d + i;
    const size_t step = j.inner.d;
    float v[kMxBlock];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) v[t] = j.x[base + min(t, blen - 1) * step];      // clamped: 32 loads in flight
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) m = max(m, t < blen ? mx_finite_mag(v[t]) : 0u);
    uint32_t code = mx_code(m, j.fmt);
    if constexpr (RULED != MX_PLAIN) {
        code = mx_rule_code(m, j.fmt, j.rule);
        if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {
            MxMse s(code);
#pragma unroll
            for (uint32_t t = 0; t < kMxBlock; t++) s.add(v[t], t < blen, j.fmt);
            code = s.code();
        }
    }
    const float X = mx_pow2(code), inv = mx_pow2(254u - code);
    if (!in) return;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++)
        if (t < blen) j.y[base + t * step] = mx_elem(v[t], inv, X, j.fmt);
    if (j.codes != nullptr) j.codes[w] = (uint8_t)code;
}

template <int CAP, int U, bool NT, int RULED>
__global__ __launch_bounds__(kBlock) void mx_fq_kernel(const MxArgs<CAP> args) {
    uint32_t local;
    const MxJob& j = args.jobs[job_of(args, local)];
    if (j.path == MX_ROWS4) mx_rows4<U, NT, RULED>(j, local);                    // workgroup-uniform
    else if (j.path == MX_ROWS1) mx_rows1<RULED>(j, local);
    else mx_strided<RULED>(j, local);
}

template <int CAP, int U, bool NT>
void launch_fq(int ruled, uint32_t blocks, hipStream_t s, const MxArgs<CAP>& args) {
    if (ruled == MX_SEARCH) hipLaunchKernelGGL((mx_fq_kernel<CAP, U, NT, MX_SEARCH>), dim3(blocks), dim3(kBlock), 0, s, args);
    else if (ruled == MX_AMAX_RULES) hipLaunchKernelGGL((mx_fq_kernel<CAP, U, NT, MX_AMAX_RULES>), dim3(blocks), dim3(kBlock), 0, s, args);
    else hipLaunchKernelGGL((mx_fq_kernel<CAP, U, NT, MX_PLAIN>), dim3(blocks), dim3(kBlock), 0, s, args);
}

// the checks of one job; *n = its elements (0: nothing to do)
int validate_job(const char* what, int k, const ppqhip_mx_job& j, int64_t* n) {
    MxFmt probe;
    int fmt;
    uint32_t rule;
    if (!split_mx_format(j.format, &fmt, &rule)) { set_error("%s: job %d: unknown MX scale rule in format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
    if (!make_mx_fmt(fmt, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, fmt); return PPQHIP_ERR_INVALID_VALUE; }
    if (j.outer < 0 || j.axis_len < 0 || j.inner < 0) { set_error("%s: job %d: negative size", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    *n = 0;
    if (j.outer == 0 || j.axis_len == 0 || j.inner == 0) return PPQHIP_OK;
    if (j.outer > kMxMax || j.axis_len > kMxMax || j.inner > kMxMax || j.outer * j.axis_len > kMxMax ||
        j.outer * j.axis_len * j.inner > kMxMax) {
        set_error("%s: job %d: more than 2^31 - 1 elements", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (j.x == nullptr || j.y == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    *n = j.outer * j.axis_len * j.inner;
    return PPQHIP_OK;
}

int64_t blocks_per_row(const ppqhip_mx_job& j) { return (j.axis_len + kMxBlock - 1) / kMxBlock; }

// An output shares memory with no other tensor of the call, with one exception: y == x, a tensor quantised in place (a block is read
// whole before any of it is written, and blocks are disjoint).
int validate(const char* what, const ppqhip_mx_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        int64_t n;
        if (int st = validate_job(what, k, jobs[k], &n)) return st;
        if (n == 0) continue;
        if ((const float*)jobs[k].y != jobs[k].x) ins.push_back(span_of(jobs[k].x, n));
        outs.push_back(span_of(jobs[k].y, n));
        if (jobs[k].scale_codes != nullptr) outs.push_back(span_of(jobs[k].scale_codes, jobs[k].outer * blocks_per_row(jobs[k]) * jobs[k].inner));
    }
    return check_overlap(what, ins, outs);
}

// the packed job and the workgroups it takes when a rows4 lane owns U float4; *ruled is raised to the class of the job's rule
uint32_t pack_job(const ppqhip_mx_job& src, int U, MxJob* d, int* ruled) {
    d->x = src.x; d->y = src.y; d->codes = src.scale_codes;
    d->len = (uint32_t)src.axis_len;
    const int64_t nb = blocks_per_row(src);
    d->nb = make_fastdiv((uint32_t)nb);
    d->inner = make_fastdiv((uint32_t)src.inner);
    int fmt;
    split_mx_format(src.format, &fmt, &d->rule);
    make_mx_fmt(fmt, &d->fmt);
    *ruled = std::max(*ruled, mx_rule_class(d->rule));
    const int64_t units = src.outer * nb * src.inner;                            // <= elements <= 2^31 - 1
    d->units = (uint32_t)units;
    int64_t per;
    if (src.inner > 1) { d->path = MX_STRIDED; per = kBlock; }
    else if (aligned16(src.x) && aligned16(src.y) && src.axis_len % 4 == 0) { d->path = MX_ROWS4; per = (int64_t)(kBlock / 8) * U; }
    else { d->path = MX_ROWS1; per = kBlock / kMxBlock; }
    return (uint32_t)((units + per - 1) / per);
}

constexpr int64_t kMxStreamElems = 48ll << 20;    // >= 192 MiB: streaming loads (see linear.hip)
constexpr int64_t kMxSmallElems = 4ll << 20;      // latency-bound tensors: one float4 per lane (see linear.hip)

double job_bytes(const ppqhip_mx_job& j) {
    const double n = (double)j.outer * (double)j.axis_len * (double)j.inner;
    return 8.0 * n + (j.scale_codes != nullptr ? (double)(j.outer * blocks_per_row(j) * j.inner) : 0.0);
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
    const int64_t n = outer * axis_len * inner;
    if (n == 0) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_FQ, job_bytes(job), s);
    MxArgs<1> args;
    const int U = n <= kMxSmallElems ? 1 : 2;
    int ruled = MX_PLAIN;
    const uint32_t blocks = pack_job(job, U, &args.jobs[0], &ruled);
    args.first_block[0] = 0;
    args.count = 1;
    if (n >= kMxStreamElems) launch_fq<1, 2, true>(ruled, blocks, s, args);
    else if (U == 2) launch_fq<1, 2, false>(ruled, blocks, s, args);
    else launch_fq<1, 1, false>(ruled, blocks, s, args);
    return finish_launch("mx_fq");
}

int ppqhip_mx_fq_multi(const ppqhip_mx_job* jobs, int num_jobs, void* stream) {
    if (int st = validate("mx_fq_multi", jobs, num_jobs)) return st;
    std::vector<const ppqhip_mx_job*> live;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        if (jobs[k].outer == 0 || jobs[k].axis_len == 0 || jobs[k].inner == 0) continue;
        live.push_back(&jobs[k]);
        bytes += job_bytes(jobs[k]);
    }
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_FQ, bytes, s);
    for (size_t base = 0; base < live.size(); base += kMxMaxJobs) {
        MxArgs<kMxMaxJobs> args;
        const uint32_t count = (uint32_t)std::min<size_t>(kMxMaxJobs, live.size() - base);
        uint64_t blocks = 0;
        int ruled = MX_PLAIN;
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += pack_job(*live[base + k], 1, &args.jobs[k], &ruled);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("mx_fq_multi: too many workgroups in one launch"); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        launch_fq<kMxMaxJobs, 1, false>(ruled, (uint32_t)blocks, s, args);
    }
    return finish_launch("mx_fq_multi");
}

}  // extern "C"
