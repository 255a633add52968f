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
// Three bodies behind ONE kernel (job table in the kernel arguments, DESIGN.md "Job tables"; the single-tensor entry point is a table
// of one job).  Each reads every element once and writes it once; the block's values wait in registers between the max and the cast:
//   rows4   inner == 1, 16-B aligned, axis_len % 4 == 0: a block is 128 B, eight lanes load one float4 each (a short last block
//           switches whole lanes off), integer max over the magnitudes with three shuffles inside the eight lanes
//   rows1   inner == 1 otherwise: one element per lane, 32 lanes per block, five shuffles -- the same arithmetic
//   strided inner > 1: one lane per (outer, block, inner) triple, numbered with inner fastest, so that each of the 32 loads of a
//           wave is coalesced along inner and a wave stays full when inner is small (9 for a 3x3 weight)
#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

struct MxFmt {                 // 28 B
    uint32_t emax;             // the element format's largest exponent: the shared exponent is exponent(amax) - emax
    uint32_t shift;            // 23 - mantissa bits: float32 mantissa bits a normal element drops
    uint32_t half_m1;          // (1 << (shift - 1)) - 1: with the kept LSB added, a carry out of the dropped bits <=> round up (RNE)
    uint32_t sub_limit;        // |u| patterns below this are on the format's fixed-point grid (its subnormals; all of MXINT8)
    float sub_scale;           // 1 / that grid's spacing
    float sub_quantum;         // the grid's spacing
    uint32_t max_bits;         // pattern of the largest normal
};

constexpr uint32_t f32_bits(int exponent) { return (uint32_t)(exponent + 127) << 23; }      // 2^exponent, -126 <= exponent <= 127

// float formats: mantissa bits m, smallest normal exponent emin = 1 - bias, largest normal (2 - 2^-m) 2^emax -- E4M3 gives its
// all-ones mantissa at emax to NaN, so its largest normal is 1.75 * 2^8
bool make_mx_fmt(int format, MxFmt* f) {
    int m, emin, emax;
    uint32_t top_mantissa;     // mantissa field of the largest normal, in m bits
    switch (format) {
        case PPQHIP_MXFP8_E4M3: m = 3; emin = -6; emax = 8; top_mantissa = 6; break;
        case PPQHIP_MXFP8_E5M2: m = 2; emin = -14; emax = 15; top_mantissa = 3; break;
        case PPQHIP_MXFP6_E3M2: m = 2; emin = -2; emax = 4; top_mantissa = 3; break;
        case PPQHIP_MXFP6_E2M3: m = 3; emin = 0; emax = 2; top_mantissa = 7; break;
        case PPQHIP_MXFP4_E2M1: m = 1; emin = 0; emax = 2; top_mantissa = 1; break;
        case PPQHIP_MXINT8:                                                      // k / 64, |k| <= 127: one fixed-point grid
            f->emax = 0; f->shift = 17; f->half_m1 = (1u << 16) - 1u; f->sub_limit = 0x7f800000u;
            f->sub_scale = 64.0f; f->sub_quantum = 0.015625f; f->max_bits = f32_bits(0) | (63u << 17);      // 127 / 64
            return true;
        default: return false;
    }
    f->emax = (uint32_t)emax; f->shift = (uint32_t)(23 - m); f->half_m1 = (1u << (22 - m)) - 1u;
    f->sub_limit = f32_bits(emin);
    union { uint32_t d; float v; } s, q;
    s.d = f32_bits(m - emin); q.d = f32_bits(emin - m);
    f->sub_scale = s.v; f->sub_quantum = q.v;
    f->max_bits = f32_bits(emax) | (top_mantissa << (23 - m));
    return true;
}

enum : uint32_t { MX_ROWS4 = 0, MX_ROWS1 = 1, MX_STRIDED = 2 };
constexpr uint32_t kMxBlock = 32;                 // elements per MX block

struct MxJob {                                    // 88 B
    const float* x;
    float* y;
    uint8_t* codes;                               // E8M0 scale codes, one per block, or null
    uint32_t len;                                 // axis_len
    uint32_t units;                               // rows4 / rows1: outer * blocks per row; strided: outer * blocks per row * inner
    FastDiv nb;                                   // blocks per row
    FastDiv inner;
    uint32_t path;
    MxFmt fmt;
};
template <int CAP>
struct MxArgs {
    MxJob jobs[CAP];
    uint32_t first_block[CAP];
    uint32_t count;
};
constexpr int kMxMaxJobs = 40;
static_assert(sizeof(MxArgs<kMxMaxJobs>) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ uint32_t mx_finite_mag(float v) {                     // |v|'s pattern; NaN and Inf do not take part
    const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
    return m < 0x7f800000u ? m : 0u;
}
// E8M0 code of a block from the pattern of its amax: a subnormal or zero amax has exponent field 0 and clamps to code 0 (2^-127)
__device__ __forceinline__ uint32_t mx_code(uint32_t amax_bits, const MxFmt& f) {
    const uint32_t e = amax_bits >> 23;
    return e > f.emax ? e - f.emax : 0u;
}
__device__ __forceinline__ float mx_pow2(uint32_t biased) {                      // 2^(biased - 127), 0 <= biased <= 254
    return __uint_as_float(biased ? biased << 23 : 0x00400000u);
}
// cast(v / X) * X on the float32 pattern.  Normal elements: round the mantissa to nearest even with one integer add (the carry runs
// into the exponent as it should); the fixed-point grid: rint() of the scaled magnitude (round half to even = the even encoding);
// both saturate at the largest normal, which also takes Inf.
__device__ __forceinline__ float mx_elem(float v, float inv, float X, const MxFmt& f) {
    const float u = v * inv;
    const uint32_t bits = __float_as_uint(u), sign = bits & 0x80000000u, mag = bits & 0x7fffffffu;
    const uint32_t rn = (mag + f.half_m1 + ((mag >> f.shift) & 1u)) & ~((1u << f.shift) - 1u);
    const uint32_t rs = __float_as_uint(__builtin_rintf(__uint_as_float(mag) * f.sub_scale) * f.sub_quantum);
    const uint32_t r = min(mag < f.sub_limit ? rs : rn, f.max_bits);
    const float q = __uint_as_float(r | sign) * X;
    return mag > 0x7f800000u ? v : q;
}

template <int U, bool NT>
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
        const uint32_t code = mx_code(m, j.fmt);
        const float X = mx_pow2(code), inv = mx_pow2(254u - code);
        float4 r;
        r.x = mx_elem(a[k].x, inv, X, j.fmt); r.y = mx_elem(a[k].y, inv, X, j.fmt);
        r.z = mx_elem(a[k].z, inv, X, j.fmt); r.w = mx_elem(a[k].w, inv, X, j.fmt);
        if (ok[k]) *reinterpret_cast<float4*>(j.y + at[k]) = r;
        if (in[k] && q == 0 && j.codes != nullptr) j.codes[g[k]] = (uint8_t)code;
    }
}

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
    const uint32_t code = mx_code(m, j.fmt);
    const float r = mx_elem(v, mx_pow2(254u - code), mx_pow2(code), j.fmt);
    if (ok) j.y[at] = r;
    if (in && q == 0 && j.codes != nullptr) j.codes[g] = (uint8_t)code;
}

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
    const uint32_t code = mx_code(m, j.fmt);
    const float X = mx_pow2(code), inv = mx_pow2(254u - code);
    if (!in) return;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++)
        if (t < blen) j.y[base + t * step] = mx_elem(v[t], inv, X, j.fmt);
    if (j.codes != nullptr) j.codes[w] = (uint8_t)code;
}

template <int CAP, int U, bool NT>
__global__ __launch_bounds__(kBlock) void mx_fq_kernel(const MxArgs<CAP> args) {
    uint32_t local;
    const MxJob& j = args.jobs[job_of(args, local)];
    if (j.path == MX_ROWS4) mx_rows4<U, NT>(j, local);                           // workgroup-uniform
    else if (j.path == MX_ROWS1) mx_rows1(j, local);
    else mx_strided(j, local);
}

constexpr int64_t kMxMax = 0x7fffffffLL;

// the checks of one job; *n = its elements (0: nothing to do)
int validate_job(const char* what, int k, const ppqhip_mx_job& j, int64_t* n) {
    MxFmt probe;
    if (!make_mx_fmt(j.format, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
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

// the packed job and the workgroups it takes when a rows4 lane owns U float4
uint32_t pack_job(const ppqhip_mx_job& src, int U, MxJob* d) {
    d->x = src.x; d->y = src.y; d->codes = src.scale_codes;
    d->len = (uint32_t)src.axis_len;
    const int64_t nb = blocks_per_row(src);
    d->nb = make_fastdiv((uint32_t)nb);
    d->inner = make_fastdiv((uint32_t)src.inner);
    make_mx_fmt(src.format, &d->fmt);
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
    const uint32_t blocks = pack_job(job, U, &args.jobs[0]);
    args.first_block[0] = 0;
    args.count = 1;
    if (n >= kMxStreamElems) hipLaunchKernelGGL((mx_fq_kernel<1, 2, true>), dim3(blocks), dim3(kBlock), 0, s, args);
    else if (U == 2) hipLaunchKernelGGL((mx_fq_kernel<1, 2, false>), dim3(blocks), dim3(kBlock), 0, s, args);
    else hipLaunchKernelGGL((mx_fq_kernel<1, 1, false>), dim3(blocks), dim3(kBlock), 0, s, args);
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
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += pack_job(*live[base + k], 1, &args.jobs[k]);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("mx_fq_multi: too many workgroups in one launch"); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        hipLaunchKernelGGL((mx_fq_kernel<kMxMaxJobs, 1, false>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
    }
    return finish_launch("mx_fq_multi");
}

}  // extern "C"
