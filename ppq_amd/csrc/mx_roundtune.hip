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
// The split needs the block amax (and the MSE sums): its three bodies are those of mx.hip -- rows4 / rows1 / strided, the same
// addressing, the same clamped loads, the same reductions and the same order of the MSE adds, so the codes are mx.hip's bit for bit
// -- written out here with their own stores rather than shared through a header: mx.hip's instantiations stay as they are compiled.
// Weights are small, so a rows4 lane owns one float4 and nothing streams.  Job tables: DESIGN.md, "Job tables".
#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"

namespace ppqhip {
namespace {

enum : uint32_t { RS_ROWS4 = 0, RS_ROWS1 = 1, RS_STRIDED = 2 };
constexpr int kMxRoundMaxJobs = 32;               // jobs of one launch of either kernel

struct RsJob {                                    // 104 B
    const float* w;
    float* floored;
    float* rounding;
    uint8_t* codes;
    uint32_t len;                                 // axis_len
    uint32_t units;                               // rows4 / rows1: outer * blocks per row; strided: outer * blocks per row * inner
    FastDiv nb;                                   // blocks per row
    FastDiv inner;
    uint32_t path;
    MxFmt fmt;
    uint32_t rule;                                // read by the RULED instantiations only
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
// The block's code from its reduced amax `m`, as mx.hip takes it: the floor rule's own code in the plain instantiation, the job's
// rule above it; under MSE the N values this lane holds are added in order and the sums of the LANES lanes of the block combined.
template <int RULED, int LANES, int N>
__device__ __forceinline__ uint32_t rs_code(const RsJob& j, uint32_t m, const float (&v)[N], const bool (&counts)[N]) {
    uint32_t code = mx_code(m, j.fmt);
    if constexpr (RULED != MX_PLAIN) {
        code = mx_rule_code(m, j.fmt, j.rule);
        if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {                  // workgroup-uniform
            MxMse s(code);
#pragma unroll
            for (int k = 0; k < N; k++) s.add(v[k], counts[k], j.fmt);
            if constexpr (LANES > 1) s.template reduce<LANES>();
            code = s.code();
        }
    }
    return code;
}

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
__device__ __forceinline__ void rs_rows4(const RsJob& j, uint32_t local) {
    constexpr uint32_t kGroups = kBlock / 8;                                     // blocks per workgroup
    const uint32_t q = threadIdx.x & 7u;
    const uint32_t want = local * kGroups + (threadIdx.x >> 3);
    const bool in = want < j.units;
    const uint32_t g = min(want, j.units - 1);
    const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + q * 4;
    const bool ok = in && e < j.len;                                             // len % 4 == 0: a float4 is inside the row or outside
    const size_t at = (size_t)row * j.len + (e < j.len ? e : b * kMxBlock);
    const float4 a = *reinterpret_cast<const float4*>(j.w + at);
    uint32_t m = max(max(mx_finite_mag(a.x), mx_finite_mag(a.y)), max(mx_finite_mag(a.z), mx_finite_mag(a.w)));
    m = ok ? m : 0u;
    m = max(m, (uint32_t)__shfl_xor((int)m, 4, 64));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
    m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
    const float v[4] = {a.x, a.y, a.z, a.w};
    const bool counts[4] = {ok, ok, ok, ok};
    const uint32_t code = rs_code<RULED, 8>(j, m, v, counts);
    const float X = mx_pow2(code), inv = mx_pow2(254u - code);
    const RsElem r0 = rs_elem(a.x, inv, X, j.fmt), r1 = rs_elem(a.y, inv, X, j.fmt), r2 = rs_elem(a.z, inv, X, j.fmt),
                 r3 = rs_elem(a.w, inv, X, j.fmt);
    if (ok) {
        *reinterpret_cast<float4*>(j.floored + at) = make_float4(r0.floored, r1.floored, r2.floored, r3.floored);
        *reinterpret_cast<float4*>(j.rounding + at) = make_float4(r0.rounding, r1.rounding, r2.rounding, r3.rounding);
    }
    if (in && q == 0) j.codes[g] = (uint8_t)code;
}

template <int RULED>
__device__ __forceinline__ void rs_rows1(const RsJob& j, uint32_t local) {
    const uint32_t q = threadIdx.x & 31u;
    const uint32_t want = local * (kBlock / kMxBlock) + (threadIdx.x >> 5);
    const bool in = want < j.units;
    const uint32_t g = min(want, j.units - 1);
    const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + q;
    const bool ok = in && e < j.len;
    const size_t at = (size_t)row * j.len + (e < j.len ? e : b * kMxBlock);
    const float v[1] = {j.w[at]};
    const bool counts[1] = {ok};
    uint32_t m = ok ? mx_finite_mag(v[0]) : 0u;
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    const uint32_t code = rs_code<RULED, 32>(j, m, v, counts);
    const RsElem r = rs_elem(v[0], mx_pow2(254u - code), mx_pow2(code), j.fmt);
    if (ok) { j.floored[at] = r.floored; j.rounding[at] = r.rounding; }
    if (in && q == 0) j.codes[g] = (uint8_t)code;
}

template <int RULED>
__device__ __forceinline__ void rs_strided(const RsJob& j, uint32_t local) {
    const uint32_t want = local * kBlock + threadIdx.x;
    const bool in = want < j.units;
    const uint32_t w = min(want, j.units - 1);
    const uint32_t blk = fdiv(w, j.inner), i = w - blk * j.inner.d;
    const uint32_t o = fdiv(blk, j.nb), b = blk - o * j.nb.d;
    const uint32_t blen = min(kMxBlock, j.len - b * kMxBlock);                   // >= 1
    const size_t base = ((size_t)o * j.len + (size_t)b * kMxBlock) * j.inner.d + i;
    const size_t step = j.inner.d;
    float v[kMxBlock];
    bool counts[kMxBlock];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) v[t] = j.w[base + min(t, blen - 1) * step];      // clamped: 32 loads in flight
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) { counts[t] = t < blen; m = max(m, counts[t] ? mx_finite_mag(v[t]) : 0u); }
    const uint32_t code = rs_code<RULED, 1>(j, m, v, counts);
    const float X = mx_pow2(code), inv = mx_pow2(254u - code);
    if (!in) return;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) {
        if (t < blen) {
            const RsElem r = rs_elem(v[t], inv, X, j.fmt);
            j.floored[base + t * step] = r.floored;
            j.rounding[base + t * step] = r.rounding;
        }
    }
    j.codes[w] = (uint8_t)code;
}

template <int RULED>
__global__ __launch_bounds__(kBlock) void mx_round_split_kernel(const RsArgs args) {
    uint32_t local;
    const RsJob& j = args.jobs[job_of(args, local)];
    if (j.path == RS_ROWS4) rs_rows4<RULED>(j, local);                           // workgroup-uniform
    else if (j.path == RS_ROWS1) rs_rows1<RULED>(j, local);
    else rs_strided<RULED>(j, local);
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
struct Geometry { int64_t outer, axis_len, inner; };
int64_t blocks_per_row(const Geometry& g) { return (g.axis_len + kMxBlock - 1) / kMxBlock; }
int64_t num_codes(const Geometry& g) { return g.outer * blocks_per_row(g) * g.inner; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the size checks of one job; *n = its elements (0: nothing to do)
int validate_geometry(const char* what, int k, const Geometry& g, int64_t* n) {
    if (g.outer < 0 || g.axis_len < 0 || g.inner < 0) { set_error("%s: job %d: negative size", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    *n = 0;
    if (g.outer == 0 || g.axis_len == 0 || g.inner == 0) return PPQHIP_OK;
    if (g.outer > kMxMax || g.axis_len > kMxMax || g.inner > kMxMax || g.outer * g.axis_len > kMxMax ||
        g.outer * g.axis_len * g.inner > kMxMax) {
        set_error("%s: job %d: more than 2^31 - 1 elements", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    *n = g.outer * g.axis_len * g.inner;
    return PPQHIP_OK;
}

int validate_split(const char* what, const ppqhip_mx_round_split_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_mx_round_split_job& j = jobs[k];
        MxFmt probe;
        int fmt;
        uint32_t rule;
        if (!split_mx_format(j.format, &fmt, &rule)) { set_error("%s: job %d: unknown MX scale rule in format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
        if (!make_mx_fmt(fmt, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, fmt); return PPQHIP_ERR_INVALID_VALUE; }
        const Geometry g{j.outer, j.axis_len, j.inner};
        int64_t n;
        if (int st = validate_geometry(what, k, g, &n)) return st;
        if (n == 0) continue;
        if (!j.w || !j.floored || !j.rounding || !j.scale_codes) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!aligned4(j.w) || !aligned4(j.floored) || !aligned4(j.rounding)) { set_error("%s: job %d: a float pointer is not 4-byte aligned", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        ins.push_back(span_of(j.w, n));
        outs.push_back(span_of(j.floored, n));
        outs.push_back(span_of(j.rounding, n));
        outs.push_back(span_of(j.scale_codes, num_codes(g)));
    }
    return check_overlap(what, ins, outs);
}

int validate_fwd(const char* what, const ppqhip_mx_round_fwd_job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_mx_round_fwd_job& j = jobs[k];
        MxFmt probe;
        if (j.format < 0 || (j.format >> PPQHIP_MX_RULE_SHIFT) != 0) { set_error("%s: job %d: format %d carries a scale rule, but the codes are given", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
        if (!make_mx_fmt(j.format, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
        const Geometry g{j.outer, j.axis_len, j.inner};
        int64_t n;
        if (int st = validate_geometry(what, k, g, &n)) return st;
        if (n == 0) continue;
        if (!j.floored || !j.rounding || !j.scale_codes || !j.out) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!aligned4(j.floored) || !aligned4(j.rounding) || !aligned4(j.out)) { set_error("%s: job %d: a float pointer is not 4-byte aligned", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        ins.push_back(span_of(j.floored, n));
        ins.push_back(span_of(j.rounding, n));
        ins.push_back(span_of(j.scale_codes, num_codes(g)));
        outs.push_back(span_of(j.out, n));
    }
    return check_overlap(what, ins, outs);
}

// the packed job and its workgroups; *ruled is raised to the class of the job's rule
uint32_t pack_split(const ppqhip_mx_round_split_job& src, RsJob* d, int* ruled) {
    d->w = src.w; d->floored = src.floored; d->rounding = src.rounding; d->codes = src.scale_codes;
    d->len = (uint32_t)src.axis_len;
    const Geometry g{src.outer, src.axis_len, src.inner};
    const int64_t nb = blocks_per_row(g);
    d->nb = make_fastdiv((uint32_t)nb);
    d->inner = make_fastdiv((uint32_t)src.inner);
    int fmt;
    split_mx_format(src.format, &fmt, &d->rule);
    make_mx_fmt(fmt, &d->fmt);
    *ruled = std::max(*ruled, mx_rule_class(d->rule));
    const int64_t units = num_codes(g);                                          // <= elements <= 2^31 - 1
    d->units = (uint32_t)units;
    int64_t per;
    if (src.inner > 1) { d->path = RS_STRIDED; per = kBlock; }
    else if (aligned16(src.w) && aligned16(src.floored) && aligned16(src.rounding) && src.axis_len % 4 == 0) { d->path = RS_ROWS4; per = kBlock / 8; }
    else { d->path = RS_ROWS1; per = kBlock / kMxBlock; }
    return (uint32_t)((units + per - 1) / per);
}

uint32_t pack_fwd(const ppqhip_mx_round_fwd_job& src, RfJob* d) {
    d->floored = src.floored; d->rounding = src.rounding; d->codes = src.scale_codes; d->out = src.out;
    const Geometry g{src.outer, src.axis_len, src.inner};
    const int64_t n = src.outer * src.axis_len * src.inner;
    d->vec = (src.inner == 1 && src.axis_len % 4 == 0 && aligned16(src.floored) && aligned16(src.rounding) && aligned16(src.out)) ? 1u : 0u;
    d->units = (uint32_t)(d->vec ? n / 4 : n);
    d->plane = make_fastdiv((uint32_t)(src.axis_len * src.inner));
    d->inner = make_fastdiv((uint32_t)src.inner);
    d->nb = (uint32_t)blocks_per_row(g);
    make_mx_fmt(src.format, &d->fmt);
    return (uint32_t)(((int64_t)d->units + kBlock - 1) / kBlock);
}

void launch_split(int ruled, uint32_t blocks, hipStream_t s, const RsArgs& args) {
    if (ruled == MX_SEARCH) hipLaunchKernelGGL(mx_round_split_kernel<MX_SEARCH>, dim3(blocks), dim3(kBlock), 0, s, args);
    else if (ruled == MX_AMAX_RULES) hipLaunchKernelGGL(mx_round_split_kernel<MX_AMAX_RULES>, dim3(blocks), dim3(kBlock), 0, s, args);
    else hipLaunchKernelGGL(mx_round_split_kernel<MX_PLAIN>, dim3(blocks), dim3(kBlock), 0, s, args);
}

template <typename Job>
bool is_empty(const Job& j) { return j.outer == 0 || j.axis_len == 0 || j.inner == 0; }

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_mx_round_split_multi(const ppqhip_mx_round_split_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_split("mx_round_split_multi", jobs, num_jobs)) return st;
    std::vector<const ppqhip_mx_round_split_job*> live;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        if (is_empty(jobs[k])) continue;
        live.push_back(&jobs[k]);
        const Geometry g{jobs[k].outer, jobs[k].axis_len, jobs[k].inner};
        bytes += 12.0 * (double)(g.outer * g.axis_len * g.inner) + (double)num_codes(g);       // w in; floored, rounding, codes out
    }
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_ROUND_SPLIT, bytes, s);
    for (size_t base = 0; base < live.size(); base += kMxRoundMaxJobs) {
        RsArgs args;
        const uint32_t count = (uint32_t)std::min<size_t>(kMxRoundMaxJobs, live.size() - base);
        uint64_t blocks = 0;
        int ruled = MX_PLAIN;
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += pack_split(*live[base + k], &args.jobs[k], &ruled);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("mx_round_split_multi: too many workgroups in one launch"); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        launch_split(ruled, (uint32_t)blocks, s, args);
    }
    return finish_launch("mx_round_split_multi");
}

int ppqhip_mx_round_fwd_multi(const ppqhip_mx_round_fwd_job* jobs, int num_jobs, void* stream) {
    if (int st = validate_fwd("mx_round_fwd_multi", jobs, num_jobs)) return st;
    std::vector<const ppqhip_mx_round_fwd_job*> live;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        if (is_empty(jobs[k])) continue;
        live.push_back(&jobs[k]);
        const Geometry g{jobs[k].outer, jobs[k].axis_len, jobs[k].inner};
        bytes += 12.0 * (double)(g.outer * g.axis_len * g.inner) + (double)num_codes(g);       // floored, rounding, codes in; out
    }
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_ROUND_FWD, bytes, s);
    for (size_t base = 0; base < live.size(); base += kMxRoundMaxJobs) {
        RfArgs args;
        const uint32_t count = (uint32_t)std::min<size_t>(kMxRoundMaxJobs, live.size() - base);
        uint64_t blocks = 0;
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += pack_fwd(*live[base + k], &args.jobs[k]);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("mx_round_fwd_multi: too many workgroups in one launch"); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        hipLaunchKernelGGL(mx_round_fwd_kernel, dim3(blocks), dim3(kBlock), 0, s, args);
    }
    return finish_launch("mx_round_fwd_multi");
}

}  // extern "C"
