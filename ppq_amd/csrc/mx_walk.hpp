// mx_walk.hpp -- THE walk over the MX blocks of a tensor addressed as [outer, axis_len, inner]: which lane
// holds which elements of which block, the clamped loads, the block's amax and its E8M0 code under the job's scale rule.  The fake
// quant (mx.hip), the packed export (mx_pack.hip) and the split of MX round tuning (mx_roundtune.hip) all walk through the templates
// below and add nothing but their element arithmetic and their stores.
//
// The bit contract: on one input the scale codes of mx_fq, the scales of mx_pack and the codes of mx_round_split are equal byte for
// byte, under every rule and on every path (so tuned weights are fixed points of mx_fq, and packed scales are the fake quant's).  It
// holds because the order below is the only one there is: all loads first, then per block the max over the lane's magnitudes, the
// max over the block's lanes (shuffles 4-2-1 or 16..1), mx_rule_code, and under MSE the adds in element order followed by the
// butterfly over the block's lanes.  A new rule, block size or addressing is written here once.
//
// Three addressings (workgroup-uniform per job; a job table may mix them):
//   rows4   inner == 1, every float pointer 16-B aligned, axis_len % 4 == 0: a block is 128 B, eight lanes load one float4 each (a
//           short last block switches whole lanes off), U float4 per lane issued back to back
//   rows1   inner == 1 otherwise: one element per lane, 32 lanes per block
//   strided inner > 1: one lane per (outer, block, inner) triple, numbered with inner fastest, so that each of the 32 loads of a
//           wave is coalesced along inner and a wave stays full when inner is small (9 for a 3x3 weight)
// The host half below is what the entry points of the three files share: the geometry and its checks, the filling of the walk, the
// choice of the RULED instantiation and the launches over a job table.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"

namespace ppqhip {

enum : uint32_t { MX_ROWS4 = 0, MX_ROWS1 = 1, MX_STRIDED = 2 };

struct MxWalk {                                   // 68 B, embedded in the device job of each kernel
    uint32_t len;                                 // axis_len
    uint32_t units;                               // blocks: outer * blocks per row * inner (one lane each on the strided path)
    FastDiv nb;                                   // blocks per row
    FastDiv inner;
    uint32_t path;
    MxFmt fmt;
    uint32_t rule;                                // PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE: read by the RULED instantiations only
};

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct MxGeometry {
    int64_t outer, axis_len, inner;
    int64_t nb() const { return (axis_len + kMxBlock - 1) / kMxBlock; }
    int64_t elems() const { return outer * axis_len * inner; }
    int64_t codes() const { return outer * nb() * inner; }
    bool empty() const { return outer == 0 || axis_len == 0 || inner == 0; }
};
template <typename Job>
inline MxGeometry mx_geometry_of(const Job& j) { return MxGeometry{j.outer, j.axis_len, j.inner}; }

// The format and the sizes of job k.  with_rule: `format` carries a scale rule above the format id (split_mx_format); without, the
// whole argument is the format, so that a rule byte is an unknown format.
inline int check_mx_job(const char* what, int k, int format, bool with_rule, const MxGeometry& g) {
    MxFmt probe;
    int fmt = format;
    uint32_t rule;
    if (with_rule && !split_mx_format(format, &fmt, &rule)) { set_error("%s: job %d: unknown MX scale rule in format %d", what, k, format); return PPQHIP_ERR_INVALID_VALUE; }
    if (!make_mx_fmt(fmt, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, fmt); return PPQHIP_ERR_INVALID_VALUE; }
    if (g.outer < 0 || g.axis_len < 0 || g.inner < 0) { set_error("%s: job %d: negative size", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    if (g.empty()) return PPQHIP_OK;
    if (g.outer > kMxMax || g.axis_len > kMxMax || g.inner > kMxMax || g.outer * g.axis_len > kMxMax || g.elems() > kMxMax) {
        set_error("%s: job %d: more than 2^31 - 1 elements", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

// Fills the walk of a checked, non-empty job and returns the workgroups it takes.  `format` may carry a scale rule; *ruled is raised
// to the class of that rule.  rows4_ok: the caller's pointers allow whole-dword or wider accesses per float4 lane; U: float4 per
// rows4 lane.
inline uint32_t fill_mx_walk(MxWalk* d, const MxGeometry& g, int format, bool rows4_ok, int U, int* ruled) {
    d->len = (uint32_t)g.axis_len;
    d->nb = make_fastdiv((uint32_t)g.nb());
    d->inner = make_fastdiv((uint32_t)g.inner);
    int fmt;
    split_mx_format(format, &fmt, &d->rule);
    make_mx_fmt(fmt, &d->fmt);
    *ruled = std::max(*ruled, mx_rule_class(d->rule));
    const int64_t units = g.codes();                                             // <= elements <= 2^31 - 1
    d->units = (uint32_t)units;
    int64_t per;
    if (g.inner > 1) { d->path = MX_STRIDED; per = kBlock; }
    else if (rows4_ok && g.axis_len % 4 == 0) { d->path = MX_ROWS4; per = (int64_t)(kBlock / 8) * U; }
    else { d->path = MX_ROWS1; per = kBlock / kMxBlock; }
    return (uint32_t)((units + per - 1) / per);
}

// launch(std::integral_constant<int, RULED>) for the class a launch needs (mx_rule_class)
template <typename Launch>
inline void with_mx_ruled(int ruled, Launch launch) {
    if (ruled == MX_SEARCH) launch(std::integral_constant<int, MX_SEARCH>());
    else if (ruled == MX_AMAX_RULES) launch(std::integral_constant<int, MX_AMAX_RULES>());
    else launch(std::integral_constant<int, MX_PLAIN>());
}

// the jobs of a checked table that have elements
template <typename Job>
inline std::vector<const Job*> live_mx_jobs(const Job* jobs, int num_jobs) {
    std::vector<const Job*> live;
    for (int k = 0; k < num_jobs; k++)
        if (!mx_geometry_of(jobs[k]).empty()) live.push_back(&jobs[k]);
    return live;
}

// The launches of an entry point over its live jobs, a table of Args' capacity at a time ("Job tables").
// fill(job, device job, &ruled) returns the job's workgroups; launch(ruled, workgroups, args) starts the kernel.
template <typename Args, typename Job, typename Fill, typename Launch>
inline int launch_mx_jobs(const char* what, const std::vector<const Job*>& live, Fill fill, Launch launch) {
    constexpr size_t capacity = sizeof(Args::jobs) / sizeof(Args::jobs[0]);
    for (size_t base = 0; base < live.size(); base += capacity) {
        Args args;
        const uint32_t count = (uint32_t)std::min(capacity, live.size() - base);
        uint64_t blocks = 0;
        int ruled = MX_PLAIN;
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += fill(*live[base + k], &args.jobs[k], &ruled);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        launch(ruled, (uint32_t)blocks, args);
    }
    return finish_launch(what);
}

#if defined(__HIPCC__)

// ---- device: positions ----------------------------------------------------------------------------------------------------------
// A lane of the row paths: PER elements (4: eight lanes per block, 1: 32 lanes) of block `g`.  Lanes behind the last block are
// clamped onto it and lanes behind the end of a short block onto its start, so that every lane loads and takes part in the shuffles.
struct MxRowPos {
    uint32_t g, q;                                // the block; the lane's place among the block's lanes
    bool in, ok;                                  // the block exists; so do the lane's elements (len % 4 == 0: all four or none)
    size_t at;                                    // offset of the lane's first element; of the block's first where !ok
};
template <uint32_t PER>
__device__ __forceinline__ MxRowPos mx_row_pos(const MxWalk& j, uint32_t step) {      // step: local * U + k
    constexpr uint32_t kLanes = kMxBlock / PER;
    MxRowPos p;
    p.q = threadIdx.x & (kLanes - 1u);
    const uint32_t want = step * (kBlock / kLanes) + threadIdx.x / kLanes;
    p.in = want < j.units;
    p.g = min(want, j.units - 1);
    const uint32_t row = fdiv(p.g, j.nb), b = p.g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + p.q * PER;
    p.ok = p.in && e < j.len;
    p.at = (size_t)row * j.len + (e < j.len ? e : b * kMxBlock);
    return p;
}

// A lane of the strided path: block b of row (o, i), lanes numbered w = (o * nb + b) * inner + i; its blen >= 1 elements lie at
// base + t * step.
struct MxStridedPos {
    bool in;
    uint32_t w, o, b, i, blen;
    size_t base, step;
};
__device__ __forceinline__ MxStridedPos mx_strided_pos(const MxWalk& j, uint32_t local) {
    MxStridedPos p;
    const uint32_t want = local * kBlock + threadIdx.x;
    p.in = want < j.units;
    p.w = min(want, j.units - 1);
    const uint32_t blk = fdiv(p.w, j.inner);
    p.i = p.w - blk * j.inner.d;
    p.o = fdiv(blk, j.nb);
    p.b = blk - p.o * j.nb.d;
    p.blen = min(kMxBlock, j.len - p.b * kMxBlock);
    p.base = ((size_t)p.o * j.len + (size_t)p.b * kMxBlock) * j.inner.d + p.i;
    p.step = j.inner.d;
    return p;
}

// ---- device: the block's code ---------------------------------------------------------------------------------------------------
// From the block's reduced amax `m`: the floor rule's own code in the plain instantiation, the job's rule above it; under MSE the N
// values this lane holds are added in order and the sums of the LANES lanes of the block combined.
// NANBLOCK (the packed export, whose magnitudes mark a NaN that the element format cannot encode with kMxNaNBlock): such a block is
// NaN as a whole -- the rule sees amax 0 and the code is 0xFF, the E8M0 NaN, under every rule.
template <int RULED, int LANES, bool NANBLOCK, int N>
__device__ __forceinline__ uint32_t mx_block_code(const MxWalk& j, uint32_t m, const float (&v)[N], const bool (&counts)[N]) {
    const bool dead = NANBLOCK && m == kMxNaNBlock;
    if (dead) m = 0u;
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
    return dead ? 0xffu : code;
}

// ---- device: the walks ----------------------------------------------------------------------------------------------------------
// mag(v): the magnitude an element brings to the block maximum (mx_finite_mag, or the coder's mxp_mag).
// A body takes its job's format and output pointers from locals made ahead of the walk: read through the job inside the lambda, the
// compiler fetches them from the kernel arguments again after every store (measured: 1 - 5 % on the strided bodies).
// Row paths: body(MxRowPos, the lane's PER values, code) runs on every lane, switched-off ones included (it may shuffle).
template <uint32_t PER, int U, bool NT, int RULED, bool NANBLOCK, typename Mag, typename Body>
__device__ __forceinline__ void mx_rows(const MxWalk& j, const float* x, uint32_t local, Mag mag, Body body) {
    constexpr int kLanes = kMxBlock / PER;
    MxRowPos p[U];
    float v[U][PER];
#pragma unroll
    for (int k = 0; k < U; k++) {                                                // clamped, branch-free: all U loads issue back to back
        p[k] = mx_row_pos<PER>(j, local * U + k);
        if constexpr (PER == 4) {
            const float4 a = load4<NT>(reinterpret_cast<const float4*>(x + p[k].at));
            v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = a.w;
        } else {
            v[k][0] = x[p[k].at];
        }
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
        uint32_t m;
        if constexpr (PER == 4) m = max(max(mag(v[k][0]), mag(v[k][1])), max(mag(v[k][2]), mag(v[k][3])));
        else m = mag(v[k][0]);
        m = p[k].ok ? m : 0u;
#pragma unroll
        for (int s = kLanes / 2; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
        bool counts[PER];
#pragma unroll
        for (uint32_t t = 0; t < PER; t++) counts[t] = p[k].ok;
        body(p[k], v[k], mx_block_code<RULED, kLanes, NANBLOCK>(j, m, v[k], counts));
    }
}
template <int U, bool NT, int RULED, bool NANBLOCK = false, typename Mag, typename Body>
__device__ __forceinline__ void mx_rows4(const MxWalk& j, const float* x, uint32_t local, Mag mag, Body body) {
    mx_rows<4, U, NT, RULED, NANBLOCK>(j, x, local, mag, body);
}
template <int RULED, bool NANBLOCK = false, typename Mag, typename Body>
__device__ __forceinline__ void mx_rows1(const MxWalk& j, const float* x, uint32_t local, Mag mag, Body body) {
    mx_rows<1, 1, false, RULED, NANBLOCK>(j, x, local, mag, body);
}

// Strided path: body(MxStridedPos, the block's 32 values (those behind blen repeat the last), code) runs on the lanes that are in.
template <int RULED, bool NANBLOCK = false, typename Mag, typename Body>
__device__ __forceinline__ void mx_strided(const MxWalk& j, const float* x, uint32_t local, Mag mag, Body body) {
    const MxStridedPos p = mx_strided_pos(j, local);
    float v[kMxBlock];
    bool counts[kMxBlock];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) v[t] = x[p.base + min(t, p.blen - 1) * p.step];       // clamped: 32 loads in flight
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) { counts[t] = t < p.blen; m = max(m, counts[t] ? mag(v[t]) : 0u); }
    const uint32_t code = mx_block_code<RULED, 1, NANBLOCK>(j, m, v, counts);
    if (!p.in) return;
    body(p, v, code);
}

#endif  // __HIPCC__

}  // namespace ppqhip
