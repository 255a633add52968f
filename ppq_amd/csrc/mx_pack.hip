// mx_pack.hip -- packed OCP Microscaling export for gfx950: float32 -> element codes + E8M0 scales (pack) and back (unpack).
//
// The contract is DESIGN.md section 9.13 and tests/mx_pack_reference.py.  Blocks, amax, shared exponent, cast and saturation are
// those of mx.hip (mx_common.hpp: the element code is read off the rounded float32 pattern mx_round returns).  The input is
// addressed as [outer, axis_len, inner]; the packed tensor has the block axis LAST and every block at full size:
//   scales   uint8 [outer, inner, nb]        nb = ceil(axis_len / 32); the E8M0 code of the block
//   elements uint8 [outer, inner, nb * B]    B = 32 (MXFP8, MXINT8), 24 (MXFP6), 16 (MXFP4) bytes per block; element i of a block sits
//            at bits [i * w, i * w + w) of the block's bytes read as one little-endian bit string (w = 8, 6, 4); the elements a short
//            last block lacks are +0
// NaN: MXFP8 has a NaN encoding (S.1111.111 / S.11111.11 = 0x7f under the sign) and the element takes it; the other formats have
// none: a block that holds a NaN gets scale 0xFF (the E8M0 NaN) and zero element bytes.  +-Inf saturates; zero keeps its sign except
// in MXINT8 (two's complement has no -0).  Unpack: value(code) * 2^(scale - 127); scale 0xFF, an FP8 NaN code -> the quiet NaN
// 0x7fc00000 (with the element's sign bit in MXFP8); an E5M2 Inf code -> +-Inf; the tail padding is dropped.
//
// One kernel per direction behind a job table (job_table.hpp) over the three addressings of mx_walk.hpp.  Pack walks as mx.hip does
// -- loads, amax and the block's scale under the job's scale rule are the walk's -- and adds the element
// codes and their stores; unpack reduces nothing, reads scales as stored and knows no rule: it takes the walk's positions only.
//   rows4   also needs the packed side 4-B aligned: a lane's four codes are 4 / 3 / 2 bytes, lanes are combined through shuffles so
//           that every store is one dword (FP6: three lanes of four store; FP4: every other lane); two float4 per lane above 4 M
//           elements, as in mx.hip
//   rows1   byte stores
//   strided the lane owns the B bytes of its block (16-B stores, 8-B for the 24-B blocks of FP6; bytes when `elements` is not 16-B
//           aligned).  This is where the axis moves last: the lane's block in packed order is (o * inner + i) * nb + b.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_coder.hpp"
#include "mx_common.hpp"
#include "mx_walk.hpp"

namespace ppqhip {
namespace {

struct MxPackJob {                                // 96 B; pack: f -> e, s; unpack: e, s -> f
    float* f;                                     // the float32 tensor, [outer, axis_len, inner]
    uint8_t* e;                                   // elements
    uint8_t* s;                                   // scales
    MxWalk walk;
    uint16_t format;
    uint16_t bytes;                               // strided: `e` is not 16-B aligned, the block's bytes are stored one by one
};
template <int CAP>
struct MxPackArgs {
    MxPackJob jobs[CAP];
    uint32_t first_block[CAP];
    uint32_t count;
};
static_assert(sizeof(MxPackArgs<kMxMaxJobs>) <= 4096, "kernel arguments are limited to 4 KB");

constexpr uint32_t kQuietNaN = 0x7fc00000u;

// the element coder (MxCoder, make_coder, mxp_mag, mxp_scale, mxp_code) is mx_coder.hpp: the fused epilogue of mx_mfma.hpp packs
// with it too

// value(code) * X
__device__ __forceinline__ float mxp_value(uint32_t code, float X, bool scale_nan, const MxFmt& f, const MxCoder& c) {
    if (c.is_int) {
        const float y = (float)(int)(int8_t)code * f.sub_quantum * X;
        return scale_nan ? __uint_as_float(kQuietNaN) : y;
    }
    const uint32_t m = 23u - f.shift;
    const uint32_t sign = (code >> (c.bits - 1u)) & 1u, mag = code & ((1u << (c.bits - 1u)) - 1u);
    const uint32_t e = mag >> m, man = mag & ((1u << m) - 1u);
    const uint32_t normal = (mag << f.shift) + (c.code_bias << f.shift);
    const uint32_t sub = __float_as_uint((float)man * f.sub_quantum);
    const float y = __uint_as_float((e ? normal : sub) | (sign << 31)) * X;
    bool nan = scale_nan, inf = false;
    if (c.has_nan) {
        if (f.shift == 20u) nan = nan || mag == 0x7fu;                           // E4M3: S.1111.111
        else { nan = nan || (e == 31u && man != 0u); inf = e == 31u && man == 0u; }
    }
    const uint32_t s = c.has_nan ? sign << 31 : 0u;
    return nan ? __uint_as_float(kQuietNaN | s) : (inf ? __uint_as_float(0x7f800000u | s) : y);
}

// the block of a strided lane in packed order (< units)
__device__ __forceinline__ uint32_t packed_block(const MxWalk& j, const MxStridedPos& p) { return (p.o * j.inner.d + p.i) * j.nb.d + p.b; }

// ---- pack ----------------------------------------------------------------------------------------------------------------------
// The walk runs with NANBLOCK: a block that is NaN as a whole arrives with scale 0xFF under every rule, and its elements are +0
// like those a short last block lacks.
template <int U, int RULED>
__device__ __forceinline__ void pack_rows4(const MxPackJob& j, uint32_t local) {
    const MxFmt f = j.walk.fmt;                                                  // by value, like e and s: read once, ahead of every store
    const MxCoder c = make_coder(j.format, f);
    uint8_t* const e = j.e;
    uint8_t* const s = j.s;
    mx_rows4<U, false, RULED, true>(j.walk, j.f, local, [&](float v) { return mxp_mag(v, c); },
                                    [&](const MxRowPos& p, const float (&v)[4], uint32_t scale) {
        const bool dead = scale == 0xffu, live = p.ok && !dead;
        const float inv = mx_pow2(254u - (dead ? 0u : scale));
        const uint32_t c0 = live ? mxp_code(v[0], inv, f, c) : 0u, c1 = live ? mxp_code(v[1], inv, f, c) : 0u;
        const uint32_t c2 = live ? mxp_code(v[2], inv, f, c) : 0u, c3 = live ? mxp_code(v[3], inv, f, c) : 0u;
        const uint32_t mine = c0 | (c1 << c.bits) | (c2 << (2u * c.bits)) | (c3 << (3u * c.bits));      // 32 / 24 / 16 bits
        const uint32_t q = p.q;
        if (c.bits == 8u) {
            if (p.in) *reinterpret_cast<uint32_t*>(e + (size_t)p.g * 32u + q * 4u) = mine;
        } else if (c.bits == 4u) {
            const uint32_t next = (uint32_t)__shfl_xor((int)mine, 1, 64);
            if (p.in && !(q & 1u)) *reinterpret_cast<uint32_t*>(e + (size_t)p.g * 16u + q * 2u) = mine | (next << 16);
        } else {                                                                 // four lanes hold 12 bytes: lanes 0 .. 2 store a dword
            const uint32_t next = (uint32_t)__shfl_down((int)mine, 1, 64), t = q & 3u;
            const uint32_t word = (mine >> (8u * t)) | (next << (24u - 8u * t));
            if (p.in && t < 3u) *reinterpret_cast<uint32_t*>(e + (size_t)p.g * 24u + (q >> 2) * 12u + t * 4u) = word;
        }
        if (p.in && q == 0) s[p.g] = (uint8_t)scale;
    });
}

template <int RULED>
__device__ __forceinline__ void pack_rows1(const MxPackJob& j, uint32_t local) {
    const MxFmt f = j.walk.fmt;                                                  // by value, like e and s: read once, ahead of every store
    const MxCoder c = make_coder(j.format, f);
    uint8_t* const e = j.e;
    uint8_t* const s = j.s;
    mx_rows1<RULED, true>(j.walk, j.f, local, [&](float v) { return mxp_mag(v, c); },
                          [&](const MxRowPos& p, const float (&v)[1], uint32_t scale) {
        const bool dead = scale == 0xffu;
        const uint32_t mine = p.ok && !dead ? mxp_code(v[0], mx_pow2(254u - (dead ? 0u : scale)), f, c) : 0u;
        const uint32_t q = p.q;
        if (c.bits == 8u) {
            if (p.in) e[(size_t)p.g * 32u + q] = (uint8_t)mine;
        } else if (c.bits == 4u) {
            const uint32_t next = (uint32_t)__shfl_xor((int)mine, 1, 64);
            if (p.in && !(q & 1u)) e[(size_t)p.g * 16u + (q >> 1)] = (uint8_t)(mine | (next << 4));
        } else {                                                                 // four lanes hold 3 bytes: lanes 0 .. 2 store one
            const uint32_t next = (uint32_t)__shfl_down((int)mine, 1, 64), t = q & 3u;
            const uint32_t byte = (mine >> (2u * t)) | (next << (6u - 2u * t));
            if (p.in && t < 3u) e[(size_t)p.g * 24u + (q >> 2) * 3u + t] = (uint8_t)byte;
        }
        if (p.in && q == 0) s[p.g] = (uint8_t)scale;
    });
}

template <int BITS, bool BYTES, int RULED>
__device__ __forceinline__ void pack_strided(const MxPackJob& j, uint32_t local) {
    constexpr int NW = BITS;                                                     // dwords per block: 32 * BITS / 32
    const MxFmt f = j.walk.fmt;                                                  // by value, like e and s: read once, ahead of every store
    const MxCoder c = make_coder(j.format, f);
    uint8_t* const e = j.e;
    uint8_t* const s = j.s;
    mx_strided<RULED, true>(j.walk, j.f, local, [&](float v) { return mxp_mag(v, c); },
                            [&](const MxStridedPos& p, const float (&v)[kMxBlock], uint32_t scale) {
        const bool dead = scale == 0xffu;
        const float inv = mx_pow2(254u - (dead ? 0u : scale));
        uint32_t w[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] = 0u;
#pragma unroll
        for (uint32_t t = 0; t < kMxBlock; t++) {
            const uint32_t code = t < p.blen && !dead ? mxp_code(v[t], inv, f, c) : 0u;
            constexpr uint32_t kB = (uint32_t)BITS;
            const uint32_t at = t * kB, word = at >> 5, off = at & 31u;         // compile-time after unrolling
            w[word] |= code << off;
            if (off + kB > 32u) w[word + 1] |= code >> (32u - off);
        }
        const uint32_t blk = packed_block(j.walk, p);
        uint8_t* out = e + (size_t)blk * (4u * NW);
        if (BYTES) {
#pragma unroll
            for (int k = 0; k < 4 * NW; k++) out[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        } else if (NW == 6) {                                                    // 24-B blocks are 8-B aligned
#pragma unroll
            for (int k = 0; k < NW; k += 2) *reinterpret_cast<uint2*>(out + 4 * k) = make_uint2(w[k], w[k + 1]);
        } else {
#pragma unroll
            for (int k = 0; k < NW; k += 4) *reinterpret_cast<uint4*>(out + 4 * k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
        }
        s[blk] = (uint8_t)scale;
    });
}

// the strided body of either direction for the job's element width and store width (workgroup-uniform, like the path)
template <typename Body>
__device__ __forceinline__ void with_strided_stores(const MxPackJob& j, Body body) {
    const uint32_t bits = mx_elem_bits(j.format);
    if (!j.bytes) {
        if (bits == 8u) body(std::integral_constant<int, 8>(), std::false_type());
        else if (bits == 6u) body(std::integral_constant<int, 6>(), std::false_type());
        else body(std::integral_constant<int, 4>(), std::false_type());
    } else {
        if (bits == 8u) body(std::integral_constant<int, 8>(), std::true_type());
        else if (bits == 6u) body(std::integral_constant<int, 6>(), std::true_type());
        else body(std::integral_constant<int, 4>(), std::true_type());
    }
}

template <int CAP, int U, int RULED>
__global__ __launch_bounds__(kBlock) void mx_pack_kernel(const MxPackArgs<CAP> args) {
    uint32_t local;
    const MxPackJob& j = args.jobs[job_of(args, local)];
    if (j.walk.path == MX_ROWS4) pack_rows4<U, RULED>(j, local);
    else if (j.walk.path == MX_ROWS1) pack_rows1<RULED>(j, local);
    else with_strided_stores(j, [&](auto bits, auto bytes) { pack_strided<decltype(bits)::value, decltype(bytes)::value, RULED>(j, local); });
}

// ---- unpack --------------------------------------------------------------------------------------------------------------------
template <int U>
__device__ __forceinline__ void unpack_rows4(const MxPackJob& j, uint32_t local) {
    const MxCoder c = make_coder(j.format, j.walk.fmt);
    const MxFmt& f = j.walk.fmt;
    uint32_t mine[U], scale[U];                                                  // a lane's four codes; its block's scale
    MxRowPos p[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
        p[k] = mx_row_pos<4>(j.walk, local * U + k);
        const uint32_t g = p[k].g, q = p[k].q;
        if (c.bits == 8u) mine[k] = *reinterpret_cast<const uint32_t*>(j.e + (size_t)g * 32u + q * 4u);
        else if (c.bits == 4u) mine[k] = *reinterpret_cast<const uint16_t*>(j.e + (size_t)g * 16u + q * 2u);
        else {                                                                   // 3 bytes at q * 3: from the two dwords around them
            const uint32_t* words = reinterpret_cast<const uint32_t*>(j.e + (size_t)g * 24u);
            const uint32_t byte = q * 3u, w = byte >> 2;
            mine[k] = __funnelshift_r(words[w], words[min(w + 1u, 5u)], 8u * (byte & 3u)) & 0xffffffu;
        }
        scale[k] = j.s[g];
    }
    const uint32_t mask = (1u << c.bits) - 1u;
#pragma unroll
    for (int k = 0; k < U; k++) {
        const float X = mx_pow2(min(scale[k], 254u));
        const bool dead = scale[k] == 0xffu;
        float4 r;
        r.x = mxp_value(mine[k] & mask, X, dead, f, c);
        r.y = mxp_value((mine[k] >> c.bits) & mask, X, dead, f, c);
        r.z = mxp_value((mine[k] >> (2u * c.bits)) & mask, X, dead, f, c);
        r.w = mxp_value((mine[k] >> (3u * c.bits)) & mask, X, dead, f, c);
        if (p[k].ok) *reinterpret_cast<float4*>(j.f + p[k].at) = r;
    }
}

__device__ __forceinline__ void unpack_rows1(const MxPackJob& j, uint32_t local) {
    const MxCoder c = make_coder(j.format, j.walk.fmt);
    const MxFmt& f = j.walk.fmt;
    const MxRowPos p = mx_row_pos<1>(j.walk, local);
    const uint32_t B = 4u * c.bits, at = p.q * c.bits, k = at >> 3;
    const uint8_t* bytes = j.e + (size_t)p.g * B;
    const uint32_t two = (uint32_t)bytes[k] | ((uint32_t)bytes[min(k + 1u, B - 1u)] << 8);
    const uint32_t code = (two >> (at & 7u)) & ((1u << c.bits) - 1u);
    const uint32_t scale = j.s[p.g];
    const float r = mxp_value(code, mx_pow2(min(scale, 254u)), scale == 0xffu, f, c);
    if (p.ok) j.f[p.at] = r;
}

template <int BITS, bool BYTES>
__device__ __forceinline__ void unpack_strided(const MxPackJob& j, uint32_t local) {
    constexpr int NW = BITS;
    const MxCoder c = make_coder(j.format, j.walk.fmt);
    const MxFmt& f = j.walk.fmt;
    const MxStridedPos p = mx_strided_pos(j.walk, local);
    const uint32_t blk = packed_block(j.walk, p);
    const uint8_t* src = j.e + (size_t)blk * (4u * NW);
    uint32_t w[NW];
    if (BYTES) {
#pragma unroll
        for (int k = 0; k < NW; k++)
            w[k] = (uint32_t)src[4 * k] | ((uint32_t)src[4 * k + 1] << 8) | ((uint32_t)src[4 * k + 2] << 16) | ((uint32_t)src[4 * k + 3] << 24);
    } else if (NW == 6) {
#pragma unroll
        for (int k = 0; k < NW; k += 2) { const uint2 t = *reinterpret_cast<const uint2*>(src + 4 * k); w[k] = t.x; w[k + 1] = t.y; }
    } else {
#pragma unroll
        for (int k = 0; k < NW; k += 4) {
            const uint4 t = *reinterpret_cast<const uint4*>(src + 4 * k);
            w[k] = t.x; w[k + 1] = t.y; w[k + 2] = t.z; w[k + 3] = t.w;
        }
    }
    const uint32_t scale = j.s[blk];
    const float X = mx_pow2(min(scale, 254u));
    if (!p.in) return;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) {
        constexpr uint32_t kB = (uint32_t)BITS;
        const uint32_t at = t * kB, word = at >> 5, off = at & 31u;
        uint32_t code = w[word] >> off;
        if (off + kB > 32u) code |= w[word + 1] << (32u - off);
        if (t < p.blen) j.f[p.base + t * p.step] = mxp_value(code & ((1u << kB) - 1u), X, scale == 0xffu, f, c);
    }
}

template <int CAP, int U>
__global__ __launch_bounds__(kBlock) void mx_unpack_kernel(const MxPackArgs<CAP> args) {
    uint32_t local;
    const MxPackJob& j = args.jobs[job_of(args, local)];
    if (j.walk.path == MX_ROWS4) unpack_rows4<U>(j, local);
    else if (j.walk.path == MX_ROWS1) unpack_rows1(j, local);
    else with_strided_stores(j, [&](auto bits, auto bytes) { unpack_strided<decltype(bits)::value, decltype(bytes)::value>(j, local); });
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// one job of either direction, in the terms both share
struct MxPackView {
    const float* f;
    const uint8_t* e;
    const uint8_t* s;
    MxGeometry g;
    int arg;                                      // `format` as it came
    bool with_rule;                               // pack: a scale rule travels above the format; unpack makes no scales, so the
                                                  // whole argument is the format and a rule byte an unknown format
    int format() const { return arg & ((1 << PPQHIP_MX_RULE_SHIFT) - 1); }      // of a checked job
    int64_t block_bytes() const { return 4 * (int64_t)mx_elem_bits((uint32_t)format()); }
    double bytes() const { return 4.0 * (double)g.elems() + (double)g.codes() * (double)(block_bytes() + 1); }
};
MxPackView view_of(const ppqhip_mx_pack_job& j) { return MxPackView{j.x, j.elements, j.scales, mx_geometry_of(j), j.format, true}; }
MxPackView view_of(const ppqhip_mx_unpack_job& j) { return MxPackView{j.y, j.elements, j.scales, mx_geometry_of(j), j.format, false}; }

// No output shares memory with any other tensor of the call; there is no in-place form.
template <typename Job>
int validate(const char* what, bool packing, const Job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const MxPackView j = view_of(jobs[k]);
        if (int st = check_mx_job(what, k, j.arg, j.with_rule, j.g)) return st;
        if (j.g.empty()) continue;
        if (j.f == nullptr || j.e == nullptr || j.s == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        (packing ? ins : outs).push_back(span_of(j.f, j.g.elems()));
        (packing ? outs : ins).push_back(span_of(j.e, j.g.codes() * j.block_bytes()));
        (packing ? outs : ins).push_back(span_of(j.s, j.g.codes()));
    }
    return check_overlap(what, ins, outs);
}

// the device job and the workgroups it takes when a rows4 lane owns U float4
uint32_t device_job(const MxPackView& src, int U, MxPackJob* d, int* ruled) {
    d->f = const_cast<float*>(src.f); d->e = const_cast<uint8_t*>(src.e); d->s = const_cast<uint8_t*>(src.s);
    d->format = (uint16_t)src.format();
    d->bytes = aligned16(src.e) ? 0 : 1;
    return fill_mx_walk(&d->walk, src.g, src.arg, aligned16(src.f) && (reinterpret_cast<uintptr_t>(src.e) & 3u) == 0, U, ruled);
}

constexpr int64_t kMxSmallElems = 4ll << 20;      // latency-bound tensors: one float4 per rows4 lane, two above (see mx.hip)

template <typename Job>
int run(const char* what, bool packing, const Job* jobs, int num_jobs, void* stream) {
    if (int st = validate(what, packing, jobs, num_jobs)) return st;
    const auto live = live_mx_jobs(jobs, num_jobs);
    if (live.empty()) return PPQHIP_OK;
    double bytes = 0.0;
    for (const Job* j : live) bytes += view_of(*j).bytes();
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(packing ? K_MX_PACK : K_MX_UNPACK, bytes, s);
    const int U = live.size() > 1 || view_of(*live[0]).g.elems() <= kMxSmallElems ? 1 : 2;      // a table of many: one float4 per lane
    const auto fill = [&](const Job& src, MxPackJob* d, int* ruled) { return device_job(view_of(src), U, d, ruled); };
    const auto launch = [&](auto cap, auto u) {
        constexpr int CAP = decltype(cap)::value, UU = decltype(u)::value;
        return launch_mx_jobs<MxPackArgs<CAP>>(what, live, fill, [&](int ruled, uint32_t blocks, const MxPackArgs<CAP>& args) {
            if (packing) with_mx_ruled(ruled, [&](auto R) { hipLaunchKernelGGL((mx_pack_kernel<CAP, UU, decltype(R)::value>), dim3(blocks), dim3(kBlock), 0, s, args); });
            else hipLaunchKernelGGL((mx_unpack_kernel<CAP, UU>), dim3(blocks), dim3(kBlock), 0, s, args);
        });
    };
    if (live.size() > 1) return launch(std::integral_constant<int, kMxMaxJobs>(), std::integral_constant<int, 1>());
    if (U == 2) return launch(std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
    return launch(std::integral_constant<int, 1>(), std::integral_constant<int, 1>());
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_mx_pack(const float* x, uint8_t* elements, uint8_t* scales, int64_t outer, int64_t axis_len, int64_t inner, int format,
                   void* stream) {
    ppqhip_mx_pack_job job;
    job.x = x; job.elements = elements; job.scales = scales;
    job.outer = outer; job.axis_len = axis_len; job.inner = inner; job.format = format; job.reserved = 0;
    return run("mx_pack", true, &job, 1, stream);
}

int ppqhip_mx_pack_multi(const ppqhip_mx_pack_job* jobs, int num_jobs, void* stream) {
    return run("mx_pack_multi", true, jobs, num_jobs, stream);
}

int ppqhip_mx_unpack(const uint8_t* elements, const uint8_t* scales, float* y, int64_t outer, int64_t axis_len, int64_t inner,
                     int format, void* stream) {
    ppqhip_mx_unpack_job job;
    job.elements = elements; job.scales = scales; job.y = y;
    job.outer = outer; job.axis_len = axis_len; job.inner = inner; job.format = format; job.reserved = 0;
    return run("mx_unpack", false, &job, 1, stream);
}

int ppqhip_mx_unpack_multi(const ppqhip_mx_unpack_job* jobs, int num_jobs, void* stream) {
    return run("mx_unpack_multi", false, jobs, num_jobs, stream);
}

}  // extern "C"
