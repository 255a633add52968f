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
// One kernel per direction behind a job table (job_table.hpp), three bodies each, as in mx.hip:
//   rows4   inner == 1, float side 16-B aligned, axis_len % 4 == 0, packed side 4-B aligned: eight lanes per block, one float4
//           each; a lane's four codes are 4 / 3 / 2 bytes, lanes are combined through shuffles so that every store is one dword
//           (FP6: three lanes of four store; FP4: every other lane); two float4 per lane above 4 M elements, as in mx.hip
//   rows1   inner == 1 otherwise: one element per lane, byte stores
//   strided inner > 1: one lane per (outer, block, inner), inner fastest, with the 32 values in registers; the lane owns the B bytes of its
//           block (16-B stores, 8-B for the 24-B blocks of FP6; bytes when `elements` is not 16-B aligned).  This is where the axis
//           moves last.  The loads are coalesced along inner, as in mx.hip.
// Pack takes the block's scale by the job's scale rule exactly as mx.hip does, from the same function of
// mx_common.hpp; unpack reads scales as stored and knows no rule.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_coder.hpp"
#include "mx_common.hpp"

namespace ppqhip {
namespace {

enum : uint32_t { MXP_ROWS4 = 0, MXP_ROWS1 = 1, MXP_STRIDED = 2, MXP_STRIDED_BYTES = 3 };

struct MxPackJob {                                // 96 B; pack: f -> e, s; unpack: e, s -> f
    float* f;                                     // the float32 tensor, [outer, axis_len, inner]
    uint8_t* e;                                   // elements
    uint8_t* s;                                   // scales
    uint32_t len;                                 // axis_len
    uint32_t units;                               // blocks: outer * inner * blocks per row
    FastDiv nb;                                   // blocks per row
    FastDiv inner;
    uint32_t path;
    uint32_t format;
    MxFmt fmt;
    uint32_t rule;                                // pack: PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE, read by the RULED instantiations only
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

// ---- pack ----------------------------------------------------------------------------------------------------------------------
// RULED (MX_PLAIN / MX_AMAX_RULES / MX_SEARCH): the instantiations above MX_PLAIN take the block's code from the job's scale rule
// (mx_common.hpp), as in mx.hip; the plain ones are the floor rule's and keep their code.  A block that is NaN as a whole keeps scale 0xFF under every rule.
__device__ __forceinline__ uint32_t ruled_scale(uint32_t code, bool dead, float& inv) {
    inv = mx_pow2(254u - code);
    return dead ? 0xffu : code;
}

template <int U, int RULED>
__device__ __forceinline__ void pack_rows4(const MxPackJob& j, uint32_t local) {
    constexpr uint32_t kGroups = kBlock / 8;                                     // blocks per workgroup and step
    const MxCoder c = make_coder(j.format, j.fmt);
    const uint32_t q = threadIdx.x & 7u;
    float4 a[U];
    uint32_t g[U];
    bool in[U], ok[U];
#pragma unroll
    for (int k = 0; k < U; k++) {                                                // clamped, branch-free: all U loads issue back to back
        const uint32_t want = (local * U + k) * kGroups + (threadIdx.x >> 3);
        in[k] = want < j.units;
        g[k] = min(want, j.units - 1);
        const uint32_t row = fdiv(g[k], j.nb), b = g[k] - row * j.nb.d;
        const uint32_t e = b * kMxBlock + q * 4;
        ok[k] = in[k] && e < j.len;                                              // len % 4 == 0: a float4 is inside the row or outside
        a[k] = *reinterpret_cast<const float4*>(j.f + (size_t)row * j.len + (e < j.len ? e : b * kMxBlock));
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
        uint32_t m = max(max(mxp_mag(a[k].x, c), mxp_mag(a[k].y, c)), max(mxp_mag(a[k].z, c), mxp_mag(a[k].w, c)));
        m = ok[k] ? m : 0u;
        m = max(m, (uint32_t)__shfl_xor((int)m, 4, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
        float inv; bool dead;
        uint32_t scale = mxp_scale(m, j.fmt, inv, dead);
        if constexpr (RULED != MX_PLAIN) {
            uint32_t code = mx_rule_code(dead ? 0u : m, j.fmt, j.rule);
            if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {              // workgroup-uniform
                MxMse s(code);
                s.add(a[k].x, ok[k], j.fmt); s.add(a[k].y, ok[k], j.fmt); s.add(a[k].z, ok[k], j.fmt); s.add(a[k].w, ok[k], j.fmt);
                s.reduce<8>();
                code = s.code();
            }
            scale = ruled_scale(code, dead, inv);
        }
        const bool live = ok[k] && !dead;                                        // padding and NaN blocks: +0
        const uint32_t c0 = live ? mxp_code(a[k].x, inv, j.fmt, c) : 0u, c1 = live ? mxp_code(a[k].y, inv, j.fmt, c) : 0u;
        const uint32_t c2 = live ? mxp_code(a[k].z, inv, j.fmt, c) : 0u, c3 = live ? mxp_code(a[k].w, inv, j.fmt, c) : 0u;
        const uint32_t mine = c0 | (c1 << c.bits) | (c2 << (2u * c.bits)) | (c3 << (3u * c.bits));  // 32 / 24 / 16 bits
        if (c.bits == 8u) {
            if (in[k]) *reinterpret_cast<uint32_t*>(j.e + (size_t)g[k] * 32u + q * 4u) = mine;
        } else if (c.bits == 4u) {
            const uint32_t next = (uint32_t)__shfl_xor((int)mine, 1, 64);
            if (in[k] && !(q & 1u)) *reinterpret_cast<uint32_t*>(j.e + (size_t)g[k] * 16u + q * 2u) = mine | (next << 16);
        } else {                                                                 // four lanes hold 12 bytes: lanes 0 .. 2 store a dword
            const uint32_t next = (uint32_t)__shfl_down((int)mine, 1, 64), t = q & 3u;
            const uint32_t word = (mine >> (8u * t)) | (next << (24u - 8u * t));
            if (in[k] && t < 3u) *reinterpret_cast<uint32_t*>(j.e + (size_t)g[k] * 24u + (q >> 2) * 12u + t * 4u) = word;
        }
        if (in[k] && q == 0) j.s[g[k]] = (uint8_t)scale;
    }
}

template <int RULED>
__device__ __forceinline__ void pack_rows1(const MxPackJob& j, uint32_t local) {
    const MxCoder c = make_coder(j.format, j.fmt);
    const uint32_t q = threadIdx.x & 31u;
    const uint32_t want = local * (kBlock / kMxBlock) + (threadIdx.x >> 5);
    const bool in = want < j.units;
    const uint32_t g = min(want, j.units - 1);
    const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + q;
    const bool ok = in && e < j.len;
    const float v = j.f[(size_t)row * j.len + (e < j.len ? e : b * kMxBlock)];
    uint32_t m = ok ? mxp_mag(v, c) : 0u;
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    float inv; bool dead;
    uint32_t scale = mxp_scale(m, j.fmt, inv, dead);
    if constexpr (RULED != MX_PLAIN) {
        uint32_t code = mx_rule_code(dead ? 0u : m, j.fmt, j.rule);
        if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {
            MxMse s(code);
            s.add(v, ok, j.fmt);
            s.reduce<32>();
            code = s.code();
        }
        scale = ruled_scale(code, dead, inv);
    }
    const uint32_t mine = ok && !dead ? mxp_code(v, inv, j.fmt, c) : 0u;
    if (c.bits == 8u) {
        if (in) j.e[(size_t)g * 32u + q] = (uint8_t)mine;
    } else if (c.bits == 4u) {
        const uint32_t next = (uint32_t)__shfl_xor((int)mine, 1, 64);
        if (in && !(q & 1u)) j.e[(size_t)g * 16u + (q >> 1)] = (uint8_t)(mine | (next << 4));
    } else {                                                                     // four lanes hold 3 bytes: lanes 0 .. 2 store one
        const uint32_t next = (uint32_t)__shfl_down((int)mine, 1, 64), t = q & 3u;
        const uint32_t byte = (mine >> (2u * t)) | (next << (6u - 2u * t));
        if (in && t < 3u) j.e[(size_t)g * 24u + (q >> 2) * 3u + t] = (uint8_t)byte;
    }
    if (in && q == 0) j.s[g] = (uint8_t)scale;
}

// the lane of a strided job: lanes are numbered over (outer, block, inner) with inner fastest, for the loads; `blk` =
// (o * inner + i) * nb + b is the lane's block in packed order
struct MxLane {
    bool in;
    uint32_t blk, blen;
    size_t base, step;
};
__device__ __forceinline__ MxLane strided_lane(const MxPackJob& j, uint32_t local) {
    MxLane l;
    const uint32_t want = local * kBlock + threadIdx.x;
    l.in = want < j.units;
    const uint32_t w = min(want, j.units - 1);
    const uint32_t ob = fdiv(w, j.inner), i = w - ob * j.inner.d;                // w = (o * nb + b) * inner + i
    const uint32_t o = fdiv(ob, j.nb), b = ob - o * j.nb.d;
    l.blen = min(kMxBlock, j.len - b * kMxBlock);                                // >= 1
    l.base = ((size_t)o * j.len + (size_t)b * kMxBlock) * j.inner.d + i;
    l.step = j.inner.d;
    l.blk = (o * j.inner.d + i) * j.nb.d + b;                                    // < units
    return l;
}

template <int BITS, bool BYTES, int RULED>
__device__ __forceinline__ void pack_strided(const MxPackJob& j, uint32_t local) {
    constexpr int NW = BITS;                                                     // dwords per block: 32 * BITS / 32
    const MxCoder c = make_coder(j.format, j.fmt);
    const MxLane l = strided_lane(j, local);
    float v[kMxBlock];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) v[t] = j.f[l.base + min(t, l.blen - 1) * l.step];      // clamped: 32 loads in flight
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) m = max(m, t < l.blen ? mxp_mag(v[t], c) : 0u);
    float inv; bool dead;
    uint32_t scale = mxp_scale(m, j.fmt, inv, dead);
    if constexpr (RULED != MX_PLAIN) {
        uint32_t code = mx_rule_code(dead ? 0u : m, j.fmt, j.rule);
        if (RULED == MX_SEARCH && j.rule == PPQHIP_MX_MSE) {
            MxMse s(code);
#pragma unroll
            for (uint32_t t = 0; t < kMxBlock; t++) s.add(v[t], t < l.blen, j.fmt);
            code = s.code();
        }
        scale = ruled_scale(code, dead, inv);
    }
    if (!l.in) return;
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = 0u;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) {
        const uint32_t code = t < l.blen && !dead ? mxp_code(v[t], inv, j.fmt, c) : 0u;
        constexpr uint32_t kB = (uint32_t)BITS;
        const uint32_t at = t * kB, word = at >> 5, off = at & 31u;             // compile-time after unrolling
        w[word] |= code << off;
        if (off + kB > 32u) w[word + 1] |= code >> (32u - off);
    }
    uint8_t* out = j.e + (size_t)l.blk * (4u * NW);
    if (BYTES) {
#pragma unroll
        for (int k = 0; k < 4 * NW; k++) out[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    } else if (NW == 6) {                                                        // 24-B blocks are 8-B aligned
#pragma unroll
        for (int k = 0; k < NW; k += 2) *reinterpret_cast<uint2*>(out + 4 * k) = make_uint2(w[k], w[k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < NW; k += 4) *reinterpret_cast<uint4*>(out + 4 * k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
    }
    j.s[l.blk] = (uint8_t)scale;
}

template <int CAP, int U, int RULED>
__global__ __launch_bounds__(kBlock) void mx_pack_kernel(const MxPackArgs<CAP> args) {
    uint32_t local;
    const MxPackJob& j = args.jobs[job_of(args, local)];
    const uint32_t bits = mx_elem_bits(j.format);                                // workgroup-uniform, like the path
    if (j.path == MXP_ROWS4) pack_rows4<U, RULED>(j, local);
    else if (j.path == MXP_ROWS1) pack_rows1<RULED>(j, local);
    else if (j.path == MXP_STRIDED) {
        if (bits == 8u) pack_strided<8, false, RULED>(j, local);
        else if (bits == 6u) pack_strided<6, false, RULED>(j, local);
        else pack_strided<4, false, RULED>(j, local);
    } else {
        if (bits == 8u) pack_strided<8, true, RULED>(j, local);
        else if (bits == 6u) pack_strided<6, true, RULED>(j, local);
        else pack_strided<4, true, RULED>(j, local);
    }
}

template <int CAP, int U>
void launch_pack(int ruled, uint32_t blocks, hipStream_t s, const MxPackArgs<CAP>& args) {
    if (ruled == MX_SEARCH) hipLaunchKernelGGL((mx_pack_kernel<CAP, U, MX_SEARCH>), dim3(blocks), dim3(kBlock), 0, s, args);
    else if (ruled == MX_AMAX_RULES) hipLaunchKernelGGL((mx_pack_kernel<CAP, U, MX_AMAX_RULES>), dim3(blocks), dim3(kBlock), 0, s, args);
    else hipLaunchKernelGGL((mx_pack_kernel<CAP, U, MX_PLAIN>), dim3(blocks), dim3(kBlock), 0, s, args);
}

// ---- unpack --------------------------------------------------------------------------------------------------------------------
template <int U>
__device__ __forceinline__ void unpack_rows4(const MxPackJob& j, uint32_t local) {
    constexpr uint32_t kGroups = kBlock / 8;
    const MxCoder c = make_coder(j.format, j.fmt);
    const uint32_t q = threadIdx.x & 7u;
    uint32_t mine[U], scale[U];                                                  // a lane's four codes; its block's scale
    size_t at[U];
    bool ok[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
        const uint32_t want = (local * U + k) * kGroups + (threadIdx.x >> 3);
        const uint32_t g = min(want, j.units - 1);
        const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
        const uint32_t e = b * kMxBlock + q * 4;
        ok[k] = want < j.units && e < j.len;
        at[k] = (size_t)row * j.len + e;
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
        r.x = mxp_value(mine[k] & mask, X, dead, j.fmt, c);
        r.y = mxp_value((mine[k] >> c.bits) & mask, X, dead, j.fmt, c);
        r.z = mxp_value((mine[k] >> (2u * c.bits)) & mask, X, dead, j.fmt, c);
        r.w = mxp_value((mine[k] >> (3u * c.bits)) & mask, X, dead, j.fmt, c);
        if (ok[k]) *reinterpret_cast<float4*>(j.f + at[k]) = r;
    }
}

__device__ __forceinline__ void unpack_rows1(const MxPackJob& j, uint32_t local) {
    const MxCoder c = make_coder(j.format, j.fmt);
    const uint32_t q = threadIdx.x & 31u;
    const uint32_t want = local * (kBlock / kMxBlock) + (threadIdx.x >> 5);
    const bool in = want < j.units;
    const uint32_t g = min(want, j.units - 1);
    const uint32_t row = fdiv(g, j.nb), b = g - row * j.nb.d;
    const uint32_t e = b * kMxBlock + q;
    const uint32_t B = 4u * c.bits, at = q * c.bits, k = at >> 3;
    const uint8_t* bytes = j.e + (size_t)g * B;
    const uint32_t two = (uint32_t)bytes[k] | ((uint32_t)bytes[min(k + 1u, B - 1u)] << 8);
    const uint32_t code = (two >> (at & 7u)) & ((1u << c.bits) - 1u);
    const uint32_t scale = j.s[g];
    const float r = mxp_value(code, mx_pow2(min(scale, 254u)), scale == 0xffu, j.fmt, c);
    if (in && e < j.len) j.f[(size_t)row * j.len + e] = r;
}

template <int BITS, bool BYTES>
__device__ __forceinline__ void unpack_strided(const MxPackJob& j, uint32_t local) {
    constexpr int NW = BITS;
    const MxCoder c = make_coder(j.format, j.fmt);
    const MxLane l = strided_lane(j, local);
    const uint8_t* src = j.e + (size_t)l.blk * (4u * NW);
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
    const uint32_t scale = j.s[l.blk];
    const float X = mx_pow2(min(scale, 254u));
    if (!l.in) return;
#pragma unroll
    for (uint32_t t = 0; t < kMxBlock; t++) {
        constexpr uint32_t kB = (uint32_t)BITS;
        const uint32_t at = t * kB, word = at >> 5, off = at & 31u;
        uint32_t code = w[word] >> off;
        if (off + kB > 32u) code |= w[word + 1] << (32u - off);
        if (t < l.blen) j.f[l.base + t * l.step] = mxp_value(code & ((1u << kB) - 1u), X, scale == 0xffu, j.fmt, c);
    }
}

template <int CAP, int U>
__global__ __launch_bounds__(kBlock) void mx_unpack_kernel(const MxPackArgs<CAP> args) {
    uint32_t local;
    const MxPackJob& j = args.jobs[job_of(args, local)];
    const uint32_t bits = mx_elem_bits(j.format);
    if (j.path == MXP_ROWS4) unpack_rows4<U>(j, local);
    else if (j.path == MXP_ROWS1) unpack_rows1(j, local);
    else if (j.path == MXP_STRIDED) {
        if (bits == 8u) unpack_strided<8, false>(j, local);
        else if (bits == 6u) unpack_strided<6, false>(j, local);
        else unpack_strided<4, false>(j, local);
    } else {
        if (bits == 8u) unpack_strided<8, true>(j, local);
        else if (bits == 6u) unpack_strided<6, true>(j, local);
        else unpack_strided<4, true>(j, local);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// one job of either direction, in the terms both share
struct MxPackView {
    const float* f;
    const uint8_t* e;
    const uint8_t* s;
    int64_t outer, axis_len, inner;
    int format;                                   // the format alone
    uint32_t rule;                                // pack: the scale rule that travelled above it
    bool known;                                   // false: `format` is the argument as it came, with a rule nobody knows
    int64_t nb() const { return (axis_len + kMxBlock - 1) / kMxBlock; }
    int64_t elems() const { return outer * axis_len * inner; }
    int64_t blocks() const { return outer * inner * nb(); }
    int64_t block_bytes() const { return 4 * (int64_t)mx_elem_bits((uint32_t)format); }
    bool empty() const { return outer == 0 || axis_len == 0 || inner == 0; }
    double bytes() const { return 4.0 * (double)elems() + (double)blocks() * (double)(block_bytes() + 1); }
};
MxPackView view_of(const ppqhip_mx_pack_job& j) {
    MxPackView v{j.x, j.elements, j.scales, j.outer, j.axis_len, j.inner, j.format, PPQHIP_MX_FLOOR, false};
    v.known = split_mx_format(j.format, &v.format, &v.rule);
    return v;
}
// unpack makes no scales: the whole argument is the format, so that a rule byte is an unknown format
MxPackView view_of(const ppqhip_mx_unpack_job& j) { return MxPackView{j.y, j.elements, j.scales, j.outer, j.axis_len, j.inner, j.format, PPQHIP_MX_FLOOR, true}; }

int validate_job(const char* what, int k, const MxPackView& j) {
    MxFmt probe;
    if (!j.known) { set_error("%s: job %d: unknown MX scale rule in format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
    if (!make_mx_fmt(j.format, &probe)) { set_error("%s: job %d: unknown MX format %d", what, k, j.format); return PPQHIP_ERR_INVALID_VALUE; }
    if (j.outer < 0 || j.axis_len < 0 || j.inner < 0) { set_error("%s: job %d: negative size", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    if (j.empty()) return PPQHIP_OK;
    if (j.outer > kMxMax || j.axis_len > kMxMax || j.inner > kMxMax || j.outer * j.axis_len > kMxMax || j.elems() > kMxMax) {
        set_error("%s: job %d: more than 2^31 - 1 elements", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (j.f == nullptr || j.e == nullptr || j.s == nullptr) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

// No output shares memory with any other tensor of the call; there is no in-place form.
template <typename Job>
int validate(const char* what, bool packing, const Job* jobs, int num_jobs) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    std::vector<Span> ins, outs;
    for (int k = 0; k < num_jobs; k++) {
        const MxPackView j = view_of(jobs[k]);
        if (int st = validate_job(what, k, j)) return st;
        if (j.empty()) continue;
        (packing ? ins : outs).push_back(span_of(j.f, j.elems()));
        (packing ? outs : ins).push_back(span_of(j.e, j.blocks() * j.block_bytes()));
        (packing ? outs : ins).push_back(span_of(j.s, j.blocks()));
    }
    return check_overlap(what, ins, outs);
}

// the device job and the workgroups it takes when a rows4 lane owns U float4; *ruled is raised to the class of the job's rule
uint32_t device_job(const MxPackView& src, int U, MxPackJob* d, int* ruled) {
    d->f = const_cast<float*>(src.f); d->e = const_cast<uint8_t*>(src.e); d->s = const_cast<uint8_t*>(src.s);
    d->len = (uint32_t)src.axis_len;
    d->nb = make_fastdiv((uint32_t)src.nb());
    d->inner = make_fastdiv((uint32_t)src.inner);
    d->format = (uint32_t)src.format;
    d->rule = src.rule;
    *ruled = std::max(*ruled, mx_rule_class(src.rule));
    make_mx_fmt(src.format, &d->fmt);
    const int64_t units = src.blocks();                                          // <= elements <= 2^31 - 1
    d->units = (uint32_t)units;
    int64_t per;
    if (src.inner > 1) { d->path = aligned16(src.e) ? MXP_STRIDED : MXP_STRIDED_BYTES; per = kBlock; }
    else if (aligned16(src.f) && src.axis_len % 4 == 0 && (reinterpret_cast<uintptr_t>(src.e) & 3u) == 0) { d->path = MXP_ROWS4; per = (int64_t)(kBlock / 8) * U; }
    else { d->path = MXP_ROWS1; per = kBlock / kMxBlock; }
    return (uint32_t)((units + per - 1) / per);
}

constexpr int64_t kMxSmallElems = 4ll << 20;      // latency-bound tensors: one float4 per rows4 lane, two above (see mx.hip)

template <typename Job>
int run(const char* what, bool packing, const Job* jobs, int num_jobs, void* stream) {
    if (int st = validate(what, packing, jobs, num_jobs)) return st;
    std::vector<MxPackView> live;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const MxPackView j = view_of(jobs[k]);
        if (j.empty()) continue;
        live.push_back(j);
        bytes += j.bytes();
    }
    if (live.empty()) return PPQHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(packing ? K_MX_PACK : K_MX_UNPACK, bytes, s);
    if (live.size() == 1) {
        MxPackArgs<1> args;
        const int U = live[0].elems() <= kMxSmallElems ? 1 : 2;
        int ruled = MX_PLAIN;
        const uint32_t blocks = device_job(live[0], U, &args.jobs[0], &ruled);
        args.first_block[0] = 0;
        args.count = 1;
        if (packing && U == 2) launch_pack<1, 2>(ruled, blocks, s, args);
        else if (packing) launch_pack<1, 1>(ruled, blocks, s, args);
        else if (U == 2) hipLaunchKernelGGL((mx_unpack_kernel<1, 2>), dim3(blocks), dim3(kBlock), 0, s, args);
        else hipLaunchKernelGGL((mx_unpack_kernel<1, 1>), dim3(blocks), dim3(kBlock), 0, s, args);
        return finish_launch(what);
    }
    for (size_t base = 0; base < live.size(); base += kMxMaxJobs) {
        MxPackArgs<kMxMaxJobs> args;
        const uint32_t count = (uint32_t)std::min<size_t>(kMxMaxJobs, live.size() - base);
        uint64_t blocks = 0;
        int ruled = MX_PLAIN;
        for (uint32_t k = 0; k < count; k++) {
            args.first_block[k] = (uint32_t)blocks;
            blocks += device_job(live[base + k], 1, &args.jobs[k], &ruled);
        }
        if (blocks > (uint64_t)kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
        pad_job_table(args, count, (uint32_t)blocks);
        if (packing) launch_pack<kMxMaxJobs, 1>(ruled, (uint32_t)blocks, s, args);
        else hipLaunchKernelGGL((mx_unpack_kernel<kMxMaxJobs, 1>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
    }
    return finish_launch(what);
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
