// mx_mfma.hpp -- what the kernels on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4) share: mx_gemm.hip and
// mx_conv.hip.  The workgroup shape, the instruction's format ids, how a lane's operand registers and scale byte are read from an
// operand packed along its last axis (DESIGN.md sections 9.13, 9.14), the NaN flags and the format check of the entry points.
#pragma once

#include "common.hpp"
#include "mx_common.hpp"

namespace ppqhip {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kGemmTile = 16;                     // one MFMA's rows and columns
constexpr int kGemmWaveTiles = 2;                 // a wave owns kGemmWaveTiles^2 MFMA tiles ...
constexpr int kGemmWaves = 2;                     // ... and a workgroup kGemmWaves^2 waves
constexpr int kGemmEdge = kGemmTile * kGemmWaveTiles * kGemmWaves;       // 64: rows and columns of C per workgroup
constexpr uint32_t kGemmStepBlocks = 4;           // MX blocks of one row per instruction (K = 128)
static_assert(kGemmWaves * kGemmWaves * kWave == kBlock, "four waves per workgroup");

__host__ __device__ constexpr uint32_t gemm_elem_bits(int format) {
    return format == PPQHIP_MXFP4_E2M1 ? 4u : (format == PPQHIP_MXFP6_E3M2 || format == PPQHIP_MXFP6_E2M3) ? 6u : 8u;
}
// the instruction's format ids (cbsz for A, blgp for B): 0 E4M3, 1 E5M2, 2 E2M3, 3 E3M2, 4 E2M1 -- the two FP6 ids are the other way
// round in PPQHIP_MX*
__host__ __device__ constexpr int gemm_hw_format(int format) {
    return format == PPQHIP_MXFP6_E3M2 ? 3 : format == PPQHIP_MXFP6_E2M3 ? 2 : format;
}

// a dword of FP8 codes holds a NaN: E4M3 S.1111.111 (0x7f under the sign), E5M2 S.11111.{01, 10, 11} (0x7d .. 0x7f); the add
// carries into bit 7 of exactly those bytes and never into the next byte
template <int F>
__device__ __forceinline__ uint32_t fp8_nan_bits(uint32_t w) {
    return ((w & 0x7f7f7f7fu) + (F == PPQHIP_MXFP8_E4M3 ? 0x01010101u : 0x03030303u)) & 0x80808080u;
}

// The lane's operand registers of format F for K-step `kb0 / 4` of the row that starts at e: FP6 / FP4 lanes hold block kb0 + grp,
// its bytes in the low dwords; an FP8 lane holds bytes [16 (grp & 1), + 16) of block kb0 + (grp >> 1) in dwords 0 .. 3 and the same
// bytes of block kb0 + 2 + (grp >> 1) in dwords 4 .. 7.  TAIL: a block at or past nb is not read (the load is clamped) and gives zeros.
template <int F, bool TAIL>
__device__ __forceinline__ v8i load_fragment(const uint8_t* e, uint32_t kb0, uint32_t grp, uint32_t nb) {
    constexpr uint32_t bits = gemm_elem_bits(F);
    v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (bits == 8u) {
        const uint32_t b0 = kb0 + (grp >> 1), b1 = b0 + 2u, half = 16u * (grp & 1u);
        const bool live0 = !TAIL || b0 < nb, live1 = !TAIL || b1 < nb;
        uint4 lo = *reinterpret_cast<const uint4*>(e + (size_t)(TAIL ? min(b0, nb - 1u) : b0) * 32u + half);
        uint4 hi = *reinterpret_cast<const uint4*>(e + (size_t)(TAIL ? min(b1, nb - 1u) : b1) * 32u + half);
        if (!live0) lo = make_uint4(0u, 0u, 0u, 0u);
        if (!live1) hi = make_uint4(0u, 0u, 0u, 0u);
        r[0] = (int)lo.x; r[1] = (int)lo.y; r[2] = (int)lo.z; r[3] = (int)lo.w;
        r[4] = (int)hi.x; r[5] = (int)hi.y; r[6] = (int)hi.z; r[7] = (int)hi.w;
    } else {
        const uint32_t kb = kb0 + grp;
        const bool live = !TAIL || kb < nb;
        const uint8_t* p = e + (size_t)(TAIL ? min(kb, nb - 1u) : kb) * (4u * bits);
        if (bits == 6u) {                                                        // 24-B blocks are 8-B aligned
            const uint2 t0 = *reinterpret_cast<const uint2*>(p), t1 = *reinterpret_cast<const uint2*>(p + 8), t2 = *reinterpret_cast<const uint2*>(p + 16);
            r[0] = (int)t0.x; r[1] = (int)t0.y; r[2] = (int)t1.x; r[3] = (int)t1.y; r[4] = (int)t2.x; r[5] = (int)t2.y;
        } else {
            const uint4 lo = *reinterpret_cast<const uint4*>(p);
            r[0] = (int)lo.x; r[1] = (int)lo.y; r[2] = (int)lo.z; r[3] = (int)lo.w;
        }
        if (!live) r = v8i{0, 0, 0, 0, 0, 0, 0, 0};
    }
    return r;
}

// one operand's fragments of a K-step: for each of the wave's kGemmWaveTiles rows (columns) of this lane, the registers above and the
// scale code of block kb0 + grp (127 past nb).  The lane's NaN flag takes the scale code 0xFF and the FP8 NaN codes it has loaded.
template <int F, bool TAIL>
__device__ __forceinline__ void load_operand(const uint8_t* const (&e)[kGemmWaveTiles], const uint8_t* const (&s)[kGemmWaveTiles], uint32_t kb0,
                                             uint32_t grp, uint32_t nb, v8i (&frag)[kGemmWaveTiles], int (&scale)[kGemmWaveTiles],
                                             uint32_t (&nan)[kGemmWaveTiles]) {
    const uint32_t kb = kb0 + grp;
    const bool live = !TAIL || kb < nb;
#pragma unroll
    for (int t = 0; t < kGemmWaveTiles; t++) {
        frag[t] = load_fragment<F, TAIL>(e[t], kb0, grp, nb);
        scale[t] = (int)s[t][TAIL ? min(kb, nb - 1u) : kb];
    }
#pragma unroll
    for (int t = 0; t < kGemmWaveTiles; t++) {
        if (!live) scale[t] = 127;
        uint32_t bad = scale[t] == 0xff ? 1u : 0u;
        if (F == PPQHIP_MXFP8_E4M3 || F == PPQHIP_MXFP8_E5M2) {
#pragma unroll
            for (int w = 0; w < 8; w++) bad |= fp8_nan_bits<F>((uint32_t)frag[t][w]);
        }
        nan[t] |= bad;
    }
}

// the flags of the 16 rows (columns) of a tile from the lanes' own: a row is owned by the four lanes r, r + 16, r + 32, r + 48
__device__ __forceinline__ uint32_t tile_flags(uint32_t lane_flag) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(lane_flag != 0u);
    return (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffull);
}

inline int check_format(const char* what, const char* operand, int format) {
    if (format == PPQHIP_MXINT8) { set_error("%s: %s: MXINT8 is not an operand type of the scaled MFMA", what, operand); return PPQHIP_ERR_INVALID_VALUE; }
    if (format < PPQHIP_MXFP8_E4M3 || format > PPQHIP_MXFP4_E2M1) { set_error("%s: %s: unknown MX format %d", what, operand, format); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

}  // namespace ppqhip
