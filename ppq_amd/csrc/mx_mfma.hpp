// mx_mfma.hpp -- what the kernels on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4) share: mx_gemm.hip and
// mx_conv.hip.  The workgroup shape, the instruction's format ids, how a lane's operand registers and scale byte are read from an
// operand packed along its last axis (DESIGN.md sections 9.13, 9.14), the NaN flags, the A / B operand sources and the K-step (section
// 4.4), the fused epilogue (residual, ReLU, MX re-quantisation of the result; section 9.16) and the host frame of the entry points: the
// format check, the fused accounting, the format dispatch and the launch.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "job_table.hpp"
#include "mx_coder.hpp"
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

// ---- a lane's operand registers ------------------------------------------------------------------------------------------------------
// The register layout of a fragment, once.  Whoever calls these computes addresses and liveness: the load is always issued, from
// an address that is readable, and zeros are selected afterwards where the block is not live -- that is what makes padding, and
// blocks past nb, safe to "read".
// FP8: bytes [16 (grp & 1), + 16) of block kb0 + (grp >> 1) at p0 in dwords 0 .. 3, the same bytes of block kb0 + 2 + (grp >> 1) at p1
// in dwords 4 .. 7.
__device__ __forceinline__ v8i fp8_fragment(const uint8_t* p0, const uint8_t* p1, bool live0, bool live1) {
    uint4 lo = *reinterpret_cast<const uint4*>(p0), hi = *reinterpret_cast<const uint4*>(p1);
    if (!live0) lo = make_uint4(0u, 0u, 0u, 0u);
    if (!live1) hi = make_uint4(0u, 0u, 0u, 0u);
    return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}
// FP6 / FP4: the 24 / 16 bytes of block kb0 + grp at p in the low dwords
template <int F>
__device__ __forceinline__ v8i block_fragment(const uint8_t* p, bool live) {
    v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (gemm_elem_bits(F) == 6u) {                                               // 24-B blocks are 8-B aligned
        const uint2 t0 = *reinterpret_cast<const uint2*>(p), t1 = *reinterpret_cast<const uint2*>(p + 8), t2 = *reinterpret_cast<const uint2*>(p + 16);
        r[0] = (int)t0.x; r[1] = (int)t0.y; r[2] = (int)t1.x; r[3] = (int)t1.y; r[4] = (int)t2.x; r[5] = (int)t2.y;
    } else {
        const uint4 lo = *reinterpret_cast<const uint4*>(p);
        r[0] = (int)lo.x; r[1] = (int)lo.y; r[2] = (int)lo.z; r[3] = (int)lo.w;
    }
    return live ? r : v8i{0, 0, 0, 0, 0, 0, 0, 0};
}
// the lane's NaN flag takes the scale code 0xFF and the FP8 NaN codes it has loaded
template <int F>
__device__ __forceinline__ void flag_nan(const v8i (&frag)[kGemmWaveTiles], const int (&scale)[kGemmWaveTiles], uint32_t (&nan)[kGemmWaveTiles]) {
#pragma unroll
    for (int t = 0; t < kGemmWaveTiles; t++) {
        uint32_t bad = scale[t] == 0xff ? 1u : 0u;
        if (F == PPQHIP_MXFP8_E4M3 || F == PPQHIP_MXFP8_E5M2) {
#pragma unroll
            for (int w = 0; w < 8; w++) bad |= fp8_nan_bits<F>((uint32_t)frag[t][w]);
        }
        nan[t] |= bad;
    }
}

// The lane's operand registers of format F for K-step `kb0 / 4` of the row that starts at e.  TAIL: a block at or past nb is not
// read (the load is clamped) and gives zeros.
template <int F, bool TAIL>
__device__ __forceinline__ v8i load_fragment(const uint8_t* e, uint32_t kb0, uint32_t grp, uint32_t nb) {
    constexpr uint32_t bits = gemm_elem_bits(F);
    if (bits == 8u) {
        const uint32_t b0 = kb0 + (grp >> 1), b1 = b0 + 2u, half = 16u * (grp & 1u);
        return fp8_fragment(e + (size_t)(TAIL ? min(b0, nb - 1u) : b0) * 32u + half, e + (size_t)(TAIL ? min(b1, nb - 1u) : b1) * 32u + half,
                            !TAIL || b0 < nb, !TAIL || b1 < nb);
    }
    const uint32_t kb = kb0 + grp;
    return block_fragment<F>(e + (size_t)(TAIL ? min(kb, nb - 1u) : kb) * (4u * bits), !TAIL || kb < nb);
}

// one operand's fragments of a K-step: for each of the wave's kGemmWaveTiles rows (columns) of this lane, the registers above and the
// scale code of block kb0 + grp (127 past nb)
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
    for (int t = 0; t < kGemmWaveTiles; t++)
        if (!live) scale[t] = 127;
    flag_nan<F>(frag, scale, nan);
}

// An operand source of a kernel does two things: prepare(m0, r) once, for the wave's kGemmWaveTiles rows
// m0 + 16 t + r of this lane, and load<TAIL>(kb0, grp, frag, scale, nan) per K-step.  This one is an operand packed along its last
// axis, [rows, nb * B] / [rows, nb]: A of mx_gemm.hip, and B of every kernel.  Rows past the last are clamped.
template <int F>
struct RowSource {
    const uint8_t* elements; const uint8_t* scales;
    uint32_t rows, nb;
    const uint8_t* e[kGemmWaveTiles]; const uint8_t* s[kGemmWaveTiles];           // the lane's rows, set by prepare

    __device__ __forceinline__ void prepare(uint32_t m0, uint32_t r) {
#pragma unroll
        for (int t = 0; t < kGemmWaveTiles; t++) {
            const size_t row = min(m0 + t * kGemmTile + r, rows - 1u);
            e[t] = elements + row * nb * (4u * gemm_elem_bits(F)); s[t] = scales + row * nb;
        }
    }
    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, uint32_t grp, v8i (&frag)[kGemmWaveTiles], int (&scale)[kGemmWaveTiles],
                                         uint32_t (&nan)[kGemmWaveTiles]) const {
        load_operand<F, TAIL>(e, s, kb0, grp, nb, frag, scale, nan);
    }
};

// the flags of the 16 rows (columns) of a tile from the lanes' own: a row is owned by the four lanes r, r + 16, r + 32, r + 48
__device__ __forceinline__ uint32_t tile_flags(uint32_t lane_flag) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(lane_flag != 0u);
    return (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffull);
}

// ---- the fused epilogue ----------------------------------------------------------------------------------
// What a fused launch takes beyond the plain one: v = acc (+ bias) (+ residual), the NaN flags, the ReLU, then v as float32 (the
// plain launch's output pointer, which may be null here) and / or v packed along the columns as ppqhip_mx_pack packs a row.
struct MxFusedOut {
    const float* residual;                        // [m, n] or null
    uint8_t* elements; uint8_t* scales;           // [m, nbo * B], [m, nbo]; both null: no packed output
    uint32_t relu, format;
    uint32_t nbo;                                 // ceil(n / 32)
    MxFmt fmt;
};

constexpr uint32_t kFusedStageBytes = 32u * kMxBlock;                            // a wave's 32 rows of 32 one-byte codes
static_assert(kGemmTile * kGemmWaveTiles == (int)kMxBlock, "a wave's columns are exactly one MX block");

// four one-byte codes of a dword as 4 x BITS bits
template <uint32_t BITS>
__device__ __forceinline__ uint32_t squeeze_codes(uint32_t w) {
    return (w & 0xffu) | (((w >> 8) & 0xffu) << BITS) | (((w >> 16) & 0xffu) << (2u * BITS)) | ((w >> 24) << (3u * BITS));
}

// The epilogue of a wave that owns rows m0 .. m0 + 31 and columns n0 .. n0 + 31 (n0 % 32 == 0: block n0 / 32 of each of its rows) of
// the [m, n] result; acc[i][j][q] is row m0 + 16 i + 4 grp + q, column n0 + 16 j + r.  Rows at or past m and columns at or past n
// hold copies of the last one (the loads are clamped): they take no part in a block maximum, give code 0 and are not stored.
// `stage` is this wave's own kFusedStageBytes of LDS: the codes of a row sit in 16 lanes x 2 tiles and are gathered through it, one
// byte per code; then lane l packs half l & 1 of row l >> 1.  Only the wave itself touches its stage, so the wave is synchronised
// and no workgroup barrier is needed: the waves that returned early are not waited for.
__device__ __forceinline__ void fused_epilogue(const v4f (&acc)[kGemmWaveTiles][kGemmWaveTiles], const uint32_t (&rows_nan)[kGemmWaveTiles],
                                               const uint32_t (&cols_nan)[kGemmWaveTiles], const float* bias, float* c, uint32_t m, uint32_t n,
                                               uint32_t m0, uint32_t n0, uint32_t lane, const MxFusedOut& f, uint8_t* stage) {
    constexpr int T = kGemmWaveTiles;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const bool pack = f.elements != nullptr;
    const MxCoder coder = make_coder(f.format, f.fmt);
    uint32_t col[T]; bool col_in[T], col_nan[T]; float b[T];
#pragma unroll
    for (int j = 0; j < T; j++) {
        col[j] = n0 + j * kGemmTile + r;
        col_in[j] = col[j] < n;
        col[j] = min(col[j], n - 1u);
        b[j] = bias != nullptr ? bias[col[j]] : 0.f;
        col_nan[j] = (cols_nan[j] >> r) & 1u;
    }
    float res[T][4][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < T; j++) {
                const uint32_t row = min(m0 + i * kGemmTile + grp * 4u + q, m - 1u);
                res[i][q][j] = f.residual != nullptr ? f.residual[(size_t)row * n + col[j]] : 0.f;
            }
#pragma unroll
    for (int i = 0; i < T; i++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t tr = grp * 4u + q, row = m0 + i * kGemmTile + tr;
            const bool row_nan = (rows_nan[i] >> tr) & 1u;
            float v[T]; bool live[T];
            uint32_t mag = 0u;
#pragma unroll
            for (int j = 0; j < T; j++) {
                float t = bias != nullptr ? acc[i][j][q] + b[j] : acc[i][j][q];
                if (f.residual != nullptr) t = t + res[i][q][j];
                if (row_nan || col_nan[j]) t = __uint_as_float(0x7fc00000u);
                if (f.relu) t = t > 0.f ? t : (t != t ? t : 0.f);                 // -0 -> +0 (the sign of a zero is a code bit); NaN stays
                v[j] = t;
                live[j] = row < m && col_in[j];
                if (live[j] && c != nullptr) c[(size_t)row * n + col[j]] = t;
                mag = max(mag, live[j] ? mxp_mag(t, coder) : 0u);
            }
            if (!pack) continue;                                                 // wave-uniform
            // the block maximum: the 16 lanes that share grp hold the row's 32 columns
            mag = max(mag, (uint32_t)__shfl_xor((int)mag, 8, 64));
            mag = max(mag, (uint32_t)__shfl_xor((int)mag, 4, 64));
            mag = max(mag, (uint32_t)__shfl_xor((int)mag, 2, 64));
            mag = max(mag, (uint32_t)__shfl_xor((int)mag, 1, 64));
            float inv; bool dead;
            const uint32_t scale = mxp_scale(mag, f.fmt, inv, dead);
#pragma unroll
            for (int j = 0; j < T; j++)
                stage[(i * kGemmTile + tr) * kMxBlock + j * kGemmTile + r] = (uint8_t)(live[j] && !dead ? mxp_code(v[j], inv, f.fmt, coder) : 0u);
            if (r == 0u && row < m) f.scales[(size_t)row * f.nbo + n0 / kMxBlock] = (uint8_t)scale;
        }
    }
    if (!pack) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                        // the wave's own writes, read by its own lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t lr = lane >> 1, half = lane & 1u, row = m0 + lr;
    const uint4 w = *reinterpret_cast<const uint4*>(stage + lr * kMxBlock + half * 16u);
    if (row >= m) return;
    const size_t block = (size_t)row * f.nbo + n0 / kMxBlock;
    if (coder.bits == 8u) {
        *reinterpret_cast<uint4*>(f.elements + block * 32u + half * 16u) = w;
    } else if (coder.bits == 4u) {
        const uint32_t d0 = squeeze_codes<4>(w.x) | (squeeze_codes<4>(w.y) << 16), d1 = squeeze_codes<4>(w.z) | (squeeze_codes<4>(w.w) << 16);
        *reinterpret_cast<uint2*>(f.elements + block * 16u + half * 8u) = make_uint2(d0, d1);
    } else {                                                                     // 4 x 24 bits = 12 bytes at 12 * half: dword stores
        const uint32_t t0 = squeeze_codes<6>(w.x), t1 = squeeze_codes<6>(w.y), t2 = squeeze_codes<6>(w.z), t3 = squeeze_codes<6>(w.w);
        uint32_t* out = reinterpret_cast<uint32_t*>(f.elements + block * 24u + half * 12u);
        out[0] = t0 | (t1 << 24); out[1] = (t1 >> 8) | (t2 << 16); out[2] = (t2 >> 16) | (t3 << 8);
    }
}

// ---- what the kernels' bodies share ----------------------------------------------------------------------
// What every kernel on this instruction computes C[m, n] = A . B^T (+ bias) with: B packed along its last axis, the output, the
// sizes and the workgroup grid.  A kernel's own argument struct holds this beside whatever its A source reads.
struct MxTileArgs {
    const uint8_t* be; const uint8_t* bs;         // B: elements [n, nb * BB], scales [n, nb]
    const float* bias;                            // [n] or null
    float* c;                                     // [m, n]; may be null in a fused launch
    uint32_t m, n, nb;                            // nb: MX blocks of one row of A and of B
    FastDiv tiles_n;                              // workgroups along n
};

// one K-step: both operands' fragments, then the wave's kGemmWaveTiles^2 instructions
template <int FA, int FB, bool TAIL, typename A>
__device__ __forceinline__ void mx_tile_step(const A& a_src, const RowSource<FB>& b_src, uint32_t kb0, uint32_t grp,
                                             v4f (&acc)[kGemmWaveTiles][kGemmWaveTiles], uint32_t (&nan_a)[kGemmWaveTiles],
                                             uint32_t (&nan_b)[kGemmWaveTiles]) {
    constexpr int HA = gemm_hw_format(FA), HB = gemm_hw_format(FB);               // immediates of the instruction
    v8i a[kGemmWaveTiles], b[kGemmWaveTiles];
    int sa[kGemmWaveTiles], sb[kGemmWaveTiles];
    a_src.template load<TAIL>(kb0, grp, a, sa, nan_a);
    b_src.template load<TAIL>(kb0, grp, b, sb, nan_b);
#pragma unroll
    for (int i = 0; i < kGemmWaveTiles; i++)
#pragma unroll
        for (int j = 0; j < kGemmWaveTiles; j++)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], HA, HB, 0, sa[i], 0, sb[j]);
}

// ---- the host frame of the entry points --------------------------------------------------------------------------------------------
// what a fused call adds to a plain one, as the entry point received it
struct MxFusedHost {
    const float* residual; int relu;
    uint8_t* out_elements; uint8_t* out_scales; int out_format;
};

// the host side of MxFusedOut: what both fused entry points check about the outputs before anything else of theirs; fills *fmt
inline int check_fused_outputs(const char* what, const char* float_name, const float* c, const uint8_t* out_elements, const uint8_t* out_scales,
                               int out_format, MxFmt* fmt) {
    if (out_format == PPQHIP_MXINT8) { set_error("%s: out_format: MXINT8 is not a format the fused epilogue packs", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (out_format < PPQHIP_MXFP8_E4M3 || out_format > PPQHIP_MXFP4_E2M1 || !make_mx_fmt(out_format, fmt)) {
        set_error("%s: out_format: unknown MX format %d", what, out_format); return PPQHIP_ERR_INVALID_VALUE;
    }
    if ((out_elements == nullptr) != (out_scales == nullptr)) { set_error("%s: out_elements and out_scales must both be set or both be null", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (c == nullptr && out_elements == nullptr) { set_error("%s: no output: %s and out_elements are both null", what, float_name); return PPQHIP_ERR_INVALID_VALUE; }
    if (out_elements != nullptr && !aligned16(out_elements)) { set_error("%s: out_elements must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

inline int check_format(const char* what, const char* operand, int format) {
    if (format == PPQHIP_MXINT8) { set_error("%s: %s: MXINT8 is not an operand type of the scaled MFMA", what, operand); return PPQHIP_ERR_INVALID_VALUE; }
    if (format < PPQHIP_MXFP8_E4M3 || format > PPQHIP_MXFP4_E2M1) { set_error("%s: %s: unknown MX format %d", what, operand, format); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

// what the fused epilogue of an [m, n] result moves beyond the plain launch: the residual and the packed result join the spans
// and the booked bytes, and f is filled (f.fmt is check_fused_outputs')
inline int book_fused(const char* what, const MxFusedHost& fused, int64_t m, int64_t n, std::vector<Span>& ins, std::vector<Span>& outs,
                      double& bytes, MxFusedOut& f) {
    const int64_t nbo = (n + kMxBlock - 1) / kMxBlock, BO = 4 * (int64_t)gemm_elem_bits(fused.out_format);
    if (m * nbo > kMxMax) { set_error("%s: more than 2^31 - 1 output blocks", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (fused.residual != nullptr) { ins.push_back(span_of(fused.residual, m * n)); bytes += 4.0 * (double)m * (double)n; }
    if (fused.out_elements != nullptr) {
        outs.push_back(span_of(fused.out_elements, m * nbo * BO)); outs.push_back(span_of(fused.out_scales, m * nbo));
        bytes += (double)m * (double)nbo * (double)(BO + 1);
    }
    f.residual = fused.residual; f.elements = fused.out_elements; f.scales = fused.out_scales;
    f.relu = fused.relu ? 1u : 0u; f.format = (uint32_t)fused.out_format; f.nbo = (uint32_t)nbo;
    return PPQHIP_OK;
}

// fn(std::integral_constant<int, F>) for the operand format `format`, which check_format has let through
template <typename Fn>
inline void with_mx_format(int format, Fn&& fn) {
    switch (format) {
        case PPQHIP_MXFP8_E4M3: fn(std::integral_constant<int, PPQHIP_MXFP8_E4M3>{}); break;
        case PPQHIP_MXFP8_E5M2: fn(std::integral_constant<int, PPQHIP_MXFP8_E5M2>{}); break;
        case PPQHIP_MXFP6_E3M2: fn(std::integral_constant<int, PPQHIP_MXFP6_E3M2>{}); break;
        case PPQHIP_MXFP6_E2M3: fn(std::integral_constant<int, PPQHIP_MXFP6_E2M3>{}); break;
        default: fn(std::integral_constant<int, PPQHIP_MXFP4_E2M1>{}); break;
    }
}

// The launch of an entry point, from its grid check on: `ins`, `outs` and `bytes` are the plain launch's, `fused` is null for
// it, and t holds everything but tiles_n.  launch(FA, FB, blocks, stream, f...) starts the kernel of formats FA::value, FB::value on
// `blocks` workgroups: the plain one without f, the fused one with the MxFusedOut.
template <typename Launch>
inline int launch_mx_tiles(const char* what, KernelId plain_id, KernelId fused_id, int a_format, int b_format, const MxFusedHost* fused,
                           MxFusedOut& f, MxTileArgs& t, std::vector<Span>& ins, std::vector<Span>& outs, double bytes, void* stream,
                           Launch&& launch) {
    const int64_t tiles_m = ((int64_t)t.m + kGemmEdge - 1) / kGemmEdge, tiles_n = ((int64_t)t.n + kGemmEdge - 1) / kGemmEdge;
    if (tiles_m * tiles_n > kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (fused != nullptr) {
        if (int st = book_fused(what, *fused, t.m, t.n, ins, outs, bytes, f)) return st;
    }
    if (int st = check_overlap(what, ins, outs)) return st;
    t.tiles_n = make_fastdiv((uint32_t)tiles_n);
    const uint32_t blocks = (uint32_t)(tiles_m * tiles_n);
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(fused != nullptr ? fused_id : plain_id, bytes, s);
    with_mx_format(a_format, [&](auto fa) {
        with_mx_format(b_format, [&](auto fb) {
            if (fused != nullptr) launch(fa, fb, blocks, s, f);
            else launch(fa, fb, blocks, s);
        });
    });
    return finish_launch(what);
}

}  // namespace ppqhip
