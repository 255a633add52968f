// mx_gemm.hip -- C[M, N] (float32) = A[M, K] . B[N, K]^T (+ bias[N]) on packed OCP Microscaling operands, through the block-scaled
// MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4).  The contract is DESIGN.md section 9.14 and tests/mx_gemm_reference.py.
//
// Both operands are read exactly as mx_pack.hip leaves a tensor packed along its last axis: elements
// [rows, nb * B] uint8, scales [rows, nb] uint8, nb = ceil(K / 32), B = 32 / 24 / 16 bytes per block of 32 elements; B as [N, K] is a
// Gemm weight [out, in].  The five float formats in any combination (25 kernels: cbsz / blgp are immediates); MXINT8 is not an
// operand type of the instruction.
//
// One instruction multiplies a 16 x 128 tile of A by a 128 x 16 tile of B: four MX blocks per row (column).  As found on the device
// (tools/mx_mfma_probe.hip), lane l owns row (A) resp. column (B) l & 15 and K-group g = l >> 4, and
//   * byte 0 (opsel 0) of the lane's scale register is the E8M0 code of block g of the K-step, k = 32 g .. 32 g + 31, in every format;
//   * an FP6 / FP4 lane holds the elements of that same block: its 24 / 16 bytes in dwords 0 .. 5 / 0 .. 3, in the dense
//     little-endian order of the export -- no permutation;
//   * an FP8 lane does NOT hold its scale's block: dwords 0 .. 3 are k = 16 g .. 16 g + 15 and dwords 4 .. 7 k = 64 + 16 g .. 64 + 16 g + 15
//     (byte order = k order), i.e. half of block g >> 1 and half of block 2 + (g >> 1); the scales still come from lanes g >> 1 and
//     2 + (g >> 1).  The lane reads two 16-byte halves of the 128 contiguous bytes of its row's K-step.
// C / D: lane l holds column l & 15, rows 4 (l >> 4) + reg.
//
// Shape: a workgroup of 256 threads owns a 64 x 64 tile of C, each of its 2 x 2 waves a 2 x 2 group of 16 x 16 tiles; the fragments
// come straight from global memory (16-byte loads, 8-byte ones for the 24-byte blocks of FP6), rows past M or N are clamped on
// load and not stored.  One accumulation order, no atomics, no split-K: two launches give identical bits.
// A K-step that reaches past nb feeds zero element bits and scale code 127 for the missing blocks; inside a short last block the
// export already holds +0.
// NaN: the result is NaN wherever dequantise-then-multiply is, whatever the instruction itself makes of the codes: a scale code
// 0xFF or an FP8 NaN code seen while a row's (column's) blocks are loaded flags the row (column), and flagged outputs are written
// as the quiet NaN 0x7fc00000.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_common.hpp"

namespace ppqhip {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kGemmTile = 16;                     // one MFMA's rows and columns
constexpr int kGemmWaveTiles = 2;                 // a wave owns kGemmWaveTiles^2 MFMA tiles ...
constexpr int kGemmWaves = 2;                     // ... and a workgroup kGemmWaves^2 waves
constexpr int kGemmEdge = kGemmTile * kGemmWaveTiles * kGemmWaves;       // 64: rows and columns of C per workgroup
constexpr uint32_t kGemmStepBlocks = 4;           // MX blocks of one row per instruction (K = 128)
static_assert(kGemmWaves * kGemmWaves * kWave == kBlock, "four waves per workgroup");

struct MxGemmArgs {
    const uint8_t* ae; const uint8_t* as;         // A: elements [m, nb * BA], scales [m, nb]
    const uint8_t* be; const uint8_t* bs;         // B: elements [n, nb * BB], scales [n, nb]
    const float* bias;                            // [n] or null
    float* c;                                     // [m, n]
    uint32_t m, n, nb;
    FastDiv tiles_n;                              // workgroups along N
};

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

template <int FA, int FB>
__global__ __launch_bounds__(kBlock) void mx_gemm_kernel(const MxGemmArgs g) {
    constexpr int T = kGemmWaveTiles;
    constexpr uint32_t BA = 4u * gemm_elem_bits(FA), BB = 4u * gemm_elem_bits(FB);
    constexpr int HA = gemm_hw_format(FA), HB = gemm_hw_format(FB);               // immediates of the instruction
    const uint32_t tm = fdiv(blockIdx.x, g.tiles_n), tn = blockIdx.x - tm * g.tiles_n.d;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t m0 = tm * kGemmEdge + (wave / kGemmWaves) * (T * kGemmTile);
    const uint32_t n0 = tn * kGemmEdge + (wave % kGemmWaves) * (T * kGemmTile);
    if (m0 >= g.m || n0 >= g.n) return;                                          // wave-uniform; there is no barrier below

    const uint8_t* ae[T]; const uint8_t* as[T]; const uint8_t* be[T]; const uint8_t* bs[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        const size_t row = min(m0 + t * kGemmTile + r, g.m - 1u), col = min(n0 + t * kGemmTile + r, g.n - 1u);
        ae[t] = g.ae + row * g.nb * BA; as[t] = g.as + row * g.nb;
        be[t] = g.be + col * g.nb * BB; bs[t] = g.bs + col * g.nb;
    }
    v4f acc[T][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    uint32_t nan_a[T], nan_b[T];
#pragma unroll
    for (int t = 0; t < T; t++) { nan_a[t] = 0u; nan_b[t] = 0u; }

    v8i a[T], b[T];
    int sa[T], sb[T];
    const uint32_t full = g.nb / kGemmStepBlocks;
    for (uint32_t s = 0; s < full; s++) {
        load_operand<FA, false>(ae, as, s * kGemmStepBlocks, grp, g.nb, a, sa, nan_a);
        load_operand<FB, false>(be, bs, s * kGemmStepBlocks, grp, g.nb, b, sb, nan_b);
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], HA, HB, 0, sa[i], 0, sb[j]);
    }
    if (g.nb % kGemmStepBlocks) {
        load_operand<FA, true>(ae, as, full * kGemmStepBlocks, grp, g.nb, a, sa, nan_a);
        load_operand<FB, true>(be, bs, full * kGemmStepBlocks, grp, g.nb, b, sb, nan_b);
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], HA, HB, 0, sa[i], 0, sb[j]);
    }

    uint32_t rows_nan[T], cols_nan[T];
#pragma unroll
    for (int t = 0; t < T; t++) { rows_nan[t] = tile_flags(nan_a[t]); cols_nan[t] = tile_flags(nan_b[t]); }
#pragma unroll
    for (int j = 0; j < T; j++) {
        const uint32_t col = n0 + j * kGemmTile + r;
        if (col >= g.n) continue;
        const float bias = g.bias != nullptr ? g.bias[col] : 0.f;
        const bool col_nan = (cols_nan[j] >> r) & 1u;
#pragma unroll
        for (int i = 0; i < T; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t tr = grp * 4u + q, row = m0 + i * kGemmTile + tr;
                const bool bad = col_nan || ((rows_nan[i] >> tr) & 1u);
                const float v = g.bias != nullptr ? acc[i][j][q] + bias : acc[i][j][q];
                if (row < g.m) g.c[(size_t)row * g.n + col] = bad ? __uint_as_float(0x7fc00000u) : v;
            }
        }
    }
}

template <int FA, int FB>
void launch(const MxGemmArgs& g, uint32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((mx_gemm_kernel<FA, FB>), dim3(blocks), dim3(kBlock), 0, s, g);
}
template <int FA>
void launch_b(int fb, const MxGemmArgs& g, uint32_t blocks, hipStream_t s) {
    switch (fb) {
        case PPQHIP_MXFP8_E4M3: launch<FA, PPQHIP_MXFP8_E4M3>(g, blocks, s); break;
        case PPQHIP_MXFP8_E5M2: launch<FA, PPQHIP_MXFP8_E5M2>(g, blocks, s); break;
        case PPQHIP_MXFP6_E3M2: launch<FA, PPQHIP_MXFP6_E3M2>(g, blocks, s); break;
        case PPQHIP_MXFP6_E2M3: launch<FA, PPQHIP_MXFP6_E2M3>(g, blocks, s); break;
        default: launch<FA, PPQHIP_MXFP4_E2M1>(g, blocks, s); break;
    }
}

int check_format(const char* what, const char* operand, int format) {
    if (format == PPQHIP_MXINT8) { set_error("%s: %s: MXINT8 is not an operand type of the scaled MFMA", what, operand); return PPQHIP_ERR_INVALID_VALUE; }
    if (format < PPQHIP_MXFP8_E4M3 || format > PPQHIP_MXFP4_E2M1) { set_error("%s: %s: unknown MX format %d", what, operand, format); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_gemm(const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
                              const uint8_t* b_scales, int b_format, const float* bias, float* c, int64_t m, int64_t n, int64_t k,
                              void* stream) {
    const char* what = "mx_gemm";
    if (int st = check_format(what, "A", a_format)) return st;
    if (int st = check_format(what, "B", b_format)) return st;
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kMxMax || n > kMxMax || k > kMxMax) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t nb = (k + kMxBlock - 1) / kMxBlock;
    const int64_t BA = 4 * (int64_t)gemm_elem_bits(a_format), BB = 4 * (int64_t)gemm_elem_bits(b_format);
    if (c == nullptr || (nb > 0 && (a_elements == nullptr || a_scales == nullptr || b_elements == nullptr || b_scales == nullptr))) {
        set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (!aligned16(c) || (nb > 0 && (!aligned16(a_elements) || !aligned16(b_elements)))) {
        set_error("%s: elements and c must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    const int64_t tiles_m = (m + kGemmEdge - 1) / kGemmEdge, tiles_n = (n + kGemmEdge - 1) / kGemmEdge;
    if (tiles_m * tiles_n > kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    std::vector<Span> ins, outs;
    if (nb > 0) {
        ins.push_back(span_of(a_elements, m * nb * BA)); ins.push_back(span_of(a_scales, m * nb));
        ins.push_back(span_of(b_elements, n * nb * BB)); ins.push_back(span_of(b_scales, n * nb));
    }
    if (bias != nullptr) ins.push_back(span_of(bias, n));
    outs.push_back(span_of(c, m * n));
    if (int st = check_overlap(what, ins, outs)) return st;

    MxGemmArgs g;
    g.ae = a_elements; g.as = a_scales; g.be = b_elements; g.bs = b_scales; g.bias = bias; g.c = c;
    g.m = (uint32_t)m; g.n = (uint32_t)n; g.nb = (uint32_t)nb;
    g.tiles_n = make_fastdiv((uint32_t)tiles_n);
    const uint32_t blocks = (uint32_t)(tiles_m * tiles_n);
    hipStream_t s = (hipStream_t)stream;
    // booked: the operands and 4 m n bytes of C; the launch does 2 m n nb 32 flops
    const double bytes = (double)m * (double)nb * (double)(BA + 1) + (double)n * (double)nb * (double)(BB + 1) + 4.0 * (double)m * (double)n;
    LaunchScope scope(K_MX_GEMM, bytes, s);
    switch (a_format) {
        case PPQHIP_MXFP8_E4M3: launch_b<PPQHIP_MXFP8_E4M3>(b_format, g, blocks, s); break;
        case PPQHIP_MXFP8_E5M2: launch_b<PPQHIP_MXFP8_E5M2>(b_format, g, blocks, s); break;
        case PPQHIP_MXFP6_E3M2: launch_b<PPQHIP_MXFP6_E3M2>(b_format, g, blocks, s); break;
        case PPQHIP_MXFP6_E2M3: launch_b<PPQHIP_MXFP6_E2M3>(b_format, g, blocks, s); break;
        default: launch_b<PPQHIP_MXFP4_E2M1>(b_format, g, blocks, s); break;
    }
    return finish_launch(what);
}
