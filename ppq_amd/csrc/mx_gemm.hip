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
// ppqhip_mx_gemm_fused runs the same K loop with the fused epilogue of mx_mfma.hpp: residual, ReLU and the result
// packed along the output columns, in a second set of 25 instantiations; the plain kernels keep their code.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_mfma.hpp"

namespace ppqhip {
namespace {

struct MxGemmArgs {
    const uint8_t* ae; const uint8_t* as;         // A: elements [m, nb * BA], scales [m, nb]
    const uint8_t* be; const uint8_t* bs;         // B: elements [n, nb * BB], scales [n, nb]
    const float* bias;                            // [n] or null
    float* c;                                     // [m, n]
    uint32_t m, n, nb;
    FastDiv tiles_n;                              // workgroups along N
};

// F is empty -- the plain kernel, (g) alone -- or one MxFusedOut: the epilogue of mx_mfma.hpp (fused_epilogue) in place of the plain
// one, (g, f).  Everything up to the epilogue is the same code; in the fused kernel g.c may be null.
template <int FA, int FB, typename... F>
__global__ __launch_bounds__(kBlock) void mx_gemm_kernel(const MxGemmArgs g, const F... f) {
    constexpr bool FUSED = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one MxFusedOut");
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
    if constexpr (FUSED) {                                                       // the stage is wave-private: no barrier, the early return stands
        __shared__ __attribute__((aligned(16))) uint8_t stage[kGemmWaves * kGemmWaves * kFusedStageBytes];
        fused_epilogue(acc, rows_nan, cols_nan, g.bias, g.c, g.m, g.n, m0, n0, lane, f..., stage + wave * kFusedStageBytes);
        return;
    }
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
void launch(const MxGemmArgs& g, const MxFusedOut* f, uint32_t blocks, hipStream_t s) {
    if (f != nullptr) hipLaunchKernelGGL((mx_gemm_kernel<FA, FB, MxFusedOut>), dim3(blocks), dim3(kBlock), 0, s, g, *f);
    else hipLaunchKernelGGL((mx_gemm_kernel<FA, FB>), dim3(blocks), dim3(kBlock), 0, s, g);
}
template <int FA>
void launch_b(int fb, const MxGemmArgs& g, const MxFusedOut* f, uint32_t blocks, hipStream_t s) {
    switch (fb) {
        case PPQHIP_MXFP8_E4M3: launch<FA, PPQHIP_MXFP8_E4M3>(g, f, blocks, s); break;
        case PPQHIP_MXFP8_E5M2: launch<FA, PPQHIP_MXFP8_E5M2>(g, f, blocks, s); break;
        case PPQHIP_MXFP6_E3M2: launch<FA, PPQHIP_MXFP6_E3M2>(g, f, blocks, s); break;
        case PPQHIP_MXFP6_E2M3: launch<FA, PPQHIP_MXFP6_E2M3>(g, f, blocks, s); break;
        default: launch<FA, PPQHIP_MXFP4_E2M1>(g, f, blocks, s); break;
    }
}

// what a fused call adds to a plain one, as the entry point received it
struct GemmFusedHost {
    const float* residual; int relu;
    uint8_t* out_elements; uint8_t* out_scales; int out_format;
};

// both entry points; `fused` is null for ppqhip_mx_gemm, whose checks, strings and launch are unchanged
int run_gemm(const char* what, const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
             const uint8_t* b_scales, int b_format, const float* bias, float* c, int64_t m, int64_t n, int64_t k, const GemmFusedHost* fused,
             void* stream) {
    if (int st = check_format(what, "A", a_format)) return st;
    if (int st = check_format(what, "B", b_format)) return st;
    MxFusedOut f = {};
    if (fused != nullptr) {
        if (int st = check_fused_outputs(what, "c", c, fused->out_elements, fused->out_scales, fused->out_format, &f.fmt)) return st;
    }
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kMxMax || n > kMxMax || k > kMxMax) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t nb = (k + kMxBlock - 1) / kMxBlock;
    const int64_t BA = 4 * (int64_t)gemm_elem_bits(a_format), BB = 4 * (int64_t)gemm_elem_bits(b_format);
    if ((c == nullptr && fused == nullptr) || (nb > 0 && (a_elements == nullptr || a_scales == nullptr || b_elements == nullptr || b_scales == nullptr))) {
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
    if (c != nullptr) outs.push_back(span_of(c, m * n));
    // booked: the operands and 4 m n bytes of C; the launch does 2 m n nb 32 flops
    double bytes = (double)m * (double)nb * (double)(BA + 1) + (double)n * (double)nb * (double)(BB + 1);
    if (c != nullptr) bytes += 4.0 * (double)m * (double)n;
    if (fused != nullptr) {                       // and what the fused epilogue moves: the residual and the packed result
        const int64_t nbo = (n + kMxBlock - 1) / kMxBlock, BO = 4 * (int64_t)gemm_elem_bits(fused->out_format);
        if (m * nbo > kMxMax) { set_error("%s: more than 2^31 - 1 output blocks", what); return PPQHIP_ERR_INVALID_VALUE; }
        if (fused->residual != nullptr) { ins.push_back(span_of(fused->residual, m * n)); bytes += 4.0 * (double)m * (double)n; }
        if (fused->out_elements != nullptr) {
            outs.push_back(span_of(fused->out_elements, m * nbo * BO)); outs.push_back(span_of(fused->out_scales, m * nbo));
            bytes += (double)m * (double)nbo * (double)(BO + 1);
        }
        f.residual = fused->residual; f.elements = fused->out_elements; f.scales = fused->out_scales;
        f.relu = fused->relu ? 1u : 0u; f.format = (uint32_t)fused->out_format; f.nbo = (uint32_t)nbo;
    }
    if (int st = check_overlap(what, ins, outs)) return st;

    MxGemmArgs g;
    g.ae = a_elements; g.as = a_scales; g.be = b_elements; g.bs = b_scales; g.bias = bias; g.c = c;
    g.m = (uint32_t)m; g.n = (uint32_t)n; g.nb = (uint32_t)nb;
    g.tiles_n = make_fastdiv((uint32_t)tiles_n);
    const uint32_t blocks = (uint32_t)(tiles_m * tiles_n);
    hipStream_t s = (hipStream_t)stream;
    const MxFusedOut* fp = fused != nullptr ? &f : nullptr;
    LaunchScope scope(fused != nullptr ? K_MX_GEMM_FUSED : K_MX_GEMM, bytes, s);
    switch (a_format) {
        case PPQHIP_MXFP8_E4M3: launch_b<PPQHIP_MXFP8_E4M3>(b_format, g, fp, blocks, s); break;
        case PPQHIP_MXFP8_E5M2: launch_b<PPQHIP_MXFP8_E5M2>(b_format, g, fp, blocks, s); break;
        case PPQHIP_MXFP6_E3M2: launch_b<PPQHIP_MXFP6_E3M2>(b_format, g, fp, blocks, s); break;
        case PPQHIP_MXFP6_E2M3: launch_b<PPQHIP_MXFP6_E2M3>(b_format, g, fp, blocks, s); break;
        default: launch_b<PPQHIP_MXFP4_E2M1>(b_format, g, fp, blocks, s); break;
    }
    return finish_launch(what);
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_gemm(const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
                              const uint8_t* b_scales, int b_format, const float* bias, float* c, int64_t m, int64_t n, int64_t k,
                              void* stream) {
    return run_gemm("mx_gemm", a_elements, a_scales, a_format, b_elements, b_scales, b_format, bias, c, m, n, k, nullptr, stream);
}

extern "C" int ppqhip_mx_gemm_fused(const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
                                    const uint8_t* b_scales, int b_format, const float* bias, const float* residual, int relu, float* c,
                                    uint8_t* out_elements, uint8_t* out_scales, int out_format, int64_t m, int64_t n, int64_t k,
                                    void* stream) {
    const GemmFusedHost fused = {residual, relu, out_elements, out_scales, out_format};
    return run_gemm("mx_gemm_fused", a_elements, a_scales, a_format, b_elements, b_scales, b_format, bias, c, m, n, k, &fused, stream);
}
