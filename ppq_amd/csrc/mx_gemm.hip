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
// What the kernel shares with mx_conv_kernel is in mx_mfma.hpp; A is read as B is: a RowSource.
#include "common.hpp"
#include "mx_mfma.hpp"

namespace ppqhip {
namespace {

struct MxGemmArgs {
    const uint8_t* ae; const uint8_t* as;         // A: elements [m, nb * BA], scales [m, nb]
    MxTileArgs t;
};

// F is empty -- the plain kernel, (g) alone -- or one MxFusedOut: the epilogue of mx_mfma.hpp (fused_epilogue) in place of the plain
// one, (g, f).  Everything up to the epilogue is the same code; in the fused kernel g.t.c may be null.  The text of this kernel
// and of mx_conv_kernel (mx_conv.hip) differs in the A source alone; it stays in the kernel because the backend schedules the FP8 K loops worse
// when it is an inlined function (profiles/mx_tile.txt).
template <int FA, int FB, typename... F>
__global__ __launch_bounds__(kBlock) void mx_gemm_kernel(const MxGemmArgs g, const F... f) {
    constexpr bool FUSED = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one MxFusedOut");
    constexpr int T = kGemmWaveTiles;
    const MxTileArgs& t = g.t;
    const uint32_t tm = fdiv(blockIdx.x, t.tiles_n), tn = blockIdx.x - tm * t.tiles_n.d;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t m0 = tm * kGemmEdge + (wave / kGemmWaves) * (T * kGemmTile);
    const uint32_t n0 = tn * kGemmEdge + (wave % kGemmWaves) * (T * kGemmTile);
    if (m0 >= t.m || n0 >= t.n) return;                                          // wave-uniform; there is no barrier below

    RowSource<FA> a_src{g.ae, g.as, t.m, t.nb};
    RowSource<FB> b_src{t.be, t.bs, t.n, t.nb};
    a_src.prepare(m0, r);
    b_src.prepare(n0, r);
    v4f acc[T][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    uint32_t nan_a[T], nan_b[T];
#pragma unroll
    for (int i = 0; i < T; i++) { nan_a[i] = 0u; nan_b[i] = 0u; }

    const uint32_t full = t.nb / kGemmStepBlocks;
    for (uint32_t s = 0; s < full; s++) mx_tile_step<FA, FB, false>(a_src, b_src, s * kGemmStepBlocks, grp, acc, nan_a, nan_b);
    if (t.nb % kGemmStepBlocks) mx_tile_step<FA, FB, true>(a_src, b_src, full * kGemmStepBlocks, grp, acc, nan_a, nan_b);

    uint32_t rows_nan[T], cols_nan[T];
#pragma unroll
    for (int i = 0; i < T; i++) { rows_nan[i] = tile_flags(nan_a[i]); cols_nan[i] = tile_flags(nan_b[i]); }
    if constexpr (FUSED) {                                                       // the stage is wave-private: no barrier, the early return stands
        __shared__ __attribute__((aligned(16))) uint8_t stage[kGemmWaves * kGemmWaves * kFusedStageBytes];
        fused_epilogue(acc, rows_nan, cols_nan, t.bias, t.c, t.m, t.n, m0, n0, lane, f..., stage + wave * kFusedStageBytes);
        return;
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        const uint32_t col = n0 + j * kGemmTile + r;
        if (col >= t.n) continue;
        const float bias = t.bias != nullptr ? t.bias[col] : 0.f;
        const bool col_nan = (cols_nan[j] >> r) & 1u;
#pragma unroll
        for (int i = 0; i < T; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t tr = grp * 4u + q, row = m0 + i * kGemmTile + tr;
                const bool bad = col_nan || ((rows_nan[i] >> tr) & 1u);
                const float v = t.bias != nullptr ? acc[i][j][q] + bias : acc[i][j][q];
                if (row < t.m) t.c[(size_t)row * t.n + col] = bad ? __uint_as_float(0x7fc00000u) : v;
            }
        }
    }
}

// both entry points; `fused` is null for ppqhip_mx_gemm, whose checks, strings and launch are unchanged
int run_gemm(const char* what, const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
             const uint8_t* b_scales, int b_format, const float* bias, float* c, int64_t m, int64_t n, int64_t k, const MxFusedHost* fused,
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

    MxGemmArgs g;
    g.ae = a_elements; g.as = a_scales;
    g.t.be = b_elements; g.t.bs = b_scales; g.t.bias = bias; g.t.c = c;
    g.t.m = (uint32_t)m; g.t.n = (uint32_t)n; g.t.nb = (uint32_t)nb;
    return launch_mx_tiles(what, K_MX_GEMM, K_MX_GEMM_FUSED, a_format, b_format, fused, f, g.t, ins, outs, bytes, stream,
                           [&g](auto fa, auto fb, uint32_t blocks, hipStream_t s, const auto&... fo) {
        hipLaunchKernelGGL((mx_gemm_kernel<decltype(fa)::value, decltype(fb)::value, std::decay_t<decltype(fo)>...>), dim3(blocks),
                           dim3(kBlock), 0, s, g, fo...);
    });
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
    const MxFusedHost fused = {residual, relu, out_elements, out_scales, out_format};
    return run_gemm("mx_gemm_fused", a_elements, a_scales, a_format, b_elements, b_scales, b_format, bias, c, m, n, k, &fused, stream);
}
