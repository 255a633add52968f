// mx_int8_gemm.hip -- C[M, N] (float32) = A[M, K] . B[N, K]^T (+ bias[N]) on two MXINT8 operands, through the int8 MFMA of gfx950
// (v_mfma_i32_16x16x32_i8).  The contract is DESIGN.md section 9.19 and tests/mx_int8_gemm_reference.py.
//
// Both operands are read exactly as mx_pack.hip leaves an MXINT8 tensor packed along its last axis: elements
// [rows, nb * 32] uint8 -- two's-complement k, value k / 64 --, scales [rows, nb] E8M0, nb = ceil(K / 32); B as [N, K] is a Gemm weight
// [out, in].  One instruction has K = 32: exactly one MX block.  Per output and block the integer dot product P_b is exact in int32;
// t_b = P_b 2^(sa + sb - 266) is rounded once to float32 (v_cvt_f32_i32 is exact for |P_b| <= 2^19, v_ldexp_f32 rounds to nearest
// even, keeps subnormals and overflows to Inf) and added to the accumulator, a float32 chain in block order that starts at +0; the
// bias is one more float32 add.  One accumulation order, no atomics, no split-K: two launches give identical bits.
//
// Fragments, as found on the device (tests/test_gpu_mx_int8_gemm.py, the routing test): lane l holds row (A) resp. column (B)
// l & 15 and the 8 bytes k = 8 (l >> 4) .. + 7 of the block in k order; C / D: lane l holds column l & 15, rows 4 (l >> 4) + reg.
//
// Shape: a workgroup of 256 threads owns a 64 x 64 tile of C, each of its 2 x 2 waves a 2 x 2 group of 16 x 16 tiles.  Unlike
// mx_gemm.hip the operands go through LDS: per K-chunk of 4 blocks the workgroup stages 64 rows of A and 64 rows of B, 128 bytes
// each, with 16-byte global loads (two per thread and operand), and their 4 scale codes per row (two bytes per thread).  A staged row
// has a pitch of 144 bytes: 36 dwords, so that the 8-byte fragment reads of the 16 rows of a K-group start 36 dwords apart -- in 16
// different groups of 4 banks -- where a pitch of 128 bytes would put all 16 on one bank; 144 keeps the 16-byte stores aligned.
// Double buffered: the next chunk's global loads are issued into registers before the current chunk's MFMAs and stored to the
// other buffer after them; one barrier per chunk.  In the tail chunk a block at or past nb is not read (its address is clamped to
// the last block) and is not multiplied.  Rows past M or N are clamped on load and not stored.
// Scales: in the C layout a lane needs sb of its own column but sa of the four rows 4 (l >> 4) + q, which are not the row it holds
// as A; both come from the LDS scale stage -- [row][4 codes], so the four rows' codes of a chunk are one 16-byte read.
// NaN: a scale code 0xFF seen while the scales are staged flags the row (column); flagged outputs are written as 0x7fc00000.
// What the kernel shares with mx_int8_conv_kernel (mx_int8_conv.hip) is in mx_int8_tile.hpp: the stage's geometry, the multiply of a
// staged chunk, the NaN flags and the store of the tile; what is here is where a thread's share of a chunk lies in two packed operands.
// ppqhip_mx_int8_gemm_fused runs the same K loop with the fused epilogue (fused_tiles in mx_int8_tile.hpp):
// residual, ReLU and the result packed as MXINT8 along the output columns, in a second instantiation; the plain kernel keeps its code.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_mfma.hpp"
#include "mx_int8_tile.hpp"

namespace ppqhip {
namespace {

struct MxInt8Args {
    const uint8_t* ae; const uint8_t* as;         // A: elements [m, nb * 32], scales [m, nb]
    const uint8_t* be; const uint8_t* bs;         // B: elements [n, nb * 32], scales [n, nb]
    const float* bias;                            // [n] or null
    float* c;                                     // [m, n]; may be null in a fused launch
    uint32_t m, n, nb;
    FastDiv tiles_n;
};

// Where a thread's share of a chunk lies: element segment t & 7 (16 bytes; block (t & 7) >> 1 of the chunk) of rows t >> 3 and
// 32 + (t >> 3) of both operands, and the scale codes 2 pair, 2 pair + 1 of row (t & 127) >> 1 of operand t >> 7.
struct StageMap {
    const uint8_t* ga[2]; const uint8_t* gb[2];   // the rows' elements in global memory (rows clamped)
    const uint8_t* gs;                            // the row's scale codes
    uint32_t seg, lds_e[2], lds_s, pair, nb;

    __device__ __forceinline__ void prepare(const MxInt8Args& g, uint32_t row0, uint32_t col0, uint32_t t) {
        nb = g.nb; seg = t & 7u; pair = t & 1u;
        const size_t pitch = (size_t)g.nb * kMxBlock;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = (t >> 3) + 32u * h;
            ga[h] = g.ae + min(row0 + row, g.m - 1u) * pitch;
            gb[h] = g.be + min(col0 + row, g.n - 1u) * pitch;
            lds_e[h] = row * kI8Pitch + seg * 16u;
        }
        const uint32_t srow = (t & 127u) >> 1;
        gs = t < 128u ? g.as + (size_t)min(row0 + srow, g.m - 1u) * g.nb : g.bs + (size_t)min(col0 + srow, g.n - 1u) * g.nb;
        lds_s = 2u * kI8TileBytes + (t >> 7) * kI8ScaleBytes + srow * kGemmStepBlocks + 2u * pair;
    }

    // the loads of the chunk that starts at block kb0; returns whether a live scale code is 0xFF
    template <bool TAIL>
    __device__ __forceinline__ bool load(uint32_t kb0, Staged& st) const {
        const uint32_t eb = kb0 + (seg >> 1);
        const size_t off = (size_t)(TAIL ? min(eb, nb - 1u) : eb) * kMxBlock + 16u * (seg & 1u);
        st.a0 = *reinterpret_cast<const v4u*>(ga[0] + off); st.a1 = *reinterpret_cast<const v4u*>(ga[1] + off);
        st.b0 = *reinterpret_cast<const v4u*>(gb[0] + off); st.b1 = *reinterpret_cast<const v4u*>(gb[1] + off);
        const uint32_t s0 = kb0 + 2u * pair, s1 = s0 + 1u;
        const uint32_t c0 = gs[TAIL ? min(s0, nb - 1u) : s0], c1 = gs[TAIL ? min(s1, nb - 1u) : s1];
        st.s = c0 | (c1 << 8);
        return (c0 == 0xffu && (!TAIL || s0 < nb)) || (c1 == 0xffu && (!TAIL || s1 < nb));
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Staged& st) const { store_staged(buf, lds_e, lds_s, st); }
};

// F is empty -- the plain kernel, (g) alone -- or one MxFusedOut: fused_tiles in place of store_tiles, (g, f).  Everything up to the
// final barrier is the same code.
template <typename... F>
__global__ __launch_bounds__(kBlock) void mx_int8_gemm_kernel(const MxInt8Args g, const F... f) {
    constexpr bool FUSED = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one MxFusedOut");
    constexpr int T = kGemmWaveTiles;
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kI8BufBytes];
    __shared__ uint32_t nan_flags[2 * kGemmEdge];                                // rows of A, then rows of B (columns of C)
    const uint32_t tm = fdiv(blockIdx.x, g.tiles_n), tn = blockIdx.x - tm * g.tiles_n.d;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t row0 = tm * kGemmEdge, col0 = tn * kGemmEdge;
    const uint32_t wm = (wave / kGemmWaves) * (T * kGemmTile), wn = (wave % kGemmWaves) * (T * kGemmTile);
    const bool busy = row0 + wm < g.m && col0 + wn < g.n;                        // wave-uniform: a wave past the edge only stages

    v4f acc[T][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    clear_nan_flags(nan_flags, t);

    bool bad = false;
    if (g.nb > 0u) {                                                             // nb == 0: the operands may be null
        StageMap map;
        map.prepare(g, row0, col0, t);
        const uint32_t chunks = (g.nb + kGemmStepBlocks - 1u) / kGemmStepBlocks, rest = g.nb % kGemmStepBlocks;
        Staged st;
        bad |= chunks == 1u && rest ? map.load<true>(0u, st) : map.load<false>(0u, st);
        map.store(stage[0], st);
        __syncthreads();
        for (uint32_t c = 0; c < chunks; c++) {
            const bool more = c + 1u < chunks, last_short = c + 2u == chunks && rest != 0u;
            if (more) bad |= last_short ? map.load<true>((c + 1u) * kGemmStepBlocks, st) : map.load<false>((c + 1u) * kGemmStepBlocks, st);
            if (busy) {
                if (!more && rest) chunk_tiles<true>(stage[c & 1u], wm, wn, r, grp, rest, acc);
                else chunk_tiles<false>(stage[c & 1u], wm, wn, r, grp, kGemmStepBlocks, acc);
            }
            if (more) map.store(stage[(c + 1u) & 1u], st);                       // last read before the barrier that ended chunk c - 1
            __syncthreads();
        }
        raise_nan_flag(nan_flags, t, bad);
    }
    __syncthreads();
    if (!busy) return;

    if constexpr (FUSED) {                                                       // the operand stage is dead: the waves gather their codes in it
        fused_tiles(acc, nan_flags, g.bias, g.c, g.m, g.n, row0, col0, wm, wn, lane, f..., &stage[0][0]);
        return;
    }
    store_tiles(acc, nan_flags, g.bias, g.c, g.m, g.n, row0, col0, wm, wn, r, grp);
}

// both entry points; `fused` is null for ppqhip_mx_int8_gemm, whose checks, strings and launch are unchanged
int run_int8_gemm(const char* what, const uint8_t* a_elements, const uint8_t* a_scales, const uint8_t* b_elements, const uint8_t* b_scales,
                  const float* bias, float* c, int64_t m, int64_t n, int64_t k, const MxFusedHost* fused, void* stream) {
    MxFusedOut f = {};
    if (fused != nullptr) {
        if (int st = check_int8_fused(what, "c", c, *fused, f)) return st;
    }
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kMxMax || n > kMxMax || k > kMxMax) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t nb = (k + kMxBlock - 1) / kMxBlock;
    if ((c == nullptr && fused == nullptr) || (nb > 0 && (a_elements == nullptr || a_scales == nullptr || b_elements == nullptr || b_scales == nullptr))) {
        set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (!aligned16(c) || (nb > 0 && (!aligned16(a_elements) || !aligned16(b_elements)))) {
        set_error("%s: elements and c must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    std::vector<Span> ins, outs;
    if (nb > 0) {
        ins.push_back(span_of(a_elements, m * nb * kMxBlock)); ins.push_back(span_of(a_scales, m * nb));
        ins.push_back(span_of(b_elements, n * nb * kMxBlock)); ins.push_back(span_of(b_scales, n * nb));
    }
    if (bias != nullptr) ins.push_back(span_of(bias, n));
    if (c != nullptr) outs.push_back(span_of(c, m * n));
    // booked: the operands and 4 m n bytes of C; the launch does 2 m n nb 32 integer operations
    double bytes = ((double)m + (double)n) * (double)nb * (double)(kMxBlock + 1);
    if (c != nullptr) bytes += 4.0 * (double)m * (double)n;

    MxInt8Args g;
    g.ae = a_elements; g.as = a_scales; g.be = b_elements; g.bs = b_scales; g.bias = bias; g.c = c;
    g.m = (uint32_t)m; g.n = (uint32_t)n; g.nb = (uint32_t)nb;
    return launch_int8_tiles(what, K_MX_INT8_GEMM, K_MX_INT8_GEMM_FUSED, fused, f, m, n, ins, outs, bytes, stream, g.tiles_n,
                             [&g](uint32_t blocks, hipStream_t s, const auto&... fo) {
        hipLaunchKernelGGL((mx_int8_gemm_kernel<std::decay_t<decltype(fo)>...>), dim3(blocks), dim3(kBlock), 0, s, g, fo...);
    });
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_int8_gemm(const uint8_t* a_elements, const uint8_t* a_scales, const uint8_t* b_elements, const uint8_t* b_scales,
                                   const float* bias, float* c, int64_t m, int64_t n, int64_t k, void* stream) {
    return run_int8_gemm("mx_int8_gemm", a_elements, a_scales, b_elements, b_scales, bias, c, m, n, k, nullptr, stream);
}

extern "C" int ppqhip_mx_int8_gemm_fused(const uint8_t* a_elements, const uint8_t* a_scales, const uint8_t* b_elements,
                                         const uint8_t* b_scales, const float* bias, const float* residual, int relu, float* c,
                                         uint8_t* out_elements, uint8_t* out_scales, int64_t m, int64_t n, int64_t k, void* stream) {
    const MxFusedHost fused = {residual, relu, out_elements, out_scales, PPQHIP_MXINT8};
    return run_int8_gemm("mx_int8_gemm_fused", a_elements, a_scales, b_elements, b_scales, bias, c, m, n, k, &fused, stream);
}
