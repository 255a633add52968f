// int8_gemm.hpp -- the GEMM of the linear INT8 family for either B codec of int8_tile.hpp: int8_gemm.hip (Q8B8, int8 weights) and
// int4_gemm.hip (Q8B4, packed int4 weights) are its two instances.  C[M, N] = requant(tail(float32(sum_k B[n, k] (A[m, k] - zx)) *
// mul[n])) on v_mfma_i32_16x16x32_i8 with the int32 accumulator chained through the MFMA's C operand over all of K.  The contract is
// DESIGN.md sections 9.22 / 9.23 and tests/int8_reference.py; the tile, the K loop, the B codecs and the epilogue are in int8_tile.hpp.
// What is here is where a thread's share of a chunk of A lies in a row-major operand, and the body of the entry points.
//
// Operands: A [M, Kp] int8 codes and B [N, Kp] as its codec stores it (Kp or Kp / 2 bytes a row), Kp = ceil32(K), the codes K .. Kp - 1
// of B zero (so those of A do not matter; they are the zero point by convention).  B as [N, K] is a Gemm weight [out, in].  One
// instruction has K = 32: one block of a row.  In the tail chunk a block at or past Kp / 32 is not read (its address is clamped to the
// last block) and is not multiplied.  Rows past M or N are clamped on load and not stored.  One accumulation order, no atomics, no
// split-K: two launches give identical bits -- and integer sums do not depend on the order anyway.
#pragma once
#include "common.hpp"
#include "job_table.hpp"
#include "int8_tile.hpp"

namespace ppqhip {

struct Int8GemmArgs {
    const uint8_t* a; const uint8_t* b;           // [m, nb * 32], [n, nb * kBlockBytes of the codec]
    uint32_t nb;
    Int8Tail e;
};

#if defined(__HIPCC__)

// Where a thread's share of a chunk lies: of A segment t & 7 (16 bytes; block (t & 7) >> 1 of the chunk) of rows t >> 3 and
// 32 + (t >> 3); of B what its codec's map says.
template <typename B>
struct GemmMap {
    const uint8_t* ga[2];                         // the rows in global memory (rows clamped)
    uint32_t seg, lds_e[2], nb;
    typename B::Map bmap;

    __device__ __forceinline__ GemmMap(const Int8GemmArgs& g, uint32_t row0, uint32_t col0, uint32_t t) : bmap(g.b, g.nb, g.e.n, col0, t) {
        nb = g.nb; seg = t & 7u;
        const size_t pitch = (size_t)g.nb * kQ8Block;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = (t >> 3) + 32u * h;
            ga[h] = g.a + min(row0 + row, g.e.m - 1u) * pitch;
            lds_e[h] = row * kQ8Pitch + seg * 16u;
        }
    }

    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, Q8Staged<B>& st) const {
        const uint32_t eb = kb0 + (seg >> 1);
        const size_t off = (size_t)(TAIL ? min(eb, nb - 1u) : eb) * kQ8Block + 16u * (seg & 1u);
        st.a[0] = *reinterpret_cast<const v4u*>(ga[0] + off); st.a[1] = *reinterpret_cast<const v4u*>(ga[1] + off);
        bmap.template load<TAIL>(kb0, st.b);
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Q8Staged<B>& st) const { q8_store_staged<B, 2>(buf, lds_e, bmap, st); }
};

template <typename B>
__global__ __launch_bounds__(kBlock, B::kMinBlocks) void q8_gemm_kernel(const Int8GemmArgs g) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kQ8BufBytes<B>];
    q8_tile<B>(g.e, g.nb, stage, [&g](uint32_t row0, uint32_t col0, uint32_t t) { return GemmMap<B>(g, row0, col0, t); });
}

// the body of ppqhip_int8_gemm / ppqhip_int4_gemm: `what` names the entry point in its refusals, `id` books the launch
template <typename B>
int q8_gemm(const char* what, KernelId id, const int8_t* a, const void* b, const Int8TailHost& h, int64_t m, int64_t n, int64_t k, void* stream) {
    if (int st = check_int8_tail(what, "c", h)) return st;
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kQ8Max || n > kQ8Max || k > kQ8Max) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t nb = (k + kQ8Block - 1) / kQ8Block, kp = nb * kQ8Block, b_row = nb * B::kBlockBytes;
    if (nb > 0 && (a == nullptr || b == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (nb > 0 && (!aligned16(a) || !aligned16(b))) { set_error("%s: operands, c and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    std::vector<Span> ins;
    if (nb > 0 && kp < kQ8MaxK) { ins.push_back(span_of(a, m * kp)); ins.push_back(span_of(static_cast<const uint8_t*>(b), n * b_row)); }
    // booked: the operands once, the column data and every output and the residual; the launch does 2 m n kp integer operations
    const double bytes = (double)m * (double)kp + (double)n * (double)b_row;

    Int8GemmArgs g;
    g.a = reinterpret_cast<const uint8_t*>(a); g.b = static_cast<const uint8_t*>(b); g.nb = (uint32_t)nb;
    return launch_q8_tiles(what, "c", id, h, m, n, kp, ins, bytes, stream, g.e, [&g](uint32_t blocks, hipStream_t s) {
        hipLaunchKernelGGL(q8_gemm_kernel<B>, dim3(blocks), dim3(kBlock), 0, s, g);
    });
}

#endif  // __HIPCC__

}  // namespace ppqhip
