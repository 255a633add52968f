// mx_int8_tile.hpp -- what the two kernels on the int8 MFMA of gfx950 (v_mfma_i32_16x16x32_i8) share: mx_int8_gemm.hip (DESIGN.md
// section 9.19) and mx_int8_conv.hip (section 9.20).  A workgroup of 256 threads owns a 64 x 64 tile of the result; per K-chunk of 4 MX
// blocks it stages 64 rows of each operand (128 bytes each, pitch 144) and their 4 scale codes per row in LDS, double buffered.  Here
// are the stage's geometry, what a thread carries into it and where it puts it, the multiply of a staged chunk, the NaN flags and the
// store of the tile.  What a kernel adds is where a thread's share of a chunk comes from in global memory: a packed row (the GEMM) or a
// gathered one (the convolution).
#pragma once
#include "common.hpp"
#include "mx_mfma.hpp"

namespace ppqhip {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kI8Pitch = kGemmStepBlocks * kMxBlock + 16u;                  // 144: a staged row of 4 blocks, padded
constexpr uint32_t kI8TileBytes = kGemmEdge * kI8Pitch;                          // 64 rows of one operand
constexpr uint32_t kI8ScaleBytes = kGemmEdge * kGemmStepBlocks;                  // their 4 codes each
constexpr uint32_t kI8BufBytes = 2u * kI8TileBytes + 2u * kI8ScaleBytes;         // A, B, A's scales, B's scales
constexpr int kI8ExpBias = 2 * 127 + 12;                                         // the two E8M0 biases and the two 1 / 64
static_assert(kI8Pitch % 16u == 0 && kI8BufBytes % 16u == 0, "16-byte stores into the stage");
static_assert(kGemmEdge * kGemmStepBlocks * kMxBlock == 2u * 16u * (uint32_t)kBlock, "two 16-byte loads per thread and operand");
static_assert(2u * kI8ScaleBytes == 2u * (uint32_t)kBlock, "two scale codes per thread");

// what a thread carries from global memory to LDS for one chunk: 2 x 16 bytes of A, 2 x 16 bytes of B, 2 scale codes
struct Staged {
    v4u a0, a1, b0, b1;                         // the thread's segment of rows t >> 3 and 32 + (t >> 3) of A and of B
    uint32_t s;                                   // the codes of blocks kb0 + 2 pair and + 1 in bytes 0 and 1
};

// The LDS store of a staged chunk: lds_e[h] = row * kI8Pitch + seg * 16 for the thread's rows t >> 3 and 32 + (t >> 3), lds_s the
// place of its two scale codes behind the two element tiles.
__device__ __forceinline__ void store_staged(uint8_t* buf, const uint32_t (&lds_e)[2], uint32_t lds_s, const Staged& st) {
    *reinterpret_cast<v4u*>(buf + lds_e[0]) = st.a0; *reinterpret_cast<v4u*>(buf + lds_e[1]) = st.a1;
    *reinterpret_cast<v4u*>(buf + kI8TileBytes + lds_e[0]) = st.b0; *reinterpret_cast<v4u*>(buf + kI8TileBytes + lds_e[1]) = st.b1;
    *reinterpret_cast<uint16_t*>(buf + lds_s) = (uint16_t)st.s;
}

// The wave's 2 x 2 tiles over the `live` (1 .. 4; 4 unless TAIL) blocks of the chunk staged in buf: per block and tile one MFMA
// from a zero accumulator, then per output the conversion, the scaling by 2^(sa + sb - 266) and the float32 add.
template <bool TAIL>
__device__ __forceinline__ void chunk_tiles(const uint8_t* buf, uint32_t wm, uint32_t wn, uint32_t r, uint32_t grp, uint32_t live,
                                            v4f (&acc)[kGemmWaveTiles][kGemmWaveTiles]) {
    constexpr int T = kGemmWaveTiles;
    const uint8_t* la = buf + (wm + r) * kI8Pitch + grp * 8u;
    const uint8_t* lb = buf + kI8TileBytes + (wn + r) * kI8Pitch + grp * 8u;
    uint4 sa[T]; uint32_t sb[T];                                                 // sa[i]: rows 4 grp + q of tile i, 4 codes each
#pragma unroll
    for (int i = 0; i < T; i++) {
        sa[i] = *reinterpret_cast<const uint4*>(buf + 2u * kI8TileBytes + (wm + i * kGemmTile + grp * 4u) * kGemmStepBlocks);
        sb[i] = *reinterpret_cast<const uint32_t*>(buf + 2u * kI8TileBytes + kI8ScaleBytes + (wn + i * kGemmTile + r) * kGemmStepBlocks);
    }
#pragma unroll
    for (uint32_t b = 0; b < kGemmStepBlocks; b++) {
        if (TAIL && b >= live) break;                                            // wave-uniform
        long a[T], bb[T];
#pragma unroll
        for (int i = 0; i < T; i++) {
            a[i] = *reinterpret_cast<const long*>(la + i * kGemmTile * kI8Pitch + b * kMxBlock);
            bb[i] = *reinterpret_cast<const long*>(lb + i * kGemmTile * kI8Pitch + b * kMxBlock);
        }
        int ea[T][4], eb[T];
#pragma unroll
        for (int i = 0; i < T; i++) {
            const uint32_t w[4] = {sa[i].x, sa[i].y, sa[i].z, sa[i].w};
#pragma unroll
            for (int q = 0; q < 4; q++) ea[i][q] = (int)((w[q] >> (8u * b)) & 0xffu);
            eb[i] = (int)((sb[i] >> (8u * b)) & 0xffu) - kI8ExpBias;
        }
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++) {
                const v4i p = __builtin_amdgcn_mfma_i32_16x16x32_i8(a[i], bb[j], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[i][j][q] = acc[i][j][q] + __builtin_ldexpf((float)p[q], ea[i][q] + eb[j]);
            }
    }
}

// The NaN flags of a workgroup: nan_flags[2 * kGemmEdge], rows of A, then rows of B (columns of C).  Thread t stages the scale codes
// of row (t & 127) >> 1 of operand t >> 7: it clears its flag before the K loop and raises it after the loop when one of the live codes
// it staged was 0xFF -- at least one barrier lies between the two, and one more before the flags are read.
__device__ __forceinline__ void clear_nan_flags(uint32_t* nan_flags, uint32_t t) {
    if (t < 2u * kGemmEdge) nan_flags[t] = 0u;
}
__device__ __forceinline__ void raise_nan_flag(uint32_t* nan_flags, uint32_t t, bool bad) {
    if (bad) nan_flags[(t >> 7) * kGemmEdge + ((t & 127u) >> 1)] = 1u;           // after the zeroing: at least one barrier lies between
}

// The store of the wave's 2 x 2 tiles into c [m, n]: + bias, 0x7fc00000 where the row or the column is flagged; rows past m and columns
// past n are not stored.
__device__ __forceinline__ void store_tiles(const v4f (&acc)[kGemmWaveTiles][kGemmWaveTiles], const uint32_t* nan_flags, const float* gbias,
                                            float* c, uint32_t m, uint32_t n, uint32_t row0, uint32_t col0, uint32_t wm, uint32_t wn,
                                            uint32_t r, uint32_t grp) {
    constexpr int T = kGemmWaveTiles;
#pragma unroll
    for (int j = 0; j < T; j++) {
        const uint32_t lc = wn + j * kGemmTile + r, col = col0 + lc;
        if (col >= n) continue;
        const float bias = gbias != nullptr ? gbias[col] : 0.f;
        const bool col_nan = nan_flags[kGemmEdge + lc] != 0u;
#pragma unroll
        for (int i = 0; i < T; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t lr = wm + i * kGemmTile + grp * 4u + q, row = row0 + lr;
                const bool nan = col_nan || nan_flags[lr] != 0u;
                const float v = gbias != nullptr ? acc[i][j][q] + bias : acc[i][j][q];
                if (row < m) c[(size_t)row * n + col] = nan ? __uint_as_float(0x7fc00000u) : v;
            }
        }
    }
}

}  // namespace ppqhip
