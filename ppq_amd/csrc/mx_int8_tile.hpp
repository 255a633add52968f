// mx_int8_tile.hpp -- what the two kernels on the int8 MFMA of gfx950 (v_mfma_i32_16x16x32_i8) share: mx_int8_gemm.hip (DESIGN.md
// section 9.19) and mx_int8_conv.hip (section 9.20).  A workgroup of 256 threads owns a 64 x 64 tile of the result; per K-chunk of 4 MX
// blocks it stages 64 rows of each operand (128 bytes each, pitch 144) and their 4 scale codes per row in LDS, double buffered.  Here
// are the stage's geometry, what a thread carries into it and where it puts it, the multiply of a staged chunk, the NaN flags and the
// store of the tile.  What a kernel adds is where a thread's share of a chunk comes from in global memory: a packed row (the GEMM) or a
// gathered one (the convolution).  Below those: the fused epilogue of both (section 9.21) -- fused_tiles, which hands the tile to
// fused_epilogue of mx_mfma.hpp -- and the host frame of the two fused entry points.
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

// ---- the fused epilogue on the int8 tile -------------------------------------------------------------------
// A wave of this tile owns 32 rows x 32 columns with acc[i][j][q] at row wm + 16 i + 4 grp + q, column wn + 16 j + r: the layout
// fused_epilogue of mx_mfma.hpp is written for, and 32 columns that start at a multiple of 32 are one output MX block per row.  So the
// int8 kernels call that epilogue as it is -- one block maximum, one coder (its is_int arm), one code gather -- and add two things.
//
// The NaN masks.  fused_epilogue takes, per 16 x 16 tile, a 16-bit mask of flagged rows and one of flagged columns; the int8 kernels
// keep one word per row and column of the workgroup in LDS (nan_flags).  After the kernel's final barrier lane l reads the flag of
// row wm + 16 i + (l & 15) resp. column wn + 16 j + (l & 15); a ballot puts the 16 flags of lanes 0 .. 15 in the low bits (the three
// other lane groups read the same words; tile_flags ORs the four copies).
//
// The LDS of the code gather.  No LDS is declared for it: wave w takes bytes [w * kFusedStageBytes, + kFusedStageBytes) of the
// operand stage.  The stage's last readers are the chunk_tiles of the last K chunk, and every wave passes the barrier that ends that
// chunk, and the kernel's final barrier after it, before any wave reaches its epilogue: no fragment read can follow a code write.
// From there on a wave touches its own slice only, so the waves that returned at the edge are not waited for.
static_assert(kGemmWaves * kGemmWaves * kFusedStageBytes <= kI8BufBytes, "the four waves' code stages fit the first operand buffer");

__device__ __forceinline__ void fused_tiles(const v4f (&acc)[kGemmWaveTiles][kGemmWaveTiles], const uint32_t* nan_flags, const float* bias,
                                            float* c, uint32_t m, uint32_t n, uint32_t row0, uint32_t col0, uint32_t wm, uint32_t wn,
                                            uint32_t lane, const MxFusedOut& f, uint8_t* operand_stage) {
    constexpr int T = kGemmWaveTiles;
    const uint32_t r = lane & 15u, wave = (wm / (T * kGemmTile)) * kGemmWaves + wn / (T * kGemmTile);
    uint32_t rows_nan[T], cols_nan[T];
#pragma unroll
    for (int i = 0; i < T; i++) {
        rows_nan[i] = tile_flags(nan_flags[wm + i * kGemmTile + r]);
        cols_nan[i] = tile_flags(nan_flags[kGemmEdge + wn + i * kGemmTile + r]);
    }
    fused_epilogue(acc, rows_nan, cols_nan, bias, c, m, n, row0 + wm, col0 + wn, lane, f, operand_stage + wave * kFusedStageBytes);
}

// ---- the host side of the two fused entry points ----------------------------------------------------------------------------------------
// What ppqhip_mx_int8_gemm_fused / ppqhip_mx_int8_conv2d_fused check about their outputs before anything else: the pointer rules of
// ppqhip_mx_gemm_fused; there is no out_format -- these kernels pack MXINT8 -- so f.fmt is that format's.
inline int check_int8_fused(const char* what, const char* float_name, const float* c, const MxFusedHost& fused, MxFusedOut& f) {
    make_mx_fmt(PPQHIP_MXINT8, &f.fmt);
    return check_fused_pointers(what, float_name, c, fused.out_elements, fused.out_scales);
}

// The launch of an int8 entry point, from its grid check on (the int8 side of launch_mx_tiles): `ins`, `outs` and `bytes` are the
// plain launch's and `fused` is null for it.  launch(blocks, stream, f...) starts the plain kernel without f, the fused one with it.
template <typename Launch>
inline int launch_int8_tiles(const char* what, KernelId plain_id, KernelId fused_id, const MxFusedHost* fused, MxFusedOut& f, int64_t m,
                             int64_t n, std::vector<Span>& ins, std::vector<Span>& outs, double bytes, void* stream, FastDiv& tiles_n_div,
                             Launch&& launch) {
    const int64_t tiles_m = (m + kGemmEdge - 1) / kGemmEdge, tiles_n = (n + kGemmEdge - 1) / kGemmEdge;
    if (tiles_m * tiles_n > kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (fused != nullptr) {
        if (int st = book_fused(what, *fused, m, n, ins, outs, bytes, f)) return st;
    }
    if (int st = check_overlap(what, ins, outs)) return st;
    tiles_n_div = make_fastdiv((uint32_t)tiles_n);
    const uint32_t blocks = (uint32_t)(tiles_m * tiles_n);
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(fused != nullptr ? fused_id : plain_id, bytes, s);
    if (fused != nullptr) launch(blocks, s, f);
    else launch(blocks, s);
    return finish_launch(what);
}

}  // namespace ppqhip
