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
#include "common.hpp"
#include "job_table.hpp"
#include "mx_mfma.hpp"

namespace ppqhip {
namespace {

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

struct MxInt8Args {
    const uint8_t* ae; const uint8_t* as;         // A: elements [m, nb * 32], scales [m, nb]
    const uint8_t* be; const uint8_t* bs;         // B: elements [n, nb * 32], scales [n, nb]
    const float* bias;                            // [n] or null
    float* c;                                     // [m, n]
    uint32_t m, n, nb;
    FastDiv tiles_n;
};

// what a thread carries from global memory to LDS for one chunk: 2 x 16 bytes of A, 2 x 16 bytes of B, 2 scale codes
struct Staged {
    v4u a0, a1, b0, b1;                         // the thread's segment of rows t >> 3 and 32 + (t >> 3) of A and of B
    uint32_t s;                                   // the codes of blocks kb0 + 2 pair and + 1 in bytes 0 and 1
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

    __device__ __forceinline__ void store(uint8_t* buf, const Staged& st) const {
        *reinterpret_cast<v4u*>(buf + lds_e[0]) = st.a0; *reinterpret_cast<v4u*>(buf + lds_e[1]) = st.a1;
        *reinterpret_cast<v4u*>(buf + kI8TileBytes + lds_e[0]) = st.b0; *reinterpret_cast<v4u*>(buf + kI8TileBytes + lds_e[1]) = st.b1;
        *reinterpret_cast<uint16_t*>(buf + lds_s) = (uint16_t)st.s;
    }
};

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

__global__ __launch_bounds__(kBlock) void mx_int8_gemm_kernel(const MxInt8Args g) {
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
    if (t < 2u * kGemmEdge) nan_flags[t] = 0u;

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
        if (bad) nan_flags[(t >> 7) * kGemmEdge + ((t & 127u) >> 1)] = 1u;       // after the zeroing: at least one barrier lies between
    }
    __syncthreads();
    if (!busy) return;

#pragma unroll
    for (int j = 0; j < T; j++) {
        const uint32_t lc = wn + j * kGemmTile + r, col = col0 + lc;
        if (col >= g.n) continue;
        const float bias = g.bias != nullptr ? g.bias[col] : 0.f;
        const bool col_nan = nan_flags[kGemmEdge + lc] != 0u;
#pragma unroll
        for (int i = 0; i < T; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t lr = wm + i * kGemmTile + grp * 4u + q, row = row0 + lr;
                const bool nan = col_nan || nan_flags[lr] != 0u;
                const float v = g.bias != nullptr ? acc[i][j][q] + bias : acc[i][j][q];
                if (row < g.m) g.c[(size_t)row * g.n + col] = nan ? __uint_as_float(0x7fc00000u) : v;
            }
        }
    }
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_int8_gemm(const uint8_t* a_elements, const uint8_t* a_scales, const uint8_t* b_elements, const uint8_t* b_scales,
                                   const float* bias, float* c, int64_t m, int64_t n, int64_t k, void* stream) {
    const char* what = "mx_int8_gemm";
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kMxMax || n > kMxMax || k > kMxMax) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t nb = (k + kMxBlock - 1) / kMxBlock;
    if (c == nullptr || (nb > 0 && (a_elements == nullptr || a_scales == nullptr || b_elements == nullptr || b_scales == nullptr))) {
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
    outs.push_back(span_of(c, m * n));
    const int64_t tiles_m = (m + kGemmEdge - 1) / kGemmEdge, tiles_n = (n + kGemmEdge - 1) / kGemmEdge;
    if (tiles_m * tiles_n > kMxMax) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (int st = check_overlap(what, ins, outs)) return st;
    // booked: the operands and 4 m n bytes of C; the launch does 2 m n nb 32 integer operations
    const double bytes = ((double)m + (double)n) * (double)nb * (double)(kMxBlock + 1) + 4.0 * (double)m * (double)n;

    MxInt8Args g;
    g.ae = a_elements; g.as = a_scales; g.be = b_elements; g.bs = b_scales; g.bias = bias; g.c = c;
    g.m = (uint32_t)m; g.n = (uint32_t)n; g.nb = (uint32_t)nb;
    g.tiles_n = make_fastdiv((uint32_t)tiles_n);
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_MX_INT8_GEMM, bytes, s);
    hipLaunchKernelGGL(mx_int8_gemm_kernel, dim3((uint32_t)(tiles_m * tiles_n)), dim3(kBlock), 0, s, g);
    return finish_launch(what);
}
