// int8_skinny.hpp -- the GEMM of the linear INT8 family for 1 <= M <= 64, where the layer is bound by reading the weight once
// (DESIGN.md section 9.26).  C[M, N] = requant(tail(float32(sum_k B[n, k] (A[m, k] - zx)) * mul[n])) on v_mfma_i32_16x16x32_i8 with
// the operands, the contract and the per-output chain (q8_value, q8_code) of int8_gemm.hpp; tests/int8_reference.py is the
// specification.  From int8_tile.hpp this file takes the tail (Int8Tail, Int8TailHost, check_int8_tail, launch_q8, q8_value, q8_code)
// and nothing of the 64 x 64 frame: the shape here is a different one.
//
// Shape.  A workgroup of 256 lanes owns 16 columns of the result -- one MFMA column tile -- and ALL M rows: MT = ceil(M / 16) row
// tiles, 1, 2 or 4.  The grid is the ceil32(N) / 16 column tiles, so that every weight byte is read from memory exactly once, by one
// workgroup.  K is cut into pieces of 64 bytes of a weight row (64 int8 codes, 128 int4 codes); piece p belongs to wave p & 3, so the
// four waves read adjacent pieces of the same 16 weight rows at the same time, 256 contiguous bytes a row per round.  Each wave chains
// its share of K through accumulators of its own; there is no LDS and no barrier in the K loop.  Integer sums are exact in any
// order, so the split gives the bits of the tile kernel.
//
// Fragments come straight from global memory as 16-byte loads, with K permuted inside the registers.  The MFMA wants 8 bytes a lane:
// row (A) or column (B) l & 15, K-group l >> 4.  Which k a fragment slot holds does not matter as long as A and B agree:
//   int8 weight: lane (r, grp) loads bytes 64 p + 16 grp .. + 15 of weight row r and of each of its MT rows of A; the low 8 bytes of
//     both feed one MFMA, the high 8 bytes a second: two MFMAs per row tile cover the piece.
//   int4 weight: the lane's 16 bytes are 4 dwords, the codes 128 p + 32 grp + 8 d .. + 7 in dword d, which the layout of section
//     9.23 turns into a fragment with (p << 4) & 0xf0f0f0f0, p & 0xf0f0f0f0 (16 w, the accumulators hold 16 I); the matching bytes
//     of A are 128 p + 32 grp .. + 31, two 16-byte loads: four MFMAs per row tile and weight load.
// A B fragment is reused from registers for all MT row tiles.  A is at most 64 x Kp bytes and stays in L2; each wave reads its K
// share of it once.  The loop is pipelined through registers: a step is kU pieces per wave, and the loads of step s + 1 are issued
// before the MFMAs of step s (two register sets, used in turn).  Consecutive MFMAs alternate between two accumulator sets, so that
// with MT == 1 no MFMA waits for the one before it.
//
// Tail of K: Kp is a multiple of 32, so a lane's 16 bytes of a weight row are wholly inside it or wholly outside; outside, the
// addresses (of B and of A) fall back to the start of the row and the B registers are zeroed.  A piece at or past the end is neither
// loaded nor multiplied.  Rows past M and weight rows past N are clamped copies, not stored.
//
// Reduce and epilogue.  Every wave writes its MT partial tiles to LDS (MT KiB a wave); after the kernel's one barrier wave w < MT adds
// the four partials of row tile w to -zx * sums[col] (shifted by 4 for int4, the total then shifted back, exactly) and runs q8_value
// and q8_code on it.  c is stored as computed; the 16 x 16 codes are gathered through 256 bytes of LDS of the wave's own and leave as
// one 16-byte store per row.  A column tile wholly at or past N (N % 32 in 1 .. 16) reads nothing and writes zy into its columns of q.
#pragma once
#include "common.hpp"
#include "job_table.hpp"
#include "int8_tile.hpp"

namespace ppqhip {

constexpr uint32_t kSkCols = 16;                  // columns of the result per workgroup: one MFMA column tile
constexpr uint32_t kSkWaves = kBlock / kWave;     // the K split: piece p belongs to wave p & 3
constexpr uint32_t kSkPieceBytes = 64;            // bytes of a weight row per piece: 16 per K-group of the MFMA
constexpr int64_t kSkMaxM = 64;                   // more rows are refused
static_assert(kSkWaves == 4 && kSkPieceBytes == 4u * 16u, "a piece is one 16-byte load per lane of a wave");

struct Int8SkinnyArgs {
    const uint8_t* a; const uint8_t* b;           // [m, kp], [n, kp / kPerByte of the codec]
    uint32_t kp;                                  // ceil32(k)
    Int8Tail e;                                   // tiles_n is not used
};

#if defined(__HIPCC__)

// ---- the weight codecs: what a lane's 16 bytes of a weight row hold and how they become fragments -------------------------------------
// kPerByte codes a byte; kSeg the codes of a lane's load and kPiece those of a piece; kALoads the 16-byte loads of A that match
// it; kFrags the MFMAs per row tile; kShift log2 of what the fragments are scaled by; kU the pieces of a step (section 9.26: the
// largest power of two at which the MT == 4 instance keeps both register sets in the 256 architectural VGPRs).
struct SkB8 {
    static constexpr uint32_t kPerByte = 1, kSeg = 16, kPiece = 64, kALoads = 1, kFrags = 2, kU = 4;
    static constexpr int kShift = 0;
    static __device__ __forceinline__ long frag(const v4u& b, int d) { return (long)(((uint64_t)b[2 * d + 1] << 32) | b[2 * d]); }
};
struct SkB4 {
    static constexpr uint32_t kPerByte = 2, kSeg = 32, kPiece = 128, kALoads = 2, kFrags = 4, kU = 2;
    static constexpr int kShift = 4;
    static __device__ __forceinline__ long frag(const v4u& b, int d) {
        const uint32_t p = b[d], lo = (p << 4) & 0xf0f0f0f0u, hi = p & 0xf0f0f0f0u;
        return (long)(((uint64_t)hi << 32) | lo);
    }
};

// what a lane carries of one step: per piece its 16 bytes of the weight row and the matching bytes of its MT rows of A
template <typename B, int MT>
struct SkRegs {
    v4u b[B::kU];
    v4u a[B::kU][MT][B::kALoads];
};

// Where a lane's loads lie, and the step: pieces p0 + 4 u, u < kU, of a wave whose first piece of the step is p0.  TAIL: the step
// reaches past Kp -- a piece at or past `pieces` is skipped (wave-uniform), a lane's segment past Kp reads the start of its rows and
// multiplies zeros.
template <typename B, int MT>
struct SkMap {
    const uint8_t* gb; const uint8_t* ga[MT];
    uint32_t seg, kp, pieces;

    __device__ __forceinline__ SkMap(const Int8SkinnyArgs& g, uint32_t col0, uint32_t r, uint32_t grp) {
        kp = g.kp; pieces = (g.kp + B::kPiece - 1u) / B::kPiece; seg = grp * B::kSeg;
        gb = g.b + min(col0 + r, g.e.n - 1u) * (size_t)(g.kp / B::kPerByte);
#pragma unroll
        for (int i = 0; i < MT; i++) ga[i] = g.a + min(i * kQ8Tile + r, g.e.m - 1u) * (size_t)g.kp;
    }

    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t p0, SkRegs<B, MT>& st) const {
#pragma unroll
        for (uint32_t u = 0; u < B::kU; u++) {
            const uint32_t p = p0 + kSkWaves * u;
            if (TAIL && p >= pieces) break;                                      // wave-uniform
            uint32_t k0 = p * B::kPiece + seg;
            const bool live = !TAIL || k0 < kp;
            if (!live) k0 = 0u;
            const v4u b = *reinterpret_cast<const v4u*>(gb + k0 / B::kPerByte);
            st.b[u] = live ? b : v4u{0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < MT; i++)
#pragma unroll
                for (uint32_t h = 0; h < B::kALoads; h++) st.a[u][i][h] = *reinterpret_cast<const v4u*>(ga[i] + k0 + 16u * h);
        }
    }

    // the MFMAs of a loaded step: per piece kFrags fragments of B, each against the same 8 bytes of every row tile
    template <bool TAIL>
    __device__ __forceinline__ void multiply(uint32_t p0, const SkRegs<B, MT>& st, v4i (&acc)[2][MT]) const {
#pragma unroll
        for (uint32_t u = 0; u < B::kU; u++) {
            if (TAIL && p0 + kSkWaves * u >= pieces) break;                      // wave-uniform
#pragma unroll
            for (int d = 0; d < (int)B::kFrags; d++) {
                const long bf = B::frag(st.b[u], d);
#pragma unroll
                for (int i = 0; i < MT; i++) {
                    const v4u& w = st.a[u][i][d >> 1];                           // bytes 8 d .. + 7 of the lane's share of A
                    const long af = (long)(((uint64_t)w[2 * (d & 1) + 1] << 32) | w[2 * (d & 1)]);
                    acc[d & 1][i] = __builtin_amdgcn_mfma_i32_16x16x32_i8(af, bf, acc[d & 1][i], 0, 0, 0);
                }
            }
        }
    }

    // a step whose last piece ends inside Kp needs no tail handling
    __device__ __forceinline__ bool whole(uint32_t p0) const { return (p0 + kSkWaves * (B::kU - 1u) + 1u) * B::kPiece <= kp; }
    __device__ __forceinline__ void load(uint32_t p0, SkRegs<B, MT>& st) const {
        if (whole(p0)) load<false>(p0, st); else load<true>(p0, st);
    }
    __device__ __forceinline__ void multiply(uint32_t p0, const SkRegs<B, MT>& st, v4i (&acc)[2][MT]) const {
        if (whole(p0)) multiply<false>(p0, st, acc); else multiply<true>(p0, st, acc);
    }
};

template <typename B, int MT>
__global__ __launch_bounds__(kBlock) void q8_skinny_kernel(const Int8SkinnyArgs g) {
    __shared__ v4i part[kSkWaves * MT * kWave];                                  // [wave][row tile][lane]: the waves' partial tiles
    __shared__ __attribute__((aligned(16))) uint8_t codes[MT][kQ8Tile * kSkCols]; // a reducing wave's 16 rows of 16 codes
    const Int8Tail& e = g.e;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t col0 = blockIdx.x * kSkCols;
    const uint32_t pad_code = (uint32_t)(int)e.zy & 0xffu;

    if (col0 >= e.n) {                                                           // a tile of padding columns only: nothing to read
        const uint32_t w = pad_code * 0x01010101u;
        if (e.q != nullptr && t < e.m) *reinterpret_cast<v4u*>(e.q + (size_t)t * e.op + col0) = v4u{w, w, w, w};
        return;
    }

    v4i acc[2][MT];
#pragma unroll
    for (int i = 0; i < MT; i++) { acc[0][i] = v4i{0, 0, 0, 0}; acc[1][i] = v4i{0, 0, 0, 0}; }
    if (g.kp > 0u) {                                                             // kp == 0: the operands may be null
        const SkMap<B, MT> map(g, col0, r, grp);
        constexpr uint32_t kStride = kSkWaves * B::kU;                           // pieces between a wave's steps
        // the wave's steps start at pieces wave, wave + kStride, ...; two register sets take turns
        SkRegs<B, MT> s0, s1;
        uint32_t p0 = wave;
        if (p0 < map.pieces) map.load(p0, s0);
        while (p0 < map.pieces) {
            const uint32_t p1 = p0 + kStride, p2 = p1 + kStride;
            if (p1 < map.pieces) map.load(p1, s1);
            map.multiply(p0, s0, acc);
            if (p1 >= map.pieces) break;
            if (p2 < map.pieces) map.load(p2, s0);
            map.multiply(p1, s1, acc);
            p0 = p2;
        }
    }

#pragma unroll
    for (int i = 0; i < MT; i++) part[(wave * MT + i) * kWave + lane] = acc[0][i] + acc[1][i];
    __syncthreads();
    if (wave >= (uint32_t)MT || wave * kQ8Tile >= e.m) return;                   // wave-uniform: the reducing waves go on, one per live row tile

    // row tile `wave`: lane l holds column col0 + r, rows 16 wave + 4 grp + q
    v4i sum = part[wave * kWave + lane];
#pragma unroll
    for (uint32_t w = 1; w < kSkWaves; w++) sum += part[(w * MT + wave) * kWave + lane];
    const bool col_in = col0 + r < e.n;
    const uint32_t col = min(col0 + r, e.n - 1u);
    const int start = e.sums != nullptr ? (int)((0u - (uint32_t)e.zx * (uint32_t)e.sums[col]) << B::kShift) : 0;
    sum = (sum + v4i{start, start, start, start}) >> B::kShift;                  // a multiple of 2^kShift: the shift back is exact
    const float mul = e.mul[col], bias = e.bias != nullptr ? e.bias[col] : 0.f;
    uint8_t* stage = codes[wave];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t tr = grp * 4u + q, row = wave * kQ8Tile + tr;
        const size_t at = (size_t)min(row, e.m - 1u) * e.n + col;                // rows past m: copies of the last one, not stored
        const float v = q8_value(e, sum[q], mul, bias, e.residual != nullptr ? e.residual[at] : 0.f);
        if (e.c != nullptr && row < e.m && col_in) e.c[at] = v;
        if (e.q != nullptr) stage[tr * kSkCols + r] = (uint8_t)(col_in ? q8_code(e, v) & 0xffu : pad_code);
    }
    if (e.q == nullptr) return;                                                  // wave-uniform
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                        // the wave's own writes, read by its own lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t row = wave * kQ8Tile + lane;
    if (lane < (uint32_t)kQ8Tile && row < e.m)                                   // col0 + 16 <= op: col0 < n and col0 % 16 == 0
        *reinterpret_cast<v4u*>(e.q + (size_t)row * e.op + col0) = *reinterpret_cast<const v4u*>(stage + lane * kSkCols);
}

// the body of ppqhip_int8_gemm_skinny / ppqhip_int4_gemm_skinny: the checks of q8_gemm (int8_gemm.hpp) in its order, and m <= 64
template <typename B>
int q8_skinny(const char* what, KernelId id, const int8_t* a, const void* b, const Int8TailHost& h, int64_t m, int64_t n, int64_t k, void* stream) {
    if (int st = check_int8_tail(what, "c", h)) return st;
    if (m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kQ8Max || n > kQ8Max || k > kQ8Max) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (m > kSkMaxM) { set_error("%s: m = %lld: the skinny kernel takes at most %lld rows", what, (long long)m, (long long)kSkMaxM); return PPQHIP_ERR_INVALID_VALUE; }
    if (m == 0 || n == 0) return PPQHIP_OK;
    const int64_t kp = (k + kQ8Block - 1) / kQ8Block * kQ8Block, b_row = kp / B::kPerByte;
    if (kp > 0 && (a == nullptr || b == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (kp > 0 && (!aligned16(a) || !aligned16(b))) { set_error("%s: operands, c and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    std::vector<Span> ins;
    if (kp > 0 && kp < kQ8MaxK) { ins.push_back(span_of(a, m * kp)); ins.push_back(span_of(static_cast<const uint8_t*>(b), n * b_row)); }
    const double bytes = (double)m * (double)kp + (double)n * (double)b_row;      // booked as q8_gemm books them

    Int8SkinnyArgs g;
    g.a = reinterpret_cast<const uint8_t*>(a); g.b = static_cast<const uint8_t*>(b); g.kp = (uint32_t)kp;
    g.e.tiles_n = make_fastdiv(1u);
    const int64_t tiles = (n + kQ8Block - 1) / kQ8Block * (kQ8Block / kSkCols);   // ceil32(n) / 16: q's padding columns have a tile too
    return launch_q8(what, "c", id, h, m, n, kp, tiles, ins, bytes, stream, g.e, [&g, m](uint32_t blocks, hipStream_t s) {
        if (m <= 16) hipLaunchKernelGGL((q8_skinny_kernel<B, 1>), dim3(blocks), dim3(kBlock), 0, s, g);
        else if (m <= 32) hipLaunchKernelGGL((q8_skinny_kernel<B, 2>), dim3(blocks), dim3(kBlock), 0, s, g);
        else hipLaunchKernelGGL((q8_skinny_kernel<B, 4>), dim3(blocks), dim3(kBlock), 0, s, g);
    });
}

#endif  // __HIPCC__

}  // namespace ppqhip
