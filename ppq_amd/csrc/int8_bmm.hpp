// int8_bmm.hpp -- the batched matmul of TWO activations of the linear INT8 family: attention's Q.K^T and P.V.
// For every batch g:  C[g, m, n] = requant(tail(float32(sum_k (A[g, m, k] - za) (B[g, k, n] - zb)) * mul)) on v_mfma_i32_16x16x32_i8,
// the per-output chain (q8_value, q8_code, q8_epilogue) that of int8_tile.hpp; tests/int8_bmm_reference.py is the specification.
// What sets it apart from int8_gemm.hpp: all batches run in one launch; BOTH operands carry a zero point and neither comes with
// sums; and B lies in memory in one of two layouts.
//
// Operands.  A [batch, M, Kp] int8 codes, Kp = ceil32(K), bytes K .. Kp - 1 of a row the code za.  B is
//   TB (a . b^T, Q.K^T): [batch, N, Kp], packed along the reduction axis like A, its padding the code zb;
//   !TB (a . b, P.V):    [batch, K, Np], Np = ceil32(N), packed along N: the K rows are not padded, rows K .. Kp - 1 do not exist.
// mul is ONE float32 in device memory, sa * sb.
//
// Shape.  The 64 x 64 tile of the family: 2 x 2 waves of 2 x 2 MFMA tiles, chunks of 128 bytes of K through the double-buffered LDS
// stage of int8_tile.hpp (A rows at pitch 144), one barrier a chunk.  The workgroup index is (batch, row tile, column tile), the
// column tile fastest; operand and output pointers are offset by the batch, nothing is shared between batches.  At the shapes this
// kernel is for (197 x 197 x 64, 197 x 64 x 197) there are one or two chunks: the loop is load latency and epilogue, so the tile stays
// at the shape whose epilogue stores whole 32-byte code rows and whose 16 workgroups a batch fill the chip at 96 batches.
//
// Zero points.  sum (a - za)(b - zb) = sum a b - za colsum_b[n] - zb rowsum_a[m] + Kp za zb, all sums over the padded range the MFMAs
// run over (the padding is (za, zb), so it adds 0 to the left side).  The kernel makes both sums from the fragments a lane already
// holds: two v_dot4_i32_i8 against 0x01010101 per 8-byte fragment and block.  A lane's partial covers its K-group; after the loop two
// xor-shuffles (16, 32) add the four K-groups.  The column sum of B then sits in lane l & 15 -- the accumulator's column.  The row sum
// of A sits by lane ROW (l & 15) and is fetched once for the accumulator rows 4 grp + q from lane 4 grp + q.  The kernel is
// instantiated on (za != 0, zb != 0): zb != 0 sums A's rows, za != 0 B's columns; symmetric operands run the plain loop.  Both waves
// of a tile row (column) make the same sums -- 4 dot4 per wave and block where both are needed twice over, against 4 MFMAs.
// Everything is modulo 2^32; the total fits int32 because Kp <= 32768 (the host refuses more): 32768 * 255 * 255 < 2^31.
//
// B packed along N.  A thread takes two 4 (k) x 4 (n) blocks of the chunk: four 4-byte global loads from four consecutive rows of B
// (16 lanes read 64 contiguous bytes of one row), transposes the block in registers with eight v_perm_b32 and writes four dwords
// into the B stage, which holds B^T as [n][k] rows exactly as the TB layout stages them -- the fragment reads and the MFMAs are the
// same code.  A row k >= K is not read: its dword is the code zb, which (b - zb) turns into 0.  The stage's pitch is 136 bytes here:
// the dword of column 4 n4 + j, k-quad k4 lies in bank (34 (4 n4 + j) + k4) mod 64 = (8 n4 + k4 + 34 j) mod 64; a wave's store has
// n4 = 0 .. 15 and four consecutive k4, which reach 32 different banks: 2-way, where the family's 144 would be 4-way (derived, not
// measured).  An 8-byte fragment read at pitch 136 starts at dword 34 r + 8 b + 2 grp: over the 32 lanes of a half wave these are
// 32 different even banks (34 r mod 64 is 4 i for even r and 34 + 4 i for odd r, i < 8, so grp = 0, 1 never meet): conflict-free,
// also derived.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "job_table.hpp"
#include "int8_tile.hpp"

namespace ppqhip {

constexpr int64_t kBmmMaxK = 32768;                                              // a longer padded reduction is refused: 32768 * 255 * 255 < 2^31
constexpr uint32_t kBmmPitchN = 136;                                             // pitch of the B stage when B is packed along N
static_assert(kBmmPitchN % 8u == 0 && kBmmPitchN >= kQ8ChunkBlocks * kQ8Block && kBmmPitchN <= kQ8Pitch, "8-byte fragment reads, inside the family's buffer");

struct Int8BmmArgs {
    const uint8_t* a; const uint8_t* b;
    uint32_t nb;                                  // Kp / 32
    uint32_t k;                                   // the rows of b that exist (!TB)
    int32_t zb;
    size_t a_batch, b_batch;                      // bytes between two batches of a and of b
    FastDiv tiles;                                // tiles per batch
    Int8Tail e;                                   // m, n, op of ONE batch; zx = za; mul [1]; residual, c, q of batch 0
};

#if defined(__HIPCC__)

// ---- B as [n, Kp]: the rows and segments of Q8B8 -------------------------------------------------------------------------------------
struct BmmBK {
    static constexpr uint32_t kPitch = kQ8Pitch;
    struct Regs { Q8B8::Regs r; };
    Q8B8::Map map;
    __device__ __forceinline__ BmmBK(const Int8BmmArgs& g, const uint8_t* b, uint32_t col0, uint32_t t) : map(b, g.nb, g.e.n, col0, t) {}
    __device__ __forceinline__ void load(uint32_t kb0, Regs& st) const { map.load<true>(kb0, st.r); }
    __device__ __forceinline__ void store(uint8_t* stage, const Regs& st) const { map.store(stage, st.r); }
};

// ---- B as [K, Np]: 4 x 4 blocks, transposed in registers -----------------------------------------------------------------------------
// block t + 256 h, h < 2, of the 32 (k-quads) x 16 (column quads) of a chunk: column quad idx & 15, k-quad idx >> 4
struct BmmBN {
    static constexpr uint32_t kPitch = kBmmPitchN;
    struct Regs { uint32_t r[2][4]; };
    const uint8_t* gb[2];                         // row 0 of b at the block's columns (clamped to the last quad of a row)
    uint32_t k4[2], lds_e[2], k, bp, fill;
    __device__ __forceinline__ BmmBN(const Int8BmmArgs& g, const uint8_t* b, uint32_t col0, uint32_t t) {
        k = g.k; bp = g.e.op; fill = ((uint32_t)g.zb & 0xffu) * 0x01010101u;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t idx = t + (uint32_t)kBlock * h, n4 = idx & 15u;
            k4[h] = (idx >> 4) * 4u;
            gb[h] = b + min(col0 + 4u * n4, bp - 4u);
            lds_e[h] = 4u * n4 * kPitch + k4[h];
        }
    }
    // rows at or past K do not exist: the code zb stands for them
    __device__ __forceinline__ void load(uint32_t kb0, Regs& st) const {
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (uint32_t kk = 0; kk < 4; kk++) {
                const uint32_t row = kb0 * kQ8Block + k4[h] + kk;
                st.r[h][kk] = row < k ? *reinterpret_cast<const uint32_t*>(gb[h] + (size_t)row * bp) : fill;
            }
    }
    // v_perm_b32 D, S0, S1, sel: byte i of D is byte sel[i] of {S0, S1} (0 .. 3 of S1, 4 .. 7 of S0)
    __device__ __forceinline__ void store(uint8_t* stage, const Regs& st) const {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t (&r)[4] = st.r[h];
            const uint32_t t0 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u), t1 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);
            const uint32_t t2 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u), t3 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
            uint8_t* at = stage + lds_e[h];                                      // column 4 n4 + j: the bytes k4 .. k4 + 3 of its row
            *reinterpret_cast<uint32_t*>(at) = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
            *reinterpret_cast<uint32_t*>(at + kPitch) = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
            *reinterpret_cast<uint32_t*>(at + 2u * kPitch) = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
            *reinterpret_cast<uint32_t*>(at + 3u * kPitch) = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
        }
    }
};

// the sum of a fragment's 8 bytes, added to s
__device__ __forceinline__ int bmm_sum8(long f, int s) {
    s = __builtin_amdgcn_sdot4((int)(uint32_t)f, 0x01010101, s, false);
    return __builtin_amdgcn_sdot4((int)(uint32_t)((uint64_t)f >> 32), 0x01010101, s, false);
}

// q8_chunk with the sums: sa[i] the lane's share of the sum of A row wm + 16 i + r (ZB), sb[j] of B column wn + 16 j + r (ZA)
template <bool TAIL, bool ZA, bool ZB, uint32_t PB>
__device__ __forceinline__ void bmm_chunk(const uint8_t* buf, uint32_t wm, uint32_t wn, uint32_t r, uint32_t grp, uint32_t live,
                                          v4i (&acc)[kQ8WaveTiles][kQ8WaveTiles], int (&sa)[kQ8WaveTiles], int (&sb)[kQ8WaveTiles]) {
    constexpr int T = kQ8WaveTiles;
    const uint8_t* la = buf + (wm + r) * kQ8Pitch + grp * 8u;
    const uint8_t* lb = buf + kQ8TileBytes<2> + (wn + r) * PB + grp * 8u;
#pragma unroll
    for (uint32_t b = 0; b < kQ8ChunkBlocks; b++) {
        if (TAIL && b >= live) break;                                            // wave-uniform
        long a[T], bb[T];
#pragma unroll
        for (int i = 0; i < T; i++) {
            a[i] = *reinterpret_cast<const long*>(la + i * kQ8Tile * kQ8Pitch + b * kQ8Block);
            bb[i] = *reinterpret_cast<const long*>(lb + i * kQ8Tile * PB + b * kQ8Block);
        }
#pragma unroll
        for (int i = 0; i < T; i++) {
            if (ZB) sa[i] = bmm_sum8(a[i], sa[i]);
            if (ZA) sb[i] = bmm_sum8(bb[i], sb[i]);
        }
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
}

template <bool ZA, bool ZB, bool TB>
__global__ __launch_bounds__(kBlock) void q8_bmm_kernel(const Int8BmmArgs g) {
    using BMap = typename std::conditional<TB, BmmBK, BmmBN>::type;
    constexpr int T = kQ8WaveTiles;
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kQ8BufBytes<Q8B8>];
    const uint32_t batch = fdiv(blockIdx.x, g.tiles), tile = blockIdx.x - batch * g.tiles.d;
    const uint32_t tm = fdiv(tile, g.e.tiles_n), tn = tile - tm * g.e.tiles_n.d;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t row0 = tm * kQ8Edge, col0 = tn * kQ8Edge;
    const uint32_t wm = (wave >> 1) * (T * kQ8Tile), wn = (wave & 1u) * (T * kQ8Tile);
    Int8Tail e = g.e;                                                            // this batch's outputs
    const size_t out = (size_t)batch * e.m;
    if (e.residual != nullptr) e.residual += out * e.n;
    if (e.c != nullptr) e.c += out * e.n;
    if (e.q != nullptr) e.q += out * e.op;
    const bool busy = row0 + wm < e.m && col0 + wn < e.n;                        // wave-uniform: a wave past the edge only stages

    v4i acc[T][T];
    int sa[T] = {0, 0}, sb[T] = {0, 0};
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4i{0, 0, 0, 0};

    const uint32_t nb = g.nb;
    if (nb > 0u) {                                                               // nb == 0: the operands may be null
        // A: segment t & 7 (16 bytes) of rows t >> 3 and 32 + (t >> 3), as int8_gemm.hpp stages it
        const uint8_t* a = g.a + (size_t)batch * g.a_batch;
        const uint32_t seg = t & 7u;
        const uint8_t* ga[2]; uint32_t lds_e[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = (t >> 3) + kQ8Slab * h;
            ga[h] = a + min(row0 + row, e.m - 1u) * ((size_t)nb * kQ8Block) + 16u * (seg & 1u);
            lds_e[h] = row * kQ8Pitch + seg * 16u;
        }
        const BMap bmap(g, g.b + (size_t)batch * g.b_batch, col0, t);
        v4u ra[2]; typename BMap::Regs rb;
        auto load = [&](uint32_t kb0) {                                          // a block at or past nb: clamped, not multiplied
            const size_t off = (size_t)min(kb0 + (seg >> 1), nb - 1u) * kQ8Block;
            ra[0] = *reinterpret_cast<const v4u*>(ga[0] + off); ra[1] = *reinterpret_cast<const v4u*>(ga[1] + off);
            bmap.load(kb0, rb);
        };
        auto store = [&](uint8_t* buf) {
            *reinterpret_cast<v4u*>(buf + lds_e[0]) = ra[0]; *reinterpret_cast<v4u*>(buf + lds_e[1]) = ra[1];
            bmap.store(buf + kQ8TileBytes<2>, rb);
        };
        const uint32_t chunks = (nb + kQ8ChunkBlocks - 1u) / kQ8ChunkBlocks, rest = nb % kQ8ChunkBlocks;
        load(0u);
        store(stage[0]);
        __syncthreads();
        for (uint32_t c = 0; c < chunks; c++) {
            const bool more = c + 1u < chunks;
            if (more) load((c + 1u) * kQ8ChunkBlocks);
            if (busy) {
                if (!more && rest) bmm_chunk<true, ZA, ZB, BMap::kPitch>(stage[c & 1u], wm, wn, r, grp, rest, acc, sa, sb);
                else bmm_chunk<false, ZA, ZB, BMap::kPitch>(stage[c & 1u], wm, wn, r, grp, kQ8ChunkBlocks, acc, sa, sb);
            }
            if (more) store(stage[(c + 1u) & 1u]);                               // last read before the barrier that ended chunk c - 1
            __syncthreads();
        }
    }
    __syncthreads();
    if (!busy) return;

    // I = sum a b - za colsum_b - zb rowsum_a + Kp za zb, modulo 2^32
    if (ZA || ZB) {
        const uint32_t za = (uint32_t)e.zx, zb = (uint32_t)g.zb;
        const uint32_t base = nb * kQ8Block * za * zb;
        uint32_t colc[T], rowc[T][4];
#pragma unroll
        for (int i = 0; i < T; i++) {
            int s = sb[i], u = sa[i];
            if (ZA) { s += __shfl_xor(s, 16, kWave); s += __shfl_xor(s, 32, kWave); }
            if (ZB) { u += __shfl_xor(u, 16, kWave); u += __shfl_xor(u, 32, kWave); }
            colc[i] = base - za * (uint32_t)s;                                   // column wn + 16 i + r: this lane's
#pragma unroll
            for (int q = 0; q < 4; q++) rowc[i][q] = ZB ? zb * (uint32_t)__shfl(u, (int)(grp * 4u) + q, kWave) : 0u;   // row wm + 16 i + 4 grp + q
        }
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[i][j][q] = (int)((uint32_t)acc[i][j][q] + colc[j] - rowc[i][q]);
    }
    q8_epilogue<true>(acc, e, row0 + wm, col0 + wn, lane, &stage[0][0] + wave * kQ8CodeBytes);
}

// the body of ppqhip_int8_bmm
inline int q8_bmm(const int8_t* a, const int8_t* b, int transpose_b, int za, int zb, const Int8TailHost& h, int64_t batch, int64_t m, int64_t n,
                  int64_t k, void* stream) {
    const char* what = "int8_bmm";
    if (int st = check_int8_tail(what, "c", h)) return st;
    if (za < -128 || za > 127 || zb < -128 || zb > 127) { set_error("%s: za %d / zb %d is not an int8 zero point", what, za, zb); return PPQHIP_ERR_INVALID_VALUE; }
    if (batch < 0 || m < 0 || n < 0 || k < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (batch > kQ8Max || m > kQ8Max || n > kQ8Max || k > kQ8Max || bounded_product(batch, m) < 0 || bounded_product(batch, n) < 0) {
        set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    const int64_t nb = (k + kQ8Block - 1) / kQ8Block, kp = nb * kQ8Block, op = (n + kQ8Block - 1) / kQ8Block * kQ8Block;
    if (kp > kBmmMaxK) { set_error("%s: a padded reduction length of %lld: more than 32768 could overflow int32", what, (long long)kp); return PPQHIP_ERR_INVALID_VALUE; }
    if (batch == 0 || m == 0 || n == 0) return PPQHIP_OK;
    if (nb > 0 && (a == nullptr || b == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (nb > 0 && (!aligned16(a) || !aligned16(b))) { set_error("%s: operands, c and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t a_batch = m * kp, b_batch = transpose_b ? n * kp : k * op;
    std::vector<Span> ins;
    if (nb > 0) { ins.push_back(span_of(a, batch * a_batch)); ins.push_back(span_of(b, batch * b_batch)); }
    const double bytes = (double)batch * ((double)a_batch + (double)b_batch);      // booked: both operands once, mul, the residual and every output

    Int8BmmArgs g;
    g.a = reinterpret_cast<const uint8_t*>(a); g.b = reinterpret_cast<const uint8_t*>(b);
    g.nb = (uint32_t)nb; g.k = (uint32_t)k; g.zb = zb; g.a_batch = (size_t)a_batch; g.b_batch = (size_t)b_batch;
    const int64_t tiles_m = (m + kQ8Edge - 1) / kQ8Edge, tiles_n = (n + kQ8Edge - 1) / kQ8Edge;
    if (bounded_product(tiles_m, tiles_n) < 0 || bounded_product(tiles_m * tiles_n, batch) < 0) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    g.e.tiles_n = make_fastdiv((uint32_t)tiles_n); g.tiles = make_fastdiv((uint32_t)(tiles_m * tiles_n));
    const int sel = (za != 0 ? 4 : 0) | (zb != 0 ? 2 : 0) | (transpose_b ? 1 : 0);
    // launch_q8 sees the batches as rows of one [batch m, n] result: that is what the residual and the outputs span
    return launch_q8(what, "c", K_INT8_BMM, h, batch * m, n, kp, batch * tiles_m * tiles_n, ins, bytes, stream, g.e, [&g, m, za, sel](uint32_t blocks, hipStream_t s) {
        g.e.m = (uint32_t)m; g.e.zx = za;
        const dim3 grid(blocks), block(kBlock);
        switch (sel) {
            case 0: hipLaunchKernelGGL((q8_bmm_kernel<false, false, false>), grid, block, 0, s, g); break;
            case 1: hipLaunchKernelGGL((q8_bmm_kernel<false, false, true>), grid, block, 0, s, g); break;
            case 2: hipLaunchKernelGGL((q8_bmm_kernel<false, true, false>), grid, block, 0, s, g); break;
            case 3: hipLaunchKernelGGL((q8_bmm_kernel<false, true, true>), grid, block, 0, s, g); break;
            case 4: hipLaunchKernelGGL((q8_bmm_kernel<true, false, false>), grid, block, 0, s, g); break;
            case 5: hipLaunchKernelGGL((q8_bmm_kernel<true, false, true>), grid, block, 0, s, g); break;
            case 6: hipLaunchKernelGGL((q8_bmm_kernel<true, true, false>), grid, block, 0, s, g); break;
            default: hipLaunchKernelGGL((q8_bmm_kernel<true, true, true>), grid, block, 0, s, g); break;
        }
    }, 1);
}

#endif  // __HIPCC__

}  // namespace ppqhip
