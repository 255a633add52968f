// int8_tile.hpp -- what the linear INT8 kernels on the int8 MFMA of gfx950 (v_mfma_i32_16x16x32_i8) share: the GEMM (int8_gemm.hpp)
// and the convolution (int8_conv.hpp), each with an int8 weight (int8_gemm.hip, int8_conv.hip) or a packed int4 one (int4_gemm.hip,
// int4_conv.hip).  The contract is DESIGN.md sections 9.22 / 9.23 and tests/int8_reference.py.  The frame is generic over the B
// operand alone -- how a weight is staged and how a lane reads its fragment (the codecs Q8B8 / Q8B4 below); what follows describes it
// with int8 weights.
//
// Linear INT8 has ONE scale per tensor or channel, so -- unlike the MXINT8 kernels of mx_int8_tile.hpp, which start every MFMA from a
// zero accumulator and pay a conversion, an ldexp and a float add per output and block of 32 -- the int32 accumulator stays in the
// MFMA's C operand for the whole of K: inside a chunk there is nothing but LDS reads and MFMAs.  Everything else happens once per
// output, in the epilogue: the conversion, the one float32 multiply by sx * sw[o], bias, residual, ReLU and the re-quantisation.
//
// Shape.  A workgroup of 256 threads owns a 64 x 64 tile of the result, each of its 2 x 2 waves a 2 x 2 group of 16 x 16 MFMA tiles
// (16 accumulator registers per lane).  Per K-chunk of 128 bytes (4 instructions deep) the workgroup stages 64 rows of each operand
// with 16-byte global loads, two per thread and operand, into a double-buffered LDS stage: the next chunk's loads are issued into
// registers before the current chunk's MFMAs and stored to the other buffer after them; one barrier per chunk.  There is no scale
// stage and there are no NaN flags: integers have neither.  A staged row has a pitch of 144 bytes = 36 dwords, so that the 8-byte
// fragment reads of the 16 rows of a K-group start 36 dwords apart -- in 16 different groups of 4 banks -- where a pitch of 128 would
// put all 16 on one bank; 144 keeps the 16-byte stores aligned (the argument of mx_int8_gemm.hip, whose pitch this is).
//
// Fragments, as established on the device: lane l holds row (A) resp. column (B) l & 15 and the 8 bytes 8 (l >> 4) .. + 7 of the
// 32-byte block; C / D: lane l holds column l & 15, rows 4 (l >> 4) + reg.
//
// Zero point.  It costs nothing in the K loop: the accumulators of column o START at -zx * sums[o], sums[o] = sum_k w[o, k] made when
// the weight was packed, and the MFMAs add sum_k w x: together sum_k w (x - zx).  With |w| <= 128, |x - zx| <= 255 and Kp < 65536
// (the host refuses more) no partial sum leaves int32.
//
// The int8 codes of a wave -- 32 rows x 32 columns, one byte each -- are gathered through LDS so that they leave as 16-byte row
// stores.  No LDS is declared for that: wave w takes bytes [1024 w, + 1024) of the operand stage, which is dead by then.  The stage's
// last readers are the MFMA reads of the last chunk, and every wave passes the barrier that ends that chunk, and the kernel's final
// barrier after it, before any wave reaches its epilogue: no fragment read can follow a code write.  From there on a wave touches its
// own slice only, so the waves that returned at the edge are not waited for (the pattern of fused_tiles in mx_int8_tile.hpp).
//
// The frame has ONE shape parameter, NA: the 16-byte segments of A a thread stages per chunk, of its rows t >> 3 + 32 h, h < NA.  The
// four waves are NA along M and 4 / NA along N: NA = 2 is the 64 x 64 tile described above (every dense kernel); NA = 4 is 128 rows x
// 32 columns, four waves stacked along M over ONE 32-row B stage -- the grouped convolution of int8_gconv.hpp, whose 32-column slices
// each need input channels of their own, so that two wave columns could not share an A stage.
#pragma once
#include "common.hpp"
#include "job_table.hpp"
#include "to_int.hpp"

namespace ppqhip {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int kQ8Tile = 16;                                                      // one MFMA's rows and columns
constexpr int kQ8WaveTiles = 2;                                                  // a wave owns 2 x 2 MFMA tiles ...
constexpr int kQ8Waves = 2;                                                      // ... and a workgroup 2 x 2 waves
constexpr uint32_t kQ8Edge = kQ8Tile * kQ8WaveTiles * kQ8Waves;                  // 64: rows and columns of the result per workgroup
constexpr uint32_t kQ8Block = 32;                                                // bytes of K per instruction; rows are padded to it
constexpr uint32_t kQ8ChunkBlocks = 4;                                           // instructions of one row per chunk
constexpr uint32_t kQ8Pitch = kQ8ChunkBlocks * kQ8Block + 16u;                   // 144: a staged row of 128 bytes, padded
constexpr uint32_t kQ8Slab = 32;                                                 // rows between a thread's segments: 256 threads / 8 segments a row
template <int NA> constexpr uint32_t kQ8Rows = kQ8Slab * NA;                     // rows of the result per workgroup: NA waves of 32 ...
template <int NA> constexpr uint32_t kQ8Cols = kQ8Slab * (kQ8Waves * kQ8Waves / NA);         // ... and its columns: 32 per wave along N
template <int NA> constexpr uint32_t kQ8TileBytes = kQ8Rows<NA> * kQ8Pitch;      // the staged rows of A
constexpr uint32_t kQ4BlockBytes = kQ8Block / 2u;                                // an int4 B row: 16 bytes per block of 32 k
constexpr uint32_t kQ4Pitch = kQ8ChunkBlocks * kQ4BlockBytes + 16u;              // 80: a staged int4 row of 64 bytes, padded
constexpr uint32_t kQ8CodeBytes = (kQ8WaveTiles * kQ8Tile) * (kQ8WaveTiles * kQ8Tile);       // a wave's 32 rows of 32 codes
constexpr int64_t kQ8MaxK = 65536;                                               // padded reduction lengths from here on are refused
constexpr int64_t kQ8Max = 0x7fffffffLL;
static_assert(kQ8Waves * kQ8Waves * kWave == kBlock, "four waves per workgroup");
static_assert(kQ8Rows<2> == kQ8Edge && kQ8Cols<2> == kQ8Edge && kQ8Rows<4> == 128u && kQ8Cols<4> == 32u, "the two shapes of the frame");
static_assert(kQ8Pitch % 16u == 0 && kQ4Pitch % 16u == 0, "16-byte stores into the stage");
static_assert(kQ8Edge * kQ8ChunkBlocks * kQ8Block == 2u * 16u * (uint32_t)kBlock, "two 16-byte loads per thread and int8 operand");
static_assert(kQ8Edge * kQ8ChunkBlocks * kQ4BlockBytes == 16u * (uint32_t)kBlock, "one 16-byte load per thread of an int4 B");
static_assert(kQ8WaveTiles * kQ8Tile == (int)kQ8Block, "a wave's columns are one 32-byte group of a code row");

// What both kernels take beyond their operands: the column data, the tail and the outputs of an [m, n] result.
struct Int8Tail {
    const int32_t* sums;                          // [n]: sum_k w[o, k]; null when zx == 0
    const float* mul;                             // [n]: sx * sw[o]
    const float* bias;                            // [n] or null
    const float* residual;                        // [m, n] or null
    float* c;                                     // [m, n] or null
    int8_t* q;                                    // [m, op] or null
    uint32_t m, n, op;                            // op = ceil32(n)
    int32_t zx;                                   // the activation's zero point, -128 .. 127
    uint32_t relu;
    float sy, zy, qmin, qmax;                     // the output grid, in the stored (int8) domain
    int32_t rounding, q_nan;                      // q_nan: the code of a NaN
    FastDiv tiles_n;
};

#if defined(__HIPCC__)

// ---- the B operand: how a weight lies in global memory, how a chunk of it is staged and how a lane reads its fragment ---------------
// A codec B has: kBlockBytes, the bytes of a row per block of 32 k; kPitch, the pitch of a staged row; kShift, log2 of what its
// fragments are scaled by (the accumulators then hold I << kShift); kMinBlocks, the workgroups per CU its kernels are bounded to;
// kRows, the rows it stages (the workgroup's columns of the result);
// Regs, what a thread carries of a chunk; Map, where a thread's share lies -- Map(b, nb, n, col0, t) for the rows col0 .. col0 + kRows - 1 (clamped to n - 1) of b [n, nb * kBlockBytes], load<TAIL>(kb0, regs)
// as in q8_k_loop, store(stage, regs) into the B stage --; frag(row, b, grp): the 8 bytes 8 grp .. + 7 of block b of a staged row.

// int8 codes as they are: segment t & 7 (16 bytes; block (t & 7) >> 1 of the chunk) of rows t >> 3 + 32 h, h < NB: 64 rows (Q8B8, the
// dense kernels) or 32 (the grouped convolution)
template <int NB>
struct Q8B8Rows {
    static constexpr uint32_t kBlockBytes = kQ8Block, kPitch = kQ8Pitch, kRows = kQ8Slab * NB;
    static constexpr int kShift = 0, kMinBlocks = 1;
    struct Regs { v4u b[NB]; };
    struct Map {
        const uint8_t* gb[NB]; uint32_t seg, lds_e[NB], nb;
        __device__ __forceinline__ Map(const uint8_t* b, uint32_t nblocks, uint32_t n, uint32_t col0, uint32_t t) {
            nb = nblocks; seg = t & 7u;
#pragma unroll
            for (int h = 0; h < NB; h++) {
                const uint32_t row = (t >> 3) + kQ8Slab * h;
                gb[h] = b + min(col0 + row, n - 1u) * ((size_t)nb * kBlockBytes);
                lds_e[h] = row * kPitch + seg * 16u;
            }
        }
        template <bool TAIL>
        __device__ __forceinline__ void load(uint32_t kb0, Regs& st) const {
            const uint32_t eb = kb0 + (seg >> 1);
            const size_t off = (size_t)(TAIL ? min(eb, nb - 1u) : eb) * kBlockBytes + 16u * (seg & 1u);
#pragma unroll
            for (int h = 0; h < NB; h++) st.b[h] = *reinterpret_cast<const v4u*>(gb[h] + off);
        }
        __device__ __forceinline__ void store(uint8_t* stage, const Regs& st) const {
#pragma unroll
            for (int h = 0; h < NB; h++) *reinterpret_cast<v4u*>(stage + lds_e[h]) = st.b[h];
        }
    };
    static __device__ __forceinline__ long frag(const uint8_t* row, uint32_t b, uint32_t grp) {
        return *reinterpret_cast<const long*>(row + b * kBlockBytes + grp * 8u);
    }
};
using Q8B8 = Q8B8Rows<2>;

// int4 codes, two per byte: of every 8 consecutive k (group g) byte 4 g + j holds code 8 g + j in bits 0 .. 3
// and code 8 g + 4 + j in bits 4 .. 7, two's complement.  A chunk of 64 rows is 4096 bytes: ONE 16-byte load per thread, block t & 3 of
// row t >> 2.  A lane's fragment is one dword p, the one of group 4 b + grp: a nibble moved to the top of its byte is the int8 value
// 16 w, sign included, so {(p << 4) & 0xf0f0f0f0, p & 0xf0f0f0f0} are the bytes 8 grp .. + 7 of the block, times 16, in A's byte order:
// three VALU operations, no sign extension, no permutation of A.  The accumulators hold 16 I; |16 w| <= 128 is the bound of Q8B8.
// Pitch 80 bytes = 20 dwords: 20 r mod 64, r = 0 .. 15, are the 16 multiples of 4 below 64, each once, so the dwords 20 r + 4 b + grp of
// the 64 lanes of a fragment read lie in 64 different banks; 80 keeps the 16-byte stores aligned.
struct Q8B4 {
    static constexpr uint32_t kBlockBytes = kQ4BlockBytes, kPitch = kQ4Pitch, kRows = kQ8Edge;
    static constexpr int kShift = 4, kMinBlocks = 4;          // without the bound the allocator takes 132 registers: 3 workgroups a CU, not Q8B8's 4
    struct Regs { v4u b; };
    struct Map {
        const uint8_t* gb; uint32_t seg, lds_e, nb;
        __device__ __forceinline__ Map(const uint8_t* b, uint32_t nblocks, uint32_t n, uint32_t col0, uint32_t t) {
            nb = nblocks; seg = t & 3u;
            gb = b + min(col0 + (t >> 2), n - 1u) * ((size_t)nb * kBlockBytes);
            lds_e = (t >> 2) * kPitch + seg * 16u;
        }
        template <bool TAIL>
        __device__ __forceinline__ void load(uint32_t kb0, Regs& st) const {
            const uint32_t eb = kb0 + seg;
            st.b = *reinterpret_cast<const v4u*>(gb + (size_t)(TAIL ? min(eb, nb - 1u) : eb) * kBlockBytes);
        }
        __device__ __forceinline__ void store(uint8_t* stage, const Regs& st) const { *reinterpret_cast<v4u*>(stage + lds_e) = st.b; }
    };
    static __device__ __forceinline__ long frag(const uint8_t* row, uint32_t b, uint32_t grp) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(row + b * kBlockBytes + grp * 4u);
        const uint32_t lo = (p << 4) & 0xf0f0f0f0u, hi = p & 0xf0f0f0f0u;
        return (long)(((uint64_t)hi << 32) | lo);
    }
};

// one buffer of the double-buffered stage: the 32 NA rows of A at pitch 144, then the codec's rows of B at its pitch
template <typename B, int NA = 2> constexpr uint32_t kQ8BufBytes = kQ8TileBytes<NA> + B::kRows * B::kPitch;
static_assert(kQ8Waves * kQ8Waves * kQ8CodeBytes <= kQ8BufBytes<Q8B8> && kQ8Waves * kQ8Waves * kQ8CodeBytes <= kQ8BufBytes<Q8B4> &&
              kQ8Waves * kQ8Waves * kQ8CodeBytes <= kQ8BufBytes<Q8B8Rows<1>, 4>, "the four waves' code stages fit the first operand buffer");

// what a thread carries from global memory to LDS for one chunk: of A its segment t & 7 (16 bytes) of rows t >> 3 + 32 h, h < NA
template <typename B, int NA = 2>
struct Q8Staged {
    v4u a[NA];
    typename B::Regs b;
};

// A into its stage at the thread's NA places, B through its map
template <typename B, int NA>
__device__ __forceinline__ void q8_store_staged(uint8_t* buf, const uint32_t (&lds_e)[NA], const typename B::Map& bmap, const Q8Staged<B, NA>& st) {
#pragma unroll
    for (int h = 0; h < NA; h++) *reinterpret_cast<v4u*>(buf + lds_e[h]) = st.a[h];
    bmap.store(buf + kQ8TileBytes<NA>, st.b);
}

// The wave's 2 x 2 tiles over the `live` (1 .. 4; 4 unless TAIL) blocks of the chunk staged in buf: per block four fragment reads
// from LDS (8 bytes of A, B as its codec reads it) and four MFMAs, each chained through its accumulator.
template <bool TAIL, typename B, int NA>
__device__ __forceinline__ void q8_chunk(const uint8_t* buf, uint32_t wm, uint32_t wn, uint32_t r, uint32_t grp, uint32_t live,
                                         v4i (&acc)[kQ8WaveTiles][kQ8WaveTiles]) {
    constexpr int T = kQ8WaveTiles;
    const uint8_t* la = buf + (wm + r) * kQ8Pitch + grp * 8u;
    const uint8_t* lb = buf + kQ8TileBytes<NA> + (wn + r) * B::kPitch;
#pragma unroll
    for (uint32_t b = 0; b < kQ8ChunkBlocks; b++) {
        if (TAIL && b >= live) break;                                            // wave-uniform
        long a[T], bb[T];
#pragma unroll
        for (int i = 0; i < T; i++) {
            a[i] = *reinterpret_cast<const long*>(la + i * kQ8Tile * kQ8Pitch + b * kQ8Block);
            bb[i] = B::frag(lb + i * kQ8Tile * B::kPitch, b, grp);
        }
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
}

// The K loop of both kernels over nb >= 1 blocks of 32 bytes.  A Map knows where a thread's share of a chunk lies: load<TAIL>(kb0, st)
// issues the global loads of the chunk that starts at block kb0 (TAIL: the chunk holds fewer than 4 live blocks; a dead one is not
// multiplied and its address is clamped), store(buf, st) puts them into the stage.  A wave past the edge (!busy) only stages.
template <typename B, int NA, typename Map>
__device__ __forceinline__ void q8_k_loop(const Map& map, uint8_t (&stage)[2][kQ8BufBytes<B, NA>], uint32_t nb, bool busy, uint32_t wm, uint32_t wn,
                                          uint32_t r, uint32_t grp, v4i (&acc)[kQ8WaveTiles][kQ8WaveTiles]) {
    const uint32_t chunks = (nb + kQ8ChunkBlocks - 1u) / kQ8ChunkBlocks, rest = nb % kQ8ChunkBlocks;
    Q8Staged<B, NA> st;
    if (chunks == 1u && rest) map.template load<true>(0u, st); else map.template load<false>(0u, st);
    map.store(stage[0], st);
    __syncthreads();
    for (uint32_t c = 0; c < chunks; c++) {
        const bool more = c + 1u < chunks, last_short = c + 2u == chunks && rest != 0u;
        if (more) {
            if (last_short) map.template load<true>((c + 1u) * kQ8ChunkBlocks, st); else map.template load<false>((c + 1u) * kQ8ChunkBlocks, st);
        }
        if (busy) {
            if (!more && rest) q8_chunk<true, B, NA>(stage[c & 1u], wm, wn, r, grp, rest, acc);
            else q8_chunk<false, B, NA>(stage[c & 1u], wm, wn, r, grp, kQ8ChunkBlocks, acc);
        }
        if (more) map.store(stage[(c + 1u) & 1u], st);                           // last read before the barrier that ended chunk c - 1
        __syncthreads();
    }
}

// the accumulators of the wave's columns n0 + 16 j + r before the first MFMA: -zx * sums[column] in the scale of the codec's
// fragments (SHIFT), 0 without sums
template <int SHIFT>
__device__ __forceinline__ void q8_start(const Int8Tail& e, uint32_t n0, uint32_t r, v4i (&acc)[kQ8WaveTiles][kQ8WaveTiles]) {
#pragma unroll
    for (int j = 0; j < kQ8WaveTiles; j++) {
        const uint32_t col = min(n0 + j * kQ8Tile + r, e.n - 1u);
        const int s = e.sums != nullptr ? (int)((0u - (uint32_t)e.zx * (uint32_t)e.sums[col]) << SHIFT) : 0;
#pragma unroll
        for (int i = 0; i < kQ8WaveTiles; i++) acc[i][j] = v4i{s, s, s, s};
    }
}

// One output's float32 chain, shared by every kernel of the family (the depthwise one of int8_dwconv.hip included): t = float32(I)
// (v_cvt_f32_i32, nearest even); v = t * mul; + bias (where the layer has one); + res (where it has a residual); the ReLU.
__device__ __forceinline__ float q8_value(const Int8Tail& e, int i, float mul, float bias, float res) {
    const float t = (float)i;
    float v = t * mul;
    if (e.bias != nullptr) v = v + bias;
    if (e.residual != nullptr) v = v + res;
    if (e.relu) v = v > 0.f ? v : (v != v ? v : 0.f);                             // -0 -> +0; NaN stays
    return v;
}

// ... and its code: to_int_scalar of linear.hip's export kernels on the stored-domain grid, the NaN code for a NaN
__device__ __forceinline__ uint32_t q8_code(const Int8Tail& e, float v) {
    return v != v ? (uint32_t)e.q_nan : (uint32_t)to_int_scalar(v, e.sy, e.zy, e.qmin, e.qmax, e.rounding);
}

// The epilogue of a wave that owns rows m0 .. m0 + 31 and columns n0 .. n0 + 31 (n0 % 32 == 0) of the [m, n] result; acc[i][j][q] is
// row m0 + 16 i + 4 grp + q, column n0 + 16 j + r.  Per output q8_value on mul[col], bias[col] and residual[row, col]; then v as
// float32 and / or its code (q8_code), the zero point in the padding columns n .. op - 1.  `stage` is
// this wave's own kQ8CodeBytes of LDS: the codes of a row sit in 16 lanes x 2 tiles and are gathered through it; then lane l stores
// half l & 1 of row l >> 1.  Only the wave itself touches its stage, so no workgroup barrier is needed.  MUL1: mul is ONE float32 for
// every column (the batched matmul of two per-tensor activations, int8_bmm.hpp).
template <bool MUL1 = false>
__device__ __forceinline__ void q8_epilogue(const v4i (&acc)[kQ8WaveTiles][kQ8WaveTiles], const Int8Tail& e, uint32_t m0, uint32_t n0,
                                            uint32_t lane, uint8_t* stage) {
    constexpr int T = kQ8WaveTiles;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    uint32_t col[T]; bool col_in[T]; float mul[T], b[T];
#pragma unroll
    for (int j = 0; j < T; j++) {
        col[j] = n0 + j * kQ8Tile + r;
        col_in[j] = col[j] < e.n;
        col[j] = min(col[j], e.n - 1u);
        mul[j] = e.mul[MUL1 ? 0u : col[j]];
        b[j] = e.bias != nullptr ? e.bias[col[j]] : 0.f;
    }
    const uint32_t pad_code = (uint32_t)(int)e.zy & 0xffu;
#pragma unroll
    for (int i = 0; i < T; i++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t tr = i * kQ8Tile + grp * 4u + q, row = m0 + tr;
            const size_t at = (size_t)min(row, e.m - 1u) * e.n;                  // rows past m: copies of the last one, not stored
#pragma unroll
            for (int j = 0; j < T; j++) {
                const float v = q8_value(e, acc[i][j][q], mul[j], b[j], e.residual != nullptr ? e.residual[at + col[j]] : 0.f);
                if (e.c != nullptr && row < e.m && col_in[j]) e.c[at + col[j]] = v;
                if (e.q != nullptr) {
                    const uint32_t code = q8_code(e, v);
                    stage[tr * kQ8Block + j * kQ8Tile + r] = (uint8_t)(col_in[j] ? code & 0xffu : pad_code);
                }
            }
        }
    }
    if (e.q == nullptr) return;                                                  // wave-uniform
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                        // the wave's own writes, read by its own lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t lr = lane >> 1, half = lane & 1u, row = m0 + lr;
    const v4u w = *reinterpret_cast<const v4u*>(stage + lr * kQ8Block + half * 16u);
    if (row < e.m) *reinterpret_cast<v4u*>(e.q + (size_t)row * e.op + n0 + half * 16u) = w;      // n0 + 32 <= op: n0 < n and n0 % 32 == 0
}

// what a kernel does around its Map: the wave's place, the accumulators, the K loop, the final barrier and the epilogue.  Where the
// codec's fragments are scaled the accumulators end as I << kShift, a multiple of 2^kShift: the arithmetic shift back is exact.
// Consecutive workgroups walk the column tiles of one row tile: tiles_n is the fast index.
template <typename B, int NA = 2, typename MakeMap>
__device__ __forceinline__ void q8_tile(const Int8Tail& e, uint32_t nb, uint8_t (&stage)[2][kQ8BufBytes<B, NA>], MakeMap&& make_map) {
    constexpr int T = kQ8WaveTiles;
    constexpr uint32_t WN = kQ8Cols<NA> / kQ8Slab;                               // waves along N
    static_assert(B::kRows == kQ8Cols<NA>, "the codec stages the workgroup's columns");
    const uint32_t tm = fdiv(blockIdx.x, e.tiles_n), tn = blockIdx.x - tm * e.tiles_n.d;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t row0 = tm * kQ8Rows<NA>, col0 = tn * kQ8Cols<NA>;
    const uint32_t wm = (wave / WN) * (T * kQ8Tile), wn = (wave % WN) * (T * kQ8Tile);
    const bool busy = row0 + wm < e.m && col0 + wn < e.n;                        // wave-uniform: a wave past the edge only stages

    v4i acc[T][T];
    q8_start<B::kShift>(e, col0 + wn, r, acc);
    if (nb > 0u) {                                                               // nb == 0: the operands may be null
        const auto map = make_map(row0, col0, t);
        q8_k_loop<B, NA>(map, stage, nb, busy, wm, wn, r, grp, acc);
    }
    __syncthreads();
    if (!busy) return;
    if (B::kShift) {
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++) acc[i][j] = acc[i][j] >> B::kShift;
    }
    q8_epilogue(acc, e, row0 + wm, col0 + wn, lane, &stage[0][0] + wave * kQ8CodeBytes);
}

#endif  // __HIPCC__

// ---- the host side of both entry points -------------------------------------------------------------------------------------------------
// the arguments of the tail as an entry point received them
struct Int8TailHost {
    const int32_t* sums; int zx; const float* mul; const float* bias; const float* residual; int relu;
    float* c; int8_t* q; float sy; int zy, qmin, qmax, rounding, q_nan;
};

// What both entry points check about the tail before anything of their own, in this order: an output at all, the zero point and its
// sums, the output grid (only where q is set).
inline int check_int8_tail(const char* what, const char* float_name, const Int8TailHost& h) {
    if (h.c == nullptr && h.q == nullptr) { set_error("%s: no output: %s and q are both null", what, float_name); return PPQHIP_ERR_INVALID_VALUE; }
    if (h.zx < -128 || h.zx > 127) { set_error("%s: zx %d is not an int8 zero point", what, h.zx); return PPQHIP_ERR_INVALID_VALUE; }
    if (h.q != nullptr) {
        if (h.zy < -128 || h.zy > 127 || h.qmin < -128 || h.qmax > 127 || h.qmin > h.qmax || h.q_nan < -128 || h.q_nan > 127) {
            set_error("%s: the output grid (zy %d, qmin %d, qmax %d, q_nan %d) does not lie in int8", what, h.zy, h.qmin, h.qmax, h.q_nan);
            return PPQHIP_ERR_INVALID_VALUE;
        }
        if (h.rounding == ROUND_TO_NEAR_INT || h.rounding < 0 || h.rounding > ROUND_UP) {
            set_error("%s: rounding policy %d has no tensor form (ppq_tensor_round)", what, h.rounding); return PPQHIP_ERR_INVALID_VALUE;
        }
    }
    return PPQHIP_OK;
}

// a * b when it stays within 2^31 - 1 (both are within it already), -1 otherwise
inline int64_t bounded_product(int64_t a, int64_t b) {
    const int64_t p = a * b;
    return p > kQ8Max ? -1 : p;
}

// The rest of an entry point once its sizes are known: m x n the result, kp the padded reduction length (kp == 0 reads no operand),
// `workgroups` what it launches, `ins` the operands' spans and `bytes` what they book.  Checks the tail's pointers, alignment and
// overlaps, fills e (but for tiles_n) and calls launch(workgroups, stream).  mul holds mul_len floats: one per column unless given.
template <typename Launch>
inline int launch_q8(const char* what, const char* float_name, KernelId id, const Int8TailHost& h, int64_t m, int64_t n, int64_t kp,
                     int64_t workgroups, std::vector<Span>& ins, double bytes, void* stream, Int8Tail& e, Launch&& launch, int64_t mul_len = -1) {
    if (mul_len < 0) mul_len = n;
    if (kp >= kQ8MaxK) { set_error("%s: a padded reduction length of %lld: 65536 and more could overflow int32", what, (long long)kp); return PPQHIP_ERR_INVALID_VALUE; }
    if (h.mul == nullptr || (h.zx != 0 && kp > 0 && h.sums == nullptr)) {
        set_error(h.mul == nullptr ? "%s: null pointer" : "%s: sums is required with a zero point other than 0", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (!aligned16(h.c) || !aligned16(h.q)) { set_error("%s: operands, %s and q must be 16-byte aligned", what, float_name); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t op = (n + kQ8Block - 1) / kQ8Block * kQ8Block;
    if (workgroups < 0 || workgroups > kQ8Max) { set_error("%s: too many workgroups in one launch", what); return PPQHIP_ERR_INVALID_VALUE; }
    std::vector<Span> outs;
    ins.push_back(span_of(h.mul, mul_len)); bytes += 4.0 * (double)mul_len;
    if (h.sums != nullptr && kp > 0) ins.push_back(span_of(h.sums, n));
    if (h.bias != nullptr) ins.push_back(span_of(h.bias, n));
    if (h.residual != nullptr) { ins.push_back(span_of(h.residual, m * n)); bytes += 4.0 * (double)m * (double)n; }
    if (h.c != nullptr) { outs.push_back(span_of(h.c, m * n)); bytes += 4.0 * (double)m * (double)n; }
    if (h.q != nullptr) { outs.push_back(span_of(h.q, m * op)); bytes += (double)m * (double)op; }
    if (int st = check_overlap(what, ins, outs)) return st;
    e.sums = kp > 0 ? h.sums : nullptr; e.mul = h.mul; e.bias = h.bias; e.residual = h.residual; e.c = h.c; e.q = h.q;
    e.m = (uint32_t)m; e.n = (uint32_t)n; e.op = (uint32_t)op;
    e.zx = h.zx; e.relu = h.relu ? 1u : 0u;
    e.sy = h.sy; e.zy = (float)h.zy; e.qmin = (float)h.qmin; e.qmax = (float)h.qmax; e.rounding = h.rounding; e.q_nan = h.q_nan;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(id, bytes, s);
    launch((uint32_t)workgroups, s);
    return finish_launch(what);
}

// launch_q8 for the kernels of q8_tile<B, NA>: one workgroup per tile of the result, 64 x 64 (NA = 2) or 128 x 32 (NA = 4)
template <int NA = 2, typename Launch>
inline int launch_q8_tiles(const char* what, const char* float_name, KernelId id, const Int8TailHost& h, int64_t m, int64_t n, int64_t kp,
                           std::vector<Span>& ins, double bytes, void* stream, Int8Tail& e, Launch&& launch) {
    const int64_t tiles_m = (m + kQ8Rows<NA> - 1) / kQ8Rows<NA>, tiles_n = (n + kQ8Cols<NA> - 1) / kQ8Cols<NA>;
    e.tiles_n = make_fastdiv((uint32_t)tiles_n);
    return launch_q8(what, float_name, id, h, m, n, kp, tiles_m * tiles_n, ins, bytes, stream, e, launch);
}

}  // namespace ppqhip
