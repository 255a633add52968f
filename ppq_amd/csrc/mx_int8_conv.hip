// mx_int8_conv.hip -- Y[M, O] (float32) = conv2d(x, w) (+ bias[O]) on two MXINT8 operands, through the int8 MFMA of gfx950
// (v_mfma_i32_16x16x32_i8): an implicit GEMM.  The contract is DESIGN.md section 9.20 and tests/mx_int8_conv_reference.py.
//
// Both operands are read exactly as mx_pack.hip leaves an MXINT8 4-D tensor packed along axis 1: the
// activation x [N, C, H, W] as elements [N, H, W, nbc * 32] and scales [N, H, W, nbc], the weight w [O, C, kh, kw] as elements
// [O, kh, kw, nbc * 32] and scales [O, kh, kw, nbc], nbc = ceil(C / 32).  The weight IS the B operand of mx_int8_gemm.hip, [O, nb']
// with nb' = kh * kw * nbc blocks per row ordered (ky, kx, channel block), and is staged by the same addressing.  Row m of the A
// operand is output pixel (n, oy, ox), M = N * OH * OW rows in that order; its block kb is channel block kb % nbc of input pixel
//   (iy, ix) = (oy * sh - ph + ky * dh, ox * sw - pw + kx * dw),   (ky, kx) = divmod(kb / nbc, kw),
// found in x at block ((n * H + iy) * W + ix) * nbc + kb % nbc.  No im2col buffer exists: A is gathered into the LDS stage.
//
// The frame is that of mx_int8_gemm.hip and lies in mx_int8_tile.hpp: 256 threads own a 64 x 64 tile of Y, the K loop runs in chunks
// of 4 blocks through a double-buffered LDS stage with a pitch of 144 bytes, one barrier per chunk; per block and tile one MFMA from a
// zero accumulator, v_cvt_f32_i32, v_ldexp_f32 by sx + sw - 266 and a float32 add: the bits of mx_int8_gemm.hip on the gathered rows.
// What is here is the A side of the staging.  Before the K loop a thread decodes, with two FastDiv divisions each, the output pixels
// of its two element rows (t >> 3 and 32 + (t >> 3)) and -- threads 0 .. 127 -- of its scale row into (n * H, oy * sh - ph,
// ox * sw - pw).  Per chunk it decodes the tap and channel block of the block its 16-byte segment lies in, kb0 + (seg >> 1), once: the
// same for both rows, which then differ in one computed address each.  Its two scale codes, of blocks kb0 + 2 pair and + 1, are decoded
// one by one: with nbc odd they belong to two taps.  Pixel rows are 32 nbc bytes apart: every 16-byte load is aligned.
// Padding: a tap outside the image, and a block at or past nb', issues NO global load; the thread stores a zero v4u and scale code 127
// and never flags it.  The block's term is +0: P is the integer 0, (float)0 is +0 and ldexp keeps +0 under any finite exponent.
// acc + (+0) leaves every acc but -0 as it is, and the chain never holds -0: it starts at +0, and x + y is -0 only for x = y = -0,
// while a term is -0 for no P.  So multiplying such a block (as here) and skipping it give the same bits.
// Rows past M or O are clamped on load and not stored; the tail chunk multiplies only its live blocks.
// NaN: a scale code 0xFF read from INSIDE the image, or from w, flags the row (column); flagged outputs are written as 0x7fc00000.
// ppqhip_mx_int8_conv2d_fused runs the same K loop with the fused epilogue (fused_tiles in mx_int8_tile.hpp):
// residual, ReLU and the result packed as MXINT8 along the output channels -- the x of the next launch --, in a second instantiation;
// the plain kernel keeps its code.
#include "common.hpp"
#include "job_table.hpp"
#include "mx_mfma.hpp"
#include "mx_int8_tile.hpp"

namespace ppqhip {
namespace {

struct MxInt8ConvArgs {
    const uint8_t* xe; const uint8_t* xs;         // x: elements [n, h, w, nbc * 32], scales [n, h, w, nbc]
    const uint8_t* we; const uint8_t* ws;         // w: elements [o, nb * 32], scales [o, nb]; nb = kh * kw * nbc (0 when x holds no block at all)
    const float* bias;                            // [o] or null
    float* y;                                     // [m, o]; may be null in a fused launch
    uint32_t m, o, nb, nbc;
    uint32_t h, w, kw;
    int32_t sh, sw, ph, pw, dh, dw;
    FastDiv tiles_n;
    FastDiv ohw, ow;                              // m -> (n, oy, ox)
    FastDiv fnbc, fkw;                            // kb -> (tap, channel block), tap -> (ky, kx)
};

struct ConvRow {                                  // output pixel of one row of A: its image's first input row and the window's corner
    uint32_t img;                                 // n * h
    int32_t iy0, ix0;                             // oy * sh - ph, ox * sw - pw
};

__device__ __forceinline__ ConvRow conv_row(const MxInt8ConvArgs& g, uint32_t row) {
    row = min(row, g.m - 1u);
    const uint32_t n = fdiv(row, g.ohw), rem = row - n * g.ohw.d, oy = fdiv(rem, g.ow), ox = rem - oy * g.ow.d;
    ConvRow r;
    r.img = n * g.h;
    r.iy0 = (int32_t)oy * g.sh - g.ph;
    r.ix0 = (int32_t)ox * g.sw - g.pw;
    return r;
}

struct ConvTap {                                  // block kb of a row of A: the same for every row
    uint32_t cb;                                  // channel block
    int32_t dy, dx;                               // ky * dh, kx * dw
    bool live;                                    // kb < nb
};

template <bool TAIL>
__device__ __forceinline__ ConvTap conv_tap(const MxInt8ConvArgs& g, uint32_t kb) {
    ConvTap t;
    t.live = !TAIL || kb < g.nb;
    if (TAIL) kb = min(kb, g.nb - 1u);
    const uint32_t tap = fdiv(kb, g.fnbc), ky = fdiv(tap, g.fkw);
    t.cb = kb - tap * g.nbc;
    t.dy = (int32_t)ky * g.dh;
    t.dx = (int32_t)(tap - ky * g.kw) * g.dw;
    return t;
}

// the block of x behind tap t of row r; false where the tap is padding or past nb: nothing is to be read then
__device__ __forceinline__ bool conv_block(const MxInt8ConvArgs& g, const ConvRow& r, const ConvTap& t, uint32_t& block) {
    const uint32_t iy = (uint32_t)(r.iy0 + t.dy), ix = (uint32_t)(r.ix0 + t.dx);      // a negative coordinate is a huge one
    const bool in = t.live && iy < g.h && ix < g.w;
    block = ((r.img + iy) * g.w + ix) * g.nbc + t.cb;
    return in;
}

// Where a thread's share of a chunk lies.  In the stage: as in mx_int8_gemm.hip -- element segment t & 7 of rows t >> 3 and
// 32 + (t >> 3) of both operands, the scale codes 2 pair, 2 pair + 1 of row (t & 127) >> 1 of operand t >> 7.  In global memory: B by
// row pointers; A by the decoded output pixels of its rows.
struct ConvStageMap {
    const MxInt8ConvArgs& g;
    ConvRow ra[2], rs;                            // the pixels of the two element rows and (t < 128) of the scale row of A
    const uint8_t* gb[2];                         // B: the rows' elements (rows clamped)
    const uint8_t* gs;                            // B: the row's scale codes (t >= 128)
    uint32_t seg, lds_e[2], lds_s, pair;
    bool a_side;                                  // t < 128: this thread stages scale codes of A (wave-uniform)

    __device__ __forceinline__ void prepare(uint32_t row0, uint32_t col0, uint32_t t) {
        seg = t & 7u; pair = t & 1u; a_side = t < 128u;
        const size_t pitch = (size_t)g.nb * kMxBlock;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = (t >> 3) + 32u * h;
            ra[h] = conv_row(g, row0 + row);
            gb[h] = g.we + min(col0 + row, g.o - 1u) * pitch;
            lds_e[h] = row * kI8Pitch + seg * 16u;
        }
        const uint32_t srow = (t & 127u) >> 1;
        rs = conv_row(g, row0 + srow);
        gs = g.ws + (size_t)min(col0 + srow, g.o - 1u) * g.nb;
        lds_s = 2u * kI8TileBytes + (t >> 7) * kI8ScaleBytes + srow * kGemmStepBlocks + 2u * pair;
    }

    // one gathered 16-byte segment of A: zero where the tap is padding or past nb (no load is issued)
    __device__ __forceinline__ v4u gather(const ConvRow& r, const ConvTap& tap) const {
        uint32_t block;
        if (!conv_block(g, r, tap, block)) return v4u{0u, 0u, 0u, 0u};
        return *reinterpret_cast<const v4u*>(g.xe + (size_t)block * kMxBlock + 16u * (seg & 1u));
    }

    // one gathered scale code of A: 127 where the tap is padding or past nb (no load is issued)
    template <bool TAIL>
    __device__ __forceinline__ uint32_t gather_scale(uint32_t kb) const {
        uint32_t block;
        if (!conv_block(g, rs, conv_tap<TAIL>(g, kb), block)) return 127u;
        return g.xs[block];
    }

    // the loads of the chunk that starts at block kb0; returns whether a live scale code is 0xFF
    template <bool TAIL>
    __device__ __forceinline__ bool load(uint32_t kb0, Staged& st) const {
        const uint32_t eb = kb0 + (seg >> 1);
        const ConvTap tap = conv_tap<TAIL>(g, eb);
        st.a0 = gather(ra[0], tap); st.a1 = gather(ra[1], tap);
        const size_t off = (size_t)(TAIL ? min(eb, g.nb - 1u) : eb) * kMxBlock + 16u * (seg & 1u);
        st.b0 = *reinterpret_cast<const v4u*>(gb[0] + off); st.b1 = *reinterpret_cast<const v4u*>(gb[1] + off);
        const uint32_t s0 = kb0 + 2u * pair, s1 = s0 + 1u;
        uint32_t c0, c1;
        if (a_side) {                                                            // padding and dead blocks give 127: never 0xFF
            c0 = gather_scale<TAIL>(s0); c1 = gather_scale<TAIL>(s1);
            st.s = c0 | (c1 << 8);
            return c0 == 0xffu || c1 == 0xffu;
        }
        c0 = gs[TAIL ? min(s0, g.nb - 1u) : s0]; c1 = gs[TAIL ? min(s1, g.nb - 1u) : s1];
        st.s = c0 | (c1 << 8);
        return (c0 == 0xffu && (!TAIL || s0 < g.nb)) || (c1 == 0xffu && (!TAIL || s1 < g.nb));
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Staged& st) const { store_staged(buf, lds_e, lds_s, st); }
};

// The K loop is the one of mx_int8_gemm_kernel (the maps differ, the order of loads, multiplies, stores and barriers does not), and so
// is F: empty for the plain kernel, one MxFusedOut for the fused one.
template <typename... F>
__global__ __launch_bounds__(kBlock) void mx_int8_conv_kernel(const MxInt8ConvArgs g, const F... f) {
    constexpr bool FUSED = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one MxFusedOut");
    constexpr int T = kGemmWaveTiles;
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kI8BufBytes];
    __shared__ uint32_t nan_flags[2 * kGemmEdge];                                // rows of A, then rows of B (columns of Y)
    const uint32_t tm = fdiv(blockIdx.x, g.tiles_n), tn = blockIdx.x - tm * g.tiles_n.d;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t row0 = tm * kGemmEdge, col0 = tn * kGemmEdge;
    const uint32_t wm = (wave / kGemmWaves) * (T * kGemmTile), wn = (wave % kGemmWaves) * (T * kGemmTile);
    const bool busy = row0 + wm < g.m && col0 + wn < g.o;                        // wave-uniform: a wave past the edge only stages

    v4f acc[T][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    clear_nan_flags(nan_flags, t);

    bool bad = false;
    if (g.nb > 0u) {                                                             // nb == 0: the operands may be null
        ConvStageMap map{g};
        map.prepare(row0, col0, t);
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
        fused_tiles(acc, nan_flags, g.bias, g.y, g.m, g.o, row0, col0, wm, wn, lane, f..., &stage[0][0]);
        return;
    }
    store_tiles(acc, nan_flags, g.bias, g.y, g.m, g.o, row0, col0, wm, wn, r, grp);
}

// a * b when it stays within 2^31 - 1 (both are within it already), -1 otherwise
int64_t bounded_product(int64_t a, int64_t b) {
    const int64_t p = a * b;
    return p > kMxMax ? -1 : p;
}

// both entry points; `fused` is null for ppqhip_mx_int8_conv2d, whose checks, strings and launch are unchanged
int run_int8_conv(const char* what, const uint8_t* x_elements, const uint8_t* x_scales, const uint8_t* w_elements, const uint8_t* w_scales,
                  const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t w, int64_t o, int64_t kh, int64_t kw,
                  int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w, const MxFusedHost* fused,
                  void* stream) {
    MxFusedOut f = {};
    if (fused != nullptr) {
        if (int st = check_int8_fused(what, "y", y, *fused, f)) return st;
    }
    const int64_t sizes[] = {n, c, h, w, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
    for (int64_t v : sizes) {
        if (v < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
        if (v > kMxMax) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    }
    if (kh < 1 || kw < 1) { set_error("%s: kernel size must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (stride_h < 1 || stride_w < 1) { set_error("%s: stride must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (dil_h < 1 || dil_w < 1) { set_error("%s: dilation must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t span_h = h + 2 * pad_h - dil_h * (kh - 1) - 1, span_w = w + 2 * pad_w - dil_w * (kw - 1) - 1;
    if (span_h < 0 || span_w < 0) { set_error("%s: the kernel window does not fit the padded input: no output", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (h + 2 * pad_h > kMxMax || w + 2 * pad_w > kMxMax) { set_error("%s: a padded size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t oh = span_h / stride_h + 1, ow = span_w / stride_w + 1;
    const int64_t nbc = (c + kMxBlock - 1) / kMxBlock;
    int64_t m = bounded_product(n, oh);
    if (m >= 0) m = bounded_product(m, ow);
    int64_t nb = bounded_product(kh, kw);
    if (nb >= 0) nb = bounded_product(nb, nbc);
    int64_t blocks_x = bounded_product(n, h);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, w);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, nbc);
    if (m < 0 || nb < 0 || blocks_x < 0) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (n == 0 || o == 0) return PPQHIP_OK;
    const bool read_x = blocks_x > 0, read_w = read_x && nb > 0;     // an input without a pixel: every tap is padding, nothing is read
    if ((y == nullptr && fused == nullptr) || (read_x && (x_elements == nullptr || x_scales == nullptr)) || (read_w && (w_elements == nullptr || w_scales == nullptr))) {
        set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (!aligned16(y) || (read_x && !aligned16(x_elements)) || (read_w && !aligned16(w_elements))) {
        set_error("%s: elements and y must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    std::vector<Span> ins, outs;
    if (read_x) { ins.push_back(span_of(x_elements, blocks_x * kMxBlock)); ins.push_back(span_of(x_scales, blocks_x)); }
    if (read_w) { ins.push_back(span_of(w_elements, o * nb * kMxBlock)); ins.push_back(span_of(w_scales, o * nb)); }
    if (bias != nullptr) ins.push_back(span_of(bias, o));
    if (y != nullptr) outs.push_back(span_of(y, m * o));
    // booked: packed x once (a pixel is read by up to kh kw windows, from cache), packed w and 4 m o bytes of y; the launch does
    // 2 m o nb 32 integer operations
    double bytes = ((double)blocks_x + (double)o * (double)nb) * (double)(kMxBlock + 1);
    if (y != nullptr) bytes += 4.0 * (double)m * (double)o;

    MxInt8ConvArgs g;
    g.xe = x_elements; g.xs = x_scales; g.we = w_elements; g.ws = w_scales; g.bias = bias; g.y = y;
    g.m = (uint32_t)m; g.o = (uint32_t)o; g.nbc = (uint32_t)nbc;
    g.nb = read_w ? (uint32_t)nb : 0u;
    g.h = (uint32_t)h; g.w = (uint32_t)w; g.kw = (uint32_t)kw;
    g.sh = (int32_t)stride_h; g.sw = (int32_t)stride_w; g.ph = (int32_t)pad_h; g.pw = (int32_t)pad_w;
    g.dh = (int32_t)dil_h; g.dw = (int32_t)dil_w;
    g.ohw = make_fastdiv((uint32_t)(oh * ow)); g.ow = make_fastdiv((uint32_t)ow);
    g.fnbc = make_fastdiv((uint32_t)std::max<int64_t>(nbc, 1)); g.fkw = make_fastdiv((uint32_t)kw);
    return launch_int8_tiles(what, K_MX_INT8_CONV, K_MX_INT8_CONV_FUSED, fused, f, m, o, ins, outs, bytes, stream, g.tiles_n,
                             [&g](uint32_t blocks, hipStream_t s, const auto&... fo) {
        hipLaunchKernelGGL((mx_int8_conv_kernel<std::decay_t<decltype(fo)>...>), dim3(blocks), dim3(kBlock), 0, s, g, fo...);
    });
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_int8_conv2d(const uint8_t* x_elements, const uint8_t* x_scales, const uint8_t* w_elements, const uint8_t* w_scales,
                                     const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t w, int64_t o, int64_t kh,
                                     int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h,
                                     int64_t dil_w, void* stream) {
    return run_int8_conv("mx_int8_conv2d", x_elements, x_scales, w_elements, w_scales, bias, y, n, c, h, w, o, kh, kw, stride_h, stride_w,
                         pad_h, pad_w, dil_h, dil_w, nullptr, stream);
}

extern "C" int ppqhip_mx_int8_conv2d_fused(const uint8_t* x_elements, const uint8_t* x_scales, const uint8_t* w_elements,
                                           const uint8_t* w_scales, const float* bias, const float* residual, int relu, float* y,
                                           uint8_t* out_elements, uint8_t* out_scales, int64_t n, int64_t c, int64_t h, int64_t w,
                                           int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                           int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream) {
    const MxFusedHost fused = {residual, relu, out_elements, out_scales, PPQHIP_MXINT8};
    return run_int8_conv("mx_int8_conv2d_fused", x_elements, x_scales, w_elements, w_scales, bias, y, n, c, h, w, o, kh, kw, stride_h,
                         stride_w, pad_h, pad_w, dil_h, dil_w, &fused, stream);
}
