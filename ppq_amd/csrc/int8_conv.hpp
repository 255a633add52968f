// int8_conv.hpp -- the convolution of the linear INT8 family for either B codec of int8_tile.hpp, on v_mfma_i32_16x16x32_i8 as an
// implicit GEMM with the int32 accumulator chained through the MFMA's C operand over all of K: int8_conv.hip (Q8B8, int8 weights) and
// int4_conv.hip (Q8B4, packed int4 weights) are its two instances.  The contract is DESIGN.md sections 9.22 / 9.23 and
// tests/int8_reference.py; the tile, the K loop, the B codecs and the epilogue are in int8_tile.hpp, shared with int8_gemm.hpp.
//
// Operands: the activation x [N, C, H, W] as int8 codes [N, H, W, Cp], the weight w [O, C, kh, kw] as [O, kh, kw, Cp] in its codec's
// storage (Cp or Cp / 2 bytes a tap), Cp = ceil32(C), the weight's channels C .. Cp - 1 zero.  The weight IS the B operand of
// int8_gemm.hpp, [O, nb blocks] with nb = kh * kw * Cp / 32 blocks per row ordered (ky, kx, channel block).  Row m of the A operand is
// output pixel (n, oy, ox), M = N * OH * OW rows in that order; its block kb is channel block kb % nbc of input pixel
//   (iy, ix) = (oy * sh - ph + ky * dh, ox * sw - pw + kx * dw),   (ky, kx) = divmod(kb / nbc, kw),
// found in x at block ((n * H + iy) * W + ix) * nbc + kb % nbc: the geometry of mx_int8_conv.hip.  No im2col buffer exists: A is
// gathered into the LDS stage.  Before the K loop a thread decodes, with two FastDiv divisions each, the output pixels of its two rows
// (t >> 3 and 32 + (t >> 3)); per chunk it decodes the tap and channel block of the block its 16-byte segment lies in once, the same
// for both rows.  Pixel rows are Cp bytes apart: every 16-byte load is aligned.
// Padding: a tap outside the image is a real 0, which is the code zx.  The thread stores a segment filled with the byte zx for it and
// issues NO global load; the correction -zx * sums[o] the accumulators start from is then the same for every pixel.  A block at or
// past nb (tail chunk) is neither read nor multiplied.  Rows past M or O are clamped on load and not stored.
#pragma once
#include "common.hpp"
#include "job_table.hpp"
#include "int8_tile.hpp"

namespace ppqhip {

struct Int8ConvArgs {
    const uint8_t* x; const uint8_t* w;           // [n, h, w, nbc * 32], [o, nb * kBlockBytes of the codec]
    uint32_t nb, nbc;                             // nb = kh * kw * nbc (0 when x holds no pixel at all)
    uint32_t h, wd, kw;
    int32_t sh, sw, ph, pw, dh, dw;
    uint32_t fill;                                // the byte zx in all four bytes
    FastDiv ohw, ow;                              // m -> (n, oy, ox)
    FastDiv fnbc, fkw;                            // kb -> (tap, channel block), tap -> (ky, kx)
    Int8Tail e;
};

#if defined(__HIPCC__)

struct ConvRow {                                  // output pixel of one row of A: its image's first input row and the window's corner
    uint32_t img;                                 // n * h
    int32_t iy0, ix0;                             // oy * sh - ph, ox * sw - pw
};

// Where a thread's share of a chunk lies.  In the stage: as in int8_gemm.hpp.  In global memory: B by its codec's map, A by the
// decoded output pixels of its rows.
template <typename B>
struct ConvMap {
    const Int8ConvArgs& g;
    ConvRow ra[2];
    uint32_t seg, lds_e[2];
    typename B::Map bmap;

    __device__ __forceinline__ ConvMap(const Int8ConvArgs& args, uint32_t row0, uint32_t col0, uint32_t t) : g(args), bmap(args.w, args.nb, args.e.n, col0, t) {
        seg = t & 7u;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = (t >> 3) + 32u * h, pix = min(row0 + row, g.e.m - 1u);
            const uint32_t n = fdiv(pix, g.ohw), rem = pix - n * g.ohw.d, oy = fdiv(rem, g.ow), ox = rem - oy * g.ow.d;
            ra[h].img = n * g.h;
            ra[h].iy0 = (int32_t)oy * g.sh - g.ph;
            ra[h].ix0 = (int32_t)ox * g.sw - g.pw;
            lds_e[h] = row * kQ8Pitch + seg * 16u;
        }
    }

    // one gathered 16-byte segment of A: the zero point where the tap is padding (no load is issued)
    __device__ __forceinline__ v4u gather(const ConvRow& r, uint32_t cb, int32_t dy, int32_t dx) const {
        const uint32_t iy = (uint32_t)(r.iy0 + dy), ix = (uint32_t)(r.ix0 + dx);             // a negative coordinate is a huge one
        if (!(iy < g.h && ix < g.wd)) return v4u{g.fill, g.fill, g.fill, g.fill};
        const size_t block = (size_t)((r.img + iy) * g.wd + ix) * g.nbc + cb;
        return *reinterpret_cast<const v4u*>(g.x + block * kQ8Block + 16u * (seg & 1u));
    }

    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, Q8Staged<B>& st) const {
        uint32_t kb = kb0 + (seg >> 1);
        if (TAIL) kb = min(kb, g.nb - 1u);                                       // a dead block: a live one's bytes, never multiplied
        const uint32_t tap = fdiv(kb, g.fnbc), ky = fdiv(tap, g.fkw), cb = kb - tap * g.nbc;
        const int32_t dy = (int32_t)ky * g.dh, dx = (int32_t)(tap - ky * g.kw) * g.dw;
        st.a0 = gather(ra[0], cb, dy, dx); st.a1 = gather(ra[1], cb, dy, dx);
        bmap.template load<TAIL>(kb0, st.b);
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Q8Staged<B>& st) const { q8_store_staged<B>(buf, lds_e, bmap, st); }
};

template <typename B>
__global__ __launch_bounds__(kBlock, B::kMinBlocks) void q8_conv_kernel(const Int8ConvArgs g) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kQ8BufBytes<B>];
    q8_tile<B>(g.e, g.nb, stage, [&g](uint32_t row0, uint32_t col0, uint32_t t) { return ConvMap<B>(g, row0, col0, t); });
}

// the body of ppqhip_int8_conv2d / ppqhip_int4_conv2d: `what` names the entry point in its refusals, `id` books the launch
template <typename B>
int q8_conv(const char* what, KernelId id, const int8_t* x, const void* w, const Int8TailHost& t, int64_t n, int64_t c, int64_t h, int64_t wd,
            int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w,
            void* stream) {
    if (int st = check_int8_tail(what, "y", t)) return st;
    const int64_t sizes[] = {n, c, h, wd, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
    for (int64_t v : sizes) {
        if (v < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
        if (v > kQ8Max) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    }
    if (kh < 1 || kw < 1) { set_error("%s: kernel size must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (stride_h < 1 || stride_w < 1) { set_error("%s: stride must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (dil_h < 1 || dil_w < 1) { set_error("%s: dilation must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t span_h = h + 2 * pad_h - dil_h * (kh - 1) - 1, span_w = wd + 2 * pad_w - dil_w * (kw - 1) - 1;
    if (span_h < 0 || span_w < 0) { set_error("%s: the kernel window does not fit the padded input: no output", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (h + 2 * pad_h > kQ8Max || wd + 2 * pad_w > kQ8Max) { set_error("%s: a padded size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t oh = span_h / stride_h + 1, ow = span_w / stride_w + 1;
    const int64_t nbc = (c + kQ8Block - 1) / kQ8Block;
    int64_t m = bounded_product(n, oh);
    if (m >= 0) m = bounded_product(m, ow);
    int64_t nb = bounded_product(kh, kw);
    if (nb >= 0) nb = bounded_product(nb, nbc);
    int64_t blocks_x = bounded_product(n, h);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, wd);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, nbc);
    if (m < 0 || nb < 0 || blocks_x < 0) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (n == 0 || o == 0) return PPQHIP_OK;
    const bool read = blocks_x > 0 && nb > 0;                        // an input without a pixel or a channel: I is 0, nothing is read
    if (read && (x == nullptr || w == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (read && (!aligned16(x) || !aligned16(w))) { set_error("%s: operands, y and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t kp = read ? nb * kQ8Block : 0, w_row = read ? nb * B::kBlockBytes : 0;
    std::vector<Span> ins;
    if (read && kp < kQ8MaxK) { ins.push_back(span_of(x, blocks_x * kQ8Block)); ins.push_back(span_of(static_cast<const uint8_t*>(w), o * w_row)); }
    // booked: x once (a pixel is read by up to kh kw windows, from cache), w, the column data, every output and the residual
    const double bytes = read ? (double)blocks_x * kQ8Block + (double)o * (double)w_row : 0.0;

    Int8ConvArgs g;
    g.x = reinterpret_cast<const uint8_t*>(x); g.w = static_cast<const uint8_t*>(w);
    g.nb = read ? (uint32_t)nb : 0u; g.nbc = (uint32_t)nbc;
    g.h = (uint32_t)h; g.wd = (uint32_t)wd; g.kw = (uint32_t)kw;
    g.sh = (int32_t)stride_h; g.sw = (int32_t)stride_w; g.ph = (int32_t)pad_h; g.pw = (int32_t)pad_w;
    g.dh = (int32_t)dil_h; g.dw = (int32_t)dil_w;
    g.fill = 0x01010101u * ((uint32_t)t.zx & 0xffu);
    g.ohw = make_fastdiv((uint32_t)(oh * ow)); g.ow = make_fastdiv((uint32_t)ow);
    g.fnbc = make_fastdiv((uint32_t)std::max<int64_t>(nbc, 1)); g.fkw = make_fastdiv((uint32_t)kw);
    return launch_q8_tiles(what, "y", id, t, m, o, kp, ins, bytes, stream, g.e, [&g](uint32_t blocks, hipStream_t s) {
        hipLaunchKernelGGL(q8_conv_kernel<B>, dim3(blocks), dim3(kBlock), 0, s, g);
    });
}

#endif  // __HIPCC__

}  // namespace ppqhip
