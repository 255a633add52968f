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

// The A side of a thread's share of a chunk, for the dense (NA = 2) and the grouped (NA = 4, int8_gconv.hpp) convolution: the decoded
// output pixels of its rows t >> 3 + 32 h, where its segments lie in the stage, and the gather.
template <int NA>
struct ConvA {
    const Int8ConvArgs& g;
    ConvRow ra[NA];
    uint32_t seg, lds_e[NA];

    __device__ __forceinline__ ConvA(const Int8ConvArgs& args, uint32_t row0, uint32_t t) : g(args) {
        seg = t & 7u;
#pragma unroll
        for (int h = 0; h < NA; h++) {
            const uint32_t row = (t >> 3) + kQ8Slab * h, pix = min(row0 + row, g.e.m - 1u);
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

    // the thread's segment of channel block cb of tap `tap`, for each of its rows
    __device__ __forceinline__ void load(uint32_t tap, uint32_t cb, v4u (&a)[NA]) const {
        const uint32_t ky = fdiv(tap, g.fkw);
        const int32_t dy = (int32_t)ky * g.dh, dx = (int32_t)(tap - ky * g.kw) * g.dw;
#pragma unroll
        for (int h = 0; h < NA; h++) a[h] = gather(ra[h], cb, dy, dx);
    }
};

// Where a thread's share of a chunk lies.  In the stage: as in int8_gemm.hpp.  In global memory: B by its codec's map, A by the
// decoded output pixels of its rows.
template <typename B>
struct ConvMap {
    ConvA<2> a;
    typename B::Map bmap;

    __device__ __forceinline__ ConvMap(const Int8ConvArgs& g, uint32_t row0, uint32_t col0, uint32_t t) : a(g, row0, t), bmap(g.w, g.nb, g.e.n, col0, t) {}

    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, Q8Staged<B>& st) const {
        uint32_t kb = kb0 + (a.seg >> 1);
        if (TAIL) kb = min(kb, a.g.nb - 1u);                                     // a dead block: a live one's bytes, never multiplied
        const uint32_t tap = fdiv(kb, a.g.fnbc);
        a.load(tap, kb - tap * a.g.nbc, st.a);
        bmap.template load<TAIL>(kb0, st.b);
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Q8Staged<B>& st) const { q8_store_staged<B, 2>(buf, a.lds_e, bmap, st); }
};

template <typename B>
__global__ __launch_bounds__(kBlock, B::kMinBlocks) void q8_conv_kernel(const Int8ConvArgs g) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kQ8BufBytes<B>];
    q8_tile<B>(g.e, g.nb, stage, [&g](uint32_t row0, uint32_t col0, uint32_t t) { return ConvMap<B>(g, row0, col0, t); });
}

// a convolution as an entry point received it, and what the checks make of it
struct ConvShape {
    int64_t n, c, h, wd, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int64_t oh, ow, nbc, m, blocks_x;             // nbc = ceil(c / 32); m = n oh ow rows; blocks_x = n h wd nbc blocks of x
};

// What the dense and the grouped entry point check about the geometry, in this order; `extra` are further sizes (groups, nbs) that
// must lie in 0 .. 2^31 - 1.  Fills oh .. blocks_x; a product above 2^31 - 1 is left as -1 for the caller's own size check.
inline int check_conv_shape(const char* what, ConvShape& z, std::initializer_list<int64_t> extra = {}) {
    std::vector<int64_t> sizes = {z.n, z.c, z.h, z.wd, z.o, z.kh, z.kw, z.stride_h, z.stride_w, z.pad_h, z.pad_w, z.dil_h, z.dil_w};
    sizes.insert(sizes.end(), extra);
    for (int64_t v : sizes) {
        if (v < 0) { set_error("%s: negative size", what); return PPQHIP_ERR_INVALID_VALUE; }
        if (v > kQ8Max) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    }
    if (z.kh < 1 || z.kw < 1) { set_error("%s: kernel size must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (z.stride_h < 1 || z.stride_w < 1) { set_error("%s: stride must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (z.dil_h < 1 || z.dil_w < 1) { set_error("%s: dilation must be at least 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t span_h = z.h + 2 * z.pad_h - z.dil_h * (z.kh - 1) - 1, span_w = z.wd + 2 * z.pad_w - z.dil_w * (z.kw - 1) - 1;
    if (span_h < 0 || span_w < 0) { set_error("%s: the kernel window does not fit the padded input: no output", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (z.h + 2 * z.pad_h > kQ8Max || z.wd + 2 * z.pad_w > kQ8Max) { set_error("%s: a padded size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    z.oh = span_h / z.stride_h + 1; z.ow = span_w / z.stride_w + 1;
    z.nbc = (z.c + kQ8Block - 1) / kQ8Block;
    z.m = bounded_product(z.n, z.oh);
    if (z.m >= 0) z.m = bounded_product(z.m, z.ow);
    z.blocks_x = bounded_product(z.n, z.h);
    if (z.blocks_x >= 0) z.blocks_x = bounded_product(z.blocks_x, z.wd);
    if (z.blocks_x >= 0) z.blocks_x = bounded_product(z.blocks_x, z.nbc);
    return PPQHIP_OK;
}

// The rest of either entry point once its reduction is known: a row of the implicit GEMM has nb blocks, of which nbk belong to one
// tap (the dense layer's nbc, the grouped one's nbs).  Checks the products, the operands' pointers and alignment, books, fills g (but
// for its tail) and hands over to launch_q8_tiles<NA>; `more` are further inputs to check for overlaps.
template <typename B, int NA, typename Launch>
int launch_q8_conv(const char* what, KernelId id, const int8_t* x, const void* w, const Int8TailHost& t, const ConvShape& z, int64_t nbk,
                   std::vector<Span> more, void* stream, Int8ConvArgs& g, Launch&& launch) {
    int64_t nb = bounded_product(z.kh, z.kw);
    if (nb >= 0) nb = bounded_product(nb, nbk);
    if (z.m < 0 || nb < 0 || z.blocks_x < 0) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (z.n == 0 || z.o == 0) return PPQHIP_OK;
    const bool read = z.blocks_x > 0 && nb > 0;                      // an input without a pixel or a channel: I is 0, nothing is read
    if (read && (x == nullptr || w == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (read && (!aligned16(x) || !aligned16(w))) { set_error("%s: operands, y and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t kp = read ? nb * kQ8Block : 0, w_row = read ? nb * B::kBlockBytes : 0;
    std::vector<Span> ins;
    if (read && kp < kQ8MaxK) {
        ins.push_back(span_of(x, z.blocks_x * kQ8Block)); ins.push_back(span_of(static_cast<const uint8_t*>(w), z.o * w_row));
        ins.insert(ins.end(), more.begin(), more.end());
    }
    // booked: x once (a pixel is read by up to kh kw windows, from cache), w, the column data, every output and the residual
    const double bytes = read ? (double)z.blocks_x * kQ8Block + (double)z.o * (double)w_row : 0.0;

    g.x = reinterpret_cast<const uint8_t*>(x); g.w = static_cast<const uint8_t*>(w);
    g.nb = read ? (uint32_t)nb : 0u; g.nbc = (uint32_t)z.nbc;
    g.h = (uint32_t)z.h; g.wd = (uint32_t)z.wd; g.kw = (uint32_t)z.kw;
    g.sh = (int32_t)z.stride_h; g.sw = (int32_t)z.stride_w; g.ph = (int32_t)z.pad_h; g.pw = (int32_t)z.pad_w;
    g.dh = (int32_t)z.dil_h; g.dw = (int32_t)z.dil_w;
    g.fill = 0x01010101u * ((uint32_t)t.zx & 0xffu);
    g.ohw = make_fastdiv((uint32_t)(z.oh * z.ow)); g.ow = make_fastdiv((uint32_t)z.ow);
    g.fnbc = make_fastdiv((uint32_t)std::max<int64_t>(nbk, 1)); g.fkw = make_fastdiv((uint32_t)z.kw);
    return launch_q8_tiles<NA>(what, "y", id, t, z.m, z.o, kp, ins, bytes, stream, g.e, launch);
}

// the body of ppqhip_int8_conv2d / ppqhip_int4_conv2d: `what` names the entry point in its refusals, `id` books the launch
template <typename B>
int q8_conv(const char* what, KernelId id, const int8_t* x, const void* w, const Int8TailHost& t, int64_t n, int64_t c, int64_t h, int64_t wd,
            int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w,
            void* stream) {
    if (int st = check_int8_tail(what, "y", t)) return st;
    ConvShape z = {n, c, h, wd, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
    if (int st = check_conv_shape(what, z)) return st;
    Int8ConvArgs g;
    return launch_q8_conv<B, 2>(what, id, x, w, t, z, z.nbc, {}, stream, g, [&g](uint32_t blocks, hipStream_t s) {
        hipLaunchKernelGGL(q8_conv_kernel<B>, dim3(blocks), dim3(kBlock), 0, s, g);
    });
}

#endif  // __HIPCC__

}  // namespace ppqhip
