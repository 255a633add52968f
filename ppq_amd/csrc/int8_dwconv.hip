// int8_dwconv.hip -- a depthwise linear INT8 convolution (groups == C, channel multiplier 1) as an integer backend runs it, on
// v_dot4c_i32_i8.  The contract is DESIGN.md section 9.24 and tests/int8_depthwise_reference.py: the one of int8_tile.hpp with the sum
// over k replaced by the sum over the taps of ONE channel,
//   I[n, oy, ox, c] = sum_{ky, kx} w[c, ky, kx] (x[n, iy, ix, c] - zx),   (iy, ix) = (oy * sh - ph + ky * dh, ox * sw - pw + kx * dw),
// a tap outside the image being a real 0, i.e. the code zx; then q8_value / q8_code of int8_tile.hpp per output, the very functions of
// the MFMA kernels' epilogue: the result has the bits of ppqhip_int8_conv2d on the dense [C, C, kh, kw] weight that is zero off the
// diagonal.  Nothing of those kernels' frame fits: there is no reduction over channels (K is kh kw = 9 .. 49 taps), so the MFMA has
// nothing to multiply and the layer is bound by the bytes it moves.
//
// Operands: x [N, H, W, Cp] int8 codes as int8_quantize(x, cfg, 1) makes them, Cp = ceil32(C); w [kh, kw, Cp] int8, tap-major and
// channels-last, the channels C .. Cp - 1 code 0; sums [C] = sum of a channel's taps; mul, bias [C]; y [N, OH, OW, C] float32 and / or
// q [N, OH, OW, Cp] int8 with zy in the padding channels; residual as y.
//
// Work split.  A workgroup of 256 lanes owns an 8 x 8 tile of output pixels of one image times one block of 32 channels; the grid is
// one-dimensional over N x ceil(OH / 8) x ceil(OW / 8) x Cp / 32, the channel block fastest (neighbouring workgroups read neighbouring
// 32-byte pieces of the same cache lines), decoded with FastDiv; addresses are size_t.  Lane t owns the channel dword t & 7 (4
// channels) of the tile's pixels t >> 3 and 32 + (t >> 3) (pixel p is row p >> 3, column p & 7: a wave is one row of the tile, twice)
// and carries 2 x 4 int32 accumulators, started from -zx * sums[c] (0 without sums).
//
// Through LDS.  Before any arithmetic the workgroup stages the PH x PW input pixels its tile reads, PH = 7 sh + (kh - 1) dh + 1 and
// PW likewise, 32 bytes each, with aligned 16-byte loads from the Cp-pitched rows.  A patch pixel outside the image is stored as the
// byte zx and NO load is issued for it, so the start -zx * sums is right for every output, padding included.  An input byte is read
// from HBM / L2 once per tile and then up to kh kw times from LDS.  The kh kw x 32 weight bytes of the block are staged once and
// EXPANDED as they are stored: per (tap, channel dword) the four dwords w & 0xff, w & 0xff00, w & 0xff0000, w & 0xff000000, so that
// one ds_read_b128 hands a lane the four one-byte-live weights of a tap (lanes of one channel dword read one address: a broadcast).
//
// The multiply.  __builtin_amdgcn_sdot4(x dword, one-byte-live weight, acc, no clamp): with three of the weight's bytes zero the dot
// product of four channels is x[j] w[j] of the live one, exactly, in int32 -- four instructions per tap and dword of channels, no
// byte extraction, no sign extension.  The tap loop runs over runtime kh, kw (K == 0); a 3 x 3 window takes the instance K == 3, whose
// loop is unrolled with every LDS offset folded and the nine weight groups read once into registers.
// int32: |w| <= 128, |x - zx| <= 255, and a window that fits the LDS budget has at most 512 taps: kh kw 128 255 < 2^31 with room to
// spare, for every partial sum as well (|zx sums| + |sum w x| <= 2 * 512 * 2^14 = 2^24).  No separate overflow refusal is needed.
//
// LDS banks (derived from the lane-to-address map, not measured; 64 banks of 4 bytes as in int8_tile.hpp).  A wave's 64 lanes read the
// dwords (px * sw * pitch + const) / 4 + (t & 7), px = 0 .. 7.  Pitch 32 bytes: the 8 pixels start 8 sw dwords apart; for odd sw the
// residues 8 sw px mod 64 are the 8 multiples of 8, each once: 64 lanes, 64 banks.  For sw = 2 they are 0, 16, 32, 48 twice each:
// every bank is asked for two different dwords (2-way).  So where sw % 4 == 2 the pixel pitch is 48 bytes: the starts are
// 24 px (sw / 2) mod 64, again the 8 multiples of 8 each once -- conflict-free, 16-byte stores still aligned, half as much LDS again.
// For sw % 4 == 0 no pitch that is a multiple of 16 bytes separates the pixels (4 k sw = 8 odd has no solution mod 64): pitch 32
// stays, 4-way at sw = 4; no calibrated network this project has met strides a depthwise layer by 4.
//
// The store.  A lane's four channels of a pixel leave as one 16-byte store of y where C % 4 == 0 (y is 16-byte aligned and a row has
// 4 C bytes), as scalar stores of the live channels otherwise, and as ONE dword of q (Cp % 32 == 0: always aligned); the residual is
// read the same way.  Channels at or past C are not stored to y and hold zy in q.  Pixels past the tile's live edge are computed on
// clamped coordinates and not stored.
//
// LDS is dynamic, sized by the host to what the geometry needs (4352 bytes for 3 x 3 at stride 1), not a static 64 KiB array: a static
// array of the budget's size would hold every launch to two workgroups a compute unit, whatever its window.  The budget is 64 KiB.
#include "int8_tile.hpp"

using namespace ppqhip;

namespace ppqhip {

constexpr uint32_t kDwEdge = 8;                                                   // output pixels per tile edge
constexpr uint32_t kDwLdsBudget = 65536;
static_assert(kDwEdge * kDwEdge * (kQ8Block / 4u) == 2u * (uint32_t)kBlock, "two pixels of one channel dword per lane");

struct Int8DwArgs {
    const uint8_t* x; const uint8_t* w;           // [n, h, w, cp], [kh, kw, cp]
    uint32_t cp, h, wd, kh, kw, oh, ow;           // kh = kw = 0 where x holds no pixel at all: nothing is read
    uint32_t sh, sw, dh, dw;
    int32_t ph, pw;
    uint32_t prow, pcol, pitch, wbase;            // the staged patch: rows, columns, bytes per pixel; where the weights start
    uint32_t fill;                                // the byte zx in all four bytes
    FastDiv fcb, ftx, fty, fpcol;                 // workgroup -> (n, tile row, tile column, channel block); patch pixel -> (row, column)
    Int8Tail e;                                   // m = n oh ow pixels, n = c, op = cp; tiles_n is not used
};

template <int K>                                  // K > 0: a K x K window, unrolled; 0: any window
__global__ __launch_bounds__(kBlock) void q8_dwconv_kernel(const Int8DwArgs g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const Int8Tail& e = g.e;
    const uint32_t kh = K ? (uint32_t)K : g.kh, kw = K ? (uint32_t)K : g.kw;
    const uint32_t t = threadIdx.x;
    uint32_t rest = fdiv(blockIdx.x, g.fcb);
    const uint32_t cb = blockIdx.x - rest * g.fcb.d;
    const uint32_t rest2 = fdiv(rest, g.ftx), tx = rest - rest2 * g.ftx.d;
    const uint32_t n = fdiv(rest2, g.fty), ty = rest2 - n * g.fty.d;
    const uint32_t oy0 = ty * kDwEdge, ox0 = tx * kDwEdge;

    // the patch: 16-byte segment i & 1 of patch pixel i >> 1
    const int32_t iy0 = (int32_t)(oy0 * g.sh) - g.ph, ix0 = (int32_t)(ox0 * g.sw) - g.pw;
    const uint8_t* xb = g.x + (size_t)cb * kQ8Block;
    for (uint32_t i = t; i < g.prow * g.pcol * 2u; i += kBlock) {
        const uint32_t pix = i >> 1, half = i & 1u, r = fdiv(pix, g.fpcol), c = pix - r * g.pcol;
        const uint32_t iy = (uint32_t)(iy0 + (int32_t)r), ix = (uint32_t)(ix0 + (int32_t)c);     // a negative coordinate is a huge one
        v4u v = v4u{g.fill, g.fill, g.fill, g.fill};
        if (iy < g.h && ix < g.wd) v = *reinterpret_cast<const v4u*>(xb + (size_t)((n * g.h + iy) * g.wd + ix) * g.cp + 16u * half);
        *reinterpret_cast<v4u*>(lds + pix * g.pitch + 16u * half) = v;
    }
    // the weights, expanded: dword i & 7 of tap i >> 3
    for (uint32_t i = t; i < kh * kw * (kQ8Block / 4u); i += kBlock) {
        const uint32_t wv = *reinterpret_cast<const uint32_t*>(g.w + (size_t)(i >> 3) * g.cp + cb * kQ8Block + (i & 7u) * 4u);
        *reinterpret_cast<v4u*>(lds + g.wbase + i * 16u) = v4u{wv & 0xffu, wv & 0xff00u, wv & 0xff0000u, wv & 0xff000000u};
    }
    __syncthreads();

    const uint32_t cd = t & 7u, c0 = cb * kQ8Block + cd * 4u;
    uint32_t oy[2], ox[2], base[2]; bool live[2];
    int acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const uint32_t py = (t >> 6) + 4u * p, px = (t >> 3) & 7u;
        live[p] = oy0 + py < g.oh && ox0 + px < g.ow;
        oy[p] = min(oy0 + py, g.oh - 1u); ox[p] = min(ox0 + px, g.ow - 1u);
        base[p] = ((oy[p] - oy0) * g.sh * g.pcol + (ox[p] - ox0) * g.sw) * g.pitch + cd * 4u;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t col = min(c0 + j, e.n - 1u);
        const int s = e.sums != nullptr ? (int)(0u - (uint32_t)e.zx * (uint32_t)e.sums[col]) : 0;
        acc[0][j] = s; acc[1][j] = s;
    }
    const uint8_t* lw = lds + g.wbase + cd * 16u;
    const uint32_t row_step = g.dh * g.pcol * g.pitch, col_step = g.dw * g.pitch;
    for (uint32_t ky = 0; ky < kh; ky++) {                                        // K > 0: constant bounds, unrolled by the compiler
        for (uint32_t kx = 0; kx < kw; kx++) {
            const v4u wv = *reinterpret_cast<const v4u*>(lw + (ky * kw + kx) * (kQ8Block / 4u) * 16u);
            const uint32_t off = ky * row_step + kx * col_step;
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const int xd = *reinterpret_cast<const int*>(lds + base[p] + off);
#pragma unroll
                for (int j = 0; j < 4; j++) acc[p][j] = __builtin_amdgcn_sdot4(xd, (int)wv[j], acc[p][j], false);
            }
        }
    }

    float mul[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t col = min(c0 + j, e.n - 1u);
        mul[j] = e.mul[col];
        b[j] = e.bias != nullptr ? e.bias[col] : 0.f;
    }
    const bool vec = (e.n & 3u) == 0u && c0 < e.n;                                // the lane's four channels are live and 16-byte aligned
    const uint32_t pad_code = (uint32_t)(int)e.zy & 0xffu;
#pragma unroll
    for (int p = 0; p < 2; p++) {
        if (!live[p]) continue;
        const uint32_t row = (n * g.oh + oy[p]) * g.ow + ox[p];
        const size_t at = (size_t)row * e.n + c0;
        float res[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
        if (e.residual != nullptr) {
            if (vec) {
                const v4u r = *reinterpret_cast<const v4u*>(e.residual + at);
#pragma unroll
                for (int j = 0; j < 4; j++) res[j] = __uint_as_float(r[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) if (c0 + j < e.n) res[j] = e.residual[at + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = q8_value(e, acc[p][j], mul[j], b[j], res[j]);
        if (e.c != nullptr) {
            if (vec) *reinterpret_cast<v4u*>(e.c + at) = v4u{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) if (c0 + j < e.n) e.c[at + j] = v[j];
            }
        }
        if (e.q != nullptr) {
            uint32_t codes = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) codes |= (c0 + j < e.n ? q8_code(e, v[j]) & 0xffu : pad_code) << (8 * j);
            *reinterpret_cast<uint32_t*>(e.q + (size_t)row * e.op + c0) = codes;
        }
    }
}

}  // namespace ppqhip

extern "C" int ppqhip_int8_dwconv2d(const int8_t* x, const int8_t* w, const int32_t* w_sums, int zx, const float* mul, const float* bias,
                                    const float* residual, int relu, float* y, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding,
                                    int q_nan, int64_t n, int64_t c, int64_t h, int64_t wd, int64_t kh, int64_t kw, int64_t stride_h,
                                    int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream) {
    const char* what = "int8_dwconv2d";
    const Int8TailHost t = {w_sums, zx, mul, bias, residual, relu, y, q, sy, zy, qmin, qmax, rounding, q_nan};
    if (int st = check_int8_tail(what, "y", t)) return st;
    const int64_t sizes[] = {n, c, h, wd, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
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
    const int64_t nbc = (c + kQ8Block - 1) / kQ8Block, cp = nbc * kQ8Block;
    int64_t m = bounded_product(n, oh);
    if (m >= 0) m = bounded_product(m, ow);
    int64_t blocks_x = bounded_product(n, h);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, wd);
    if (blocks_x >= 0) blocks_x = bounded_product(blocks_x, nbc);
    if (m < 0 || blocks_x < 0) { set_error("%s: a size above 2^31 - 1", what); return PPQHIP_ERR_INVALID_VALUE; }
    // the staged patch and the expanded weights; every factor is below 2^31 and the first product that passes the budget ends the sum
    const int64_t prow = (kDwEdge - 1) * stride_h + (kh - 1) * dil_h + 1, pcol = (kDwEdge - 1) * stride_w + (kw - 1) * dil_w + 1;
    const int64_t pitch = stride_w % 4 == 2 ? 48 : 32;
    const double need = (double)prow * (double)pcol * (double)pitch + (double)kh * (double)kw * 128.0;
    if (need > (double)kDwLdsBudget) {
        set_error("%s: a %lld x %lld window at stride (%lld, %lld) and dilation (%lld, %lld) stages %.0f bytes of LDS: a workgroup has %u",
                  what, (long long)kh, (long long)kw, (long long)stride_h, (long long)stride_w, (long long)dil_h, (long long)dil_w, need, kDwLdsBudget);
        return PPQHIP_ERR_UNSUPPORTED;
    }
    if (n == 0 || c == 0) return PPQHIP_OK;
    const bool read = blocks_x > 0;                                  // an input without a pixel: I is 0, nothing is read
    if (read && (x == nullptr || w == nullptr)) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (read && (!aligned16(x) || !aligned16(w))) { set_error("%s: operands, y and q must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t taps = kh * kw, kp = read ? taps * kQ8Block : 0;
    std::vector<Span> ins;
    if (read) { ins.push_back(span_of(x, blocks_x * kQ8Block)); ins.push_back(span_of(w, taps * cp)); }
    // booked: x once (a pixel is read by up to four tiles' patches, from cache), w, the channel data, every output and the residual
    const double bytes = read ? (double)blocks_x * kQ8Block + (double)taps * (double)cp : 0.0;
    const int64_t tiles_y = (oh + kDwEdge - 1) / kDwEdge, tiles_x = (ow + kDwEdge - 1) / kDwEdge;
    int64_t workgroups = bounded_product(n, tiles_y);
    if (workgroups >= 0) workgroups = bounded_product(workgroups, tiles_x);
    if (workgroups >= 0) workgroups = bounded_product(workgroups, nbc);

    Int8DwArgs g;
    g.x = reinterpret_cast<const uint8_t*>(x); g.w = reinterpret_cast<const uint8_t*>(w);
    g.cp = (uint32_t)cp; g.h = (uint32_t)h; g.wd = (uint32_t)wd; g.oh = (uint32_t)oh; g.ow = (uint32_t)ow;
    g.kh = read ? (uint32_t)kh : 0u; g.kw = read ? (uint32_t)kw : 0u;
    g.sh = (uint32_t)stride_h; g.sw = (uint32_t)stride_w; g.dh = (uint32_t)dil_h; g.dw = (uint32_t)dil_w;
    g.ph = (int32_t)pad_h; g.pw = (int32_t)pad_w;
    g.prow = read ? (uint32_t)prow : 0u; g.pcol = read ? (uint32_t)pcol : 0u; g.pitch = (uint32_t)pitch;
    g.wbase = g.prow * g.pcol * g.pitch;
    g.fill = 0x01010101u * ((uint32_t)zx & 0xffu);
    g.fcb = make_fastdiv((uint32_t)nbc); g.ftx = make_fastdiv((uint32_t)tiles_x); g.fty = make_fastdiv((uint32_t)tiles_y);
    g.fpcol = make_fastdiv((uint32_t)pcol);
    g.e.tiles_n = make_fastdiv(1u);
    const uint32_t lds_bytes = read ? (uint32_t)need : 0u;
    const bool k3 = read && kh == 3 && kw == 3;
    return launch_q8(what, "y", K_INT8_DWCONV, t, m, c, kp, workgroups, ins, bytes, stream, g.e, [&g, lds_bytes, k3](uint32_t blocks, hipStream_t s) {
        if (k3) hipLaunchKernelGGL(q8_dwconv_kernel<3>, dim3(blocks), dim3(kBlock), lds_bytes, s, g);
        else hipLaunchKernelGGL(q8_dwconv_kernel<0>, dim3(blocks), dim3(kBlock), lds_bytes, s, g);
    });
}
