// mx_conv.hip -- Y[M, O] (float32) = conv2d(x, w) (+ bias[O]) on packed OCP Microscaling operands, through the block-scaled MFMA of
// gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4): an implicit GEMM.  The contract is DESIGN.md section 9.15 and tests/mx_conv_reference.py.
//
// Both operands are read exactly as mx_pack.hip leaves a 4-D tensor packed along axis 1 (the block axis is
// stored last): the activation x [N, C, H, W] as elements [N, H, W, nbc * BA] and scales [N, H, W, nbc], the weight w [O, C, kh, kw] as
// elements [O, kh, kw, nbc * BB] and scales [O, kh, kw, nbc], nbc = ceil(C / 32).  The weight IS the B operand of mx_gemm.hip,
// [O, nb'] with nb' = kh * kw * nbc blocks per row ordered (ky, kx, channel block), and is read by the same code.  Row m of the A
// operand is output pixel (n, oy, ox), M = N * OH * OW rows in that order; its block kb is channel block kb % nbc of input pixel
//   (iy, ix) = (oy * sh - ph + ky * dh, ox * sw - pw + kx * dw),   (ky, kx) = divmod(kb / nbc, kw),
// found in x at block ((n * H + iy) * W + ix) * nbc + kb % nbc.  A tap that falls into the padding is not read and feeds zero element
// bits and scale code 127, as a block past nb' does in either kernel; no im2col buffer exists.
// The lanes are those of mx_gemm.hip (mx_mfma.hpp): an FP6 / FP4 lane needs the one block kb0 + g of its K-step, an FP8 lane the
// halves of blocks kb0 + (g >> 1) and kb0 + 2 + (g >> 1) -- with nbc % 4 != 0 two different taps, hence two different pixels -- and
// the scale byte of block kb0 + g, a third address.  m -> (n, oy, ox) is decoded once per row before the K loop.
// FP6 pixel rows are 24 nbc bytes apart, 8 mod 16 for an odd nbc: the 8-byte loads of the FP6 blocks cover that.
// Y is [N, OH, OW, O] row-major: the channels-last storage of a [N, O, OH, OW] tensor.
// One accumulation order (ascending kb, one K-step per instruction), no atomics, no split-K: two launches give identical bits, and
// the bits are those of mx_gemm.hip on the gathered A operand: same instructions, same register contents, same order.
// NaN: as in mx_gemm.hip; padding is not read, so an output is NaN exactly when its window covers a NaN block of x, or its output
// channel holds one in w.
// ppqhip_mx_conv2d_fused runs the same K loop with the fused epilogue of mx_mfma.hpp: residual, ReLU and the result
// packed along the output columns, in a second set of 25 instantiations; the plain kernels keep their code.
// What the kernel shares with mx_gemm_kernel is in mx_mfma.hpp; what is here is its A source: the
// implicit-GEMM addressing.
#include "common.hpp"
#include "mx_mfma.hpp"

namespace ppqhip {
namespace {

struct MxConvArgs {
    const uint8_t* xe; const uint8_t* xs;         // x: elements [n, h, w, nbc * BA], scales [n, h, w, nbc]
    MxTileArgs t;                                 // B is w [o, nb * BB] / [o, nb], c is y [m, o]; nb = kh * kw * nbc (0 when x holds no block at all)
    uint32_t nbc;
    uint32_t h, w, kw;
    int32_t sh, sw, ph, pw, dh, dw;
    FastDiv ohw, ow;                              // m -> (n, oy, ox)
    FastDiv fnbc, fkw;                            // kb -> (tap, channel block), tap -> (ky, kx)
};

struct ConvRow {                                  // output pixel of one row of A: its image's first input row and the window's corner
    uint32_t img;                                 // n * h
    int32_t iy0, ix0;                             // oy * sh - ph, ox * sw - pw
};
struct ConvTap {                                  // block kb of a row of A: the same for every row
    uint32_t cb;                                  // channel block
    int32_t dy, dx;                               // ky * dh, kx * dw
    bool live;                                    // kb < nb
};

template <bool TAIL>
__device__ __forceinline__ ConvTap conv_tap(const MxConvArgs& g, uint32_t kb) {
    ConvTap t;
    t.live = !TAIL || kb < g.t.nb;
    if (TAIL) kb = min(kb, g.t.nb - 1u);
    const uint32_t tap = fdiv(kb, g.fnbc), ky = fdiv(tap, g.fkw);
    t.cb = kb - tap * g.nbc;
    t.dy = (int32_t)ky * g.dh;
    t.dx = (int32_t)(tap - ky * g.kw) * g.dw;
    return t;
}

// the block of x behind tap t of row r: false, and block 0 (always readable), where the tap is padding or past nb
__device__ __forceinline__ bool conv_block(const MxConvArgs& g, const ConvRow& r, const ConvTap& t, uint32_t& block) {
    const uint32_t iy = (uint32_t)(r.iy0 + t.dy), ix = (uint32_t)(r.ix0 + t.dx);      // a negative coordinate is a huge one
    const bool in = t.live && iy < g.h && ix < g.w;
    block = in ? ((r.img + iy) * g.w + ix) * g.nbc + t.cb : 0u;
    return in;
}

// The A source of the kernel (mx_mfma.hpp, RowSource): m -> (n, oy, ox) once per row, then per K-step what RowSource gives for a packed row --
// the operand registers of K-step kb0 / 4 and the scale code of block kb0 + grp -- every block through its own computed address.
template <int F>
struct ConvSource {
    const MxConvArgs& g;
    ConvRow rows[kGemmWaveTiles];                 // the lane's rows, set by prepare

    __device__ __forceinline__ void prepare(uint32_t m0, uint32_t r) {
#pragma unroll
        for (int t = 0; t < kGemmWaveTiles; t++) {
            const uint32_t row = min(m0 + t * kGemmTile + r, g.t.m - 1u);
            const uint32_t n = fdiv(row, g.ohw), rem = row - n * g.ohw.d, oy = fdiv(rem, g.ow), ox = rem - oy * g.ow.d;
            rows[t].img = n * g.h;
            rows[t].iy0 = (int32_t)oy * g.sh - g.ph;
            rows[t].ix0 = (int32_t)ox * g.sw - g.pw;
        }
    }
    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, uint32_t grp, v8i (&frag)[kGemmWaveTiles], int (&scale)[kGemmWaveTiles],
                                         uint32_t (&nan)[kGemmWaveTiles]) const {
        constexpr uint32_t bits = gemm_elem_bits(F);
        const ConvTap ts = conv_tap<TAIL>(g, kb0 + grp);
        const ConvTap t0 = conv_tap<TAIL>(g, kb0 + (grp >> 1)), t1 = conv_tap<TAIL>(g, kb0 + 2u + (grp >> 1));       // FP8 only
        const uint32_t half = 16u * (grp & 1u);
#pragma unroll
        for (int t = 0; t < kGemmWaveTiles; t++) {
            uint32_t bs;
            const bool ins = conv_block(g, rows[t], ts, bs);
            if (bits == 8u) {
                uint32_t b0, b1;
                const bool in0 = conv_block(g, rows[t], t0, b0), in1 = conv_block(g, rows[t], t1, b1);
                frag[t] = fp8_fragment(g.xe + (size_t)b0 * 32u + half, g.xe + (size_t)b1 * 32u + half, in0, in1);
            } else {
                frag[t] = block_fragment<F>(g.xe + (size_t)bs * (4u * bits), ins);
            }
            const int s = (int)g.xs[bs];
            scale[t] = ins ? s : 127;
        }
        flag_nan<F>(frag, scale, nan);
    }
};

// F is empty -- the plain kernel, (g) alone -- or one MxFusedOut: the epilogue of mx_mfma.hpp (fused_epilogue) in place of the plain
// one, (g, f).  Everything up to the epilogue is the same code; in the fused kernel g.t.c may be null.  The text of this kernel
// and of mx_gemm_kernel (mx_gemm.hip) differs in the A source alone; it stays in the kernel because the backend schedules the FP8 K loops worse
// when it is an inlined function (profiles/mx_tile.txt).
template <int FA, int FB, typename... F>
__global__ __launch_bounds__(kBlock) void mx_conv_kernel(const MxConvArgs g, const F... f) {
    constexpr bool FUSED = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one MxFusedOut");
    constexpr int T = kGemmWaveTiles;
    const MxTileArgs& t = g.t;
    const uint32_t tm = fdiv(blockIdx.x, t.tiles_n), tn = blockIdx.x - tm * t.tiles_n.d;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 15u, grp = lane >> 4;
    const uint32_t m0 = tm * kGemmEdge + (wave / kGemmWaves) * (T * kGemmTile);
    const uint32_t n0 = tn * kGemmEdge + (wave % kGemmWaves) * (T * kGemmTile);
    if (m0 >= t.m || n0 >= t.n) return;                                          // wave-uniform; there is no barrier below

    ConvSource<FA> a_src{g};
    RowSource<FB> b_src{t.be, t.bs, t.n, t.nb};
    a_src.prepare(m0, r);
    b_src.prepare(n0, r);
    v4f acc[T][T];
#pragma unroll
    for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    uint32_t nan_a[T], nan_b[T];
#pragma unroll
    for (int i = 0; i < T; i++) { nan_a[i] = 0u; nan_b[i] = 0u; }

    const uint32_t full = t.nb / kGemmStepBlocks;
    for (uint32_t s = 0; s < full; s++) mx_tile_step<FA, FB, false>(a_src, b_src, s * kGemmStepBlocks, grp, acc, nan_a, nan_b);
    if (t.nb % kGemmStepBlocks) mx_tile_step<FA, FB, true>(a_src, b_src, full * kGemmStepBlocks, grp, acc, nan_a, nan_b);

    uint32_t rows_nan[T], cols_nan[T];
#pragma unroll
    for (int i = 0; i < T; i++) { rows_nan[i] = tile_flags(nan_a[i]); cols_nan[i] = tile_flags(nan_b[i]); }
    if constexpr (FUSED) {                                                       // the stage is wave-private: no barrier, the early return stands
        __shared__ __attribute__((aligned(16))) uint8_t stage[kGemmWaves * kGemmWaves * kFusedStageBytes];
        fused_epilogue(acc, rows_nan, cols_nan, t.bias, t.c, t.m, t.n, m0, n0, lane, f..., stage + wave * kFusedStageBytes);
        return;
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        const uint32_t col = n0 + j * kGemmTile + r;
        if (col >= t.n) continue;
        const float bias = t.bias != nullptr ? t.bias[col] : 0.f;
        const bool col_nan = (cols_nan[j] >> r) & 1u;
#pragma unroll
        for (int i = 0; i < T; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t tr = grp * 4u + q, row = m0 + i * kGemmTile + tr;
                const bool bad = col_nan || ((rows_nan[i] >> tr) & 1u);
                const float v = t.bias != nullptr ? acc[i][j][q] + bias : acc[i][j][q];
                if (row < t.m) t.c[(size_t)row * t.n + col] = bad ? __uint_as_float(0x7fc00000u) : v;
            }
        }
    }
}

// a * b when it stays within 2^31 - 1 (both are within it already), -1 otherwise
int64_t bounded_product(int64_t a, int64_t b) {
    const int64_t p = a * b;
    return p > kMxMax ? -1 : p;
}

// both entry points; `fused` is null for ppqhip_mx_conv2d, whose checks, strings and launch are unchanged
int run_conv(const char* what, const uint8_t* x_elements, const uint8_t* x_scales, int x_format, const uint8_t* w_elements,
             const uint8_t* w_scales, int w_format, const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t w, int64_t o,
             int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w,
             const MxFusedHost* fused, void* stream) {
    if (int st = check_format(what, "x", x_format)) return st;
    if (int st = check_format(what, "w", w_format)) return st;
    MxFusedOut f = {};
    if (fused != nullptr) {
        if (int st = check_fused_outputs(what, "y", y, fused->out_elements, fused->out_scales, fused->out_format, &f.fmt)) return st;
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
    const int64_t BA = 4 * (int64_t)gemm_elem_bits(x_format), BB = 4 * (int64_t)gemm_elem_bits(w_format);
    if ((y == nullptr && fused == nullptr) || (read_x && (x_elements == nullptr || x_scales == nullptr)) || (read_w && (w_elements == nullptr || w_scales == nullptr))) {
        set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (!aligned16(y) || (read_x && !aligned16(x_elements)) || (read_w && !aligned16(w_elements))) {
        set_error("%s: elements and y must be 16-byte aligned", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    std::vector<Span> ins, outs;
    if (read_x) { ins.push_back(span_of(x_elements, blocks_x * BA)); ins.push_back(span_of(x_scales, blocks_x)); }
    if (read_w) { ins.push_back(span_of(w_elements, o * nb * BB)); ins.push_back(span_of(w_scales, o * nb)); }
    if (bias != nullptr) ins.push_back(span_of(bias, o));
    if (y != nullptr) outs.push_back(span_of(y, m * o));
    // booked: packed x once (a pixel is read by up to kh kw windows, from cache), packed w and 4 m o bytes of y; the launch does
    // 2 m o nb 32 flops
    double bytes = (double)blocks_x * (double)(BA + 1) + (double)o * (double)nb * (double)(BB + 1);
    if (y != nullptr) bytes += 4.0 * (double)m * (double)o;
    MxConvArgs g;
    g.xe = x_elements; g.xs = x_scales;
    g.t.be = w_elements; g.t.bs = w_scales; g.t.bias = bias; g.t.c = y;
    g.t.m = (uint32_t)m; g.t.n = (uint32_t)o; g.nbc = (uint32_t)nbc;
    g.t.nb = read_w ? (uint32_t)nb : 0u;
    g.h = (uint32_t)h; g.w = (uint32_t)w; g.kw = (uint32_t)kw;
    g.sh = (int32_t)stride_h; g.sw = (int32_t)stride_w; g.ph = (int32_t)pad_h; g.pw = (int32_t)pad_w;
    g.dh = (int32_t)dil_h; g.dw = (int32_t)dil_w;
    g.ohw = make_fastdiv((uint32_t)(oh * ow)); g.ow = make_fastdiv((uint32_t)ow);
    g.fnbc = make_fastdiv((uint32_t)std::max<int64_t>(nbc, 1)); g.fkw = make_fastdiv((uint32_t)kw);
    return launch_mx_tiles(what, K_MX_CONV, K_MX_CONV_FUSED, x_format, w_format, fused, f, g.t, ins, outs, bytes, stream,
                           [&g](auto fa, auto fb, uint32_t blocks, hipStream_t s, const auto&... fo) {
        hipLaunchKernelGGL((mx_conv_kernel<decltype(fa)::value, decltype(fb)::value, std::decay_t<decltype(fo)>...>), dim3(blocks),
                           dim3(kBlock), 0, s, g, fo...);
    });
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_mx_conv2d(const uint8_t* x_elements, const uint8_t* x_scales, int x_format, const uint8_t* w_elements,
                                const uint8_t* w_scales, int w_format, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                                int64_t w, int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream) {
    return run_conv("mx_conv2d", x_elements, x_scales, x_format, w_elements, w_scales, w_format, bias, y, n, c, h, w, o, kh, kw, stride_h,
                    stride_w, pad_h, pad_w, dil_h, dil_w, nullptr, stream);
}

extern "C" int ppqhip_mx_conv2d_fused(const uint8_t* x_elements, const uint8_t* x_scales, int x_format, const uint8_t* w_elements,
                                      const uint8_t* w_scales, int w_format, const float* bias, const float* residual, int relu, float* y,
                                      uint8_t* out_elements, uint8_t* out_scales, int out_format, int64_t n, int64_t c, int64_t h,
                                      int64_t w, int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                      int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream) {
    const MxFusedHost fused = {residual, relu, out_elements, out_scales, out_format};
    return run_conv("mx_conv2d_fused", x_elements, x_scales, x_format, w_elements, w_scales, w_format, bias, y, n, c, h, w, o, kh, kw,
                    stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, &fused, stream);
}
