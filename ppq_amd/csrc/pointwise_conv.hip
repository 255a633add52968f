// pointwise_conv.hip -- ppqhip_conv1x1: the 1x1 convolutions of a contiguous NCHW float32 network as ONE native GEMM launch on the
// FP32-input MFMA (v_mfma_f32_32x32x2_f32), no layout transposes, no im2col.
//
// Per call  Y[o, q] = sum_k W[o, k] X[k, q]  with the columns q = (image, output pixel) of the WHOLE batch flattened into one axis:
// a column's address is  x + image * c * h * w + src(pixel) + k * h * w,  so the only thing a stride-2 `down` convolution, an odd
// plane (7x7 = 49) or a plane that is no multiple of the tile changes is the per-column offset, which a thread computes once before
// its K loop.  Where stride is 1, planes and c are multiples of 4 and x / w are 16-byte aligned the loads are 16 bytes wide (VEC);
// everything else (7x7 planes, stride 2, odd channel counts) takes the same kernel with dword loads.
//
// Arithmetic contract (include/ppq_hip.h): y[n, o, p] is the float32 fmaf chain over k = 0 .. c - 1 in ascending order from +0, the
// bias is added afterwards with one more rounding.  What keeps that true here:
//   * one accumulator element per output for the whole K loop: no split-K, no atomics, no reassociation;
//   * MFMA step s of a K tile multiplies k = 2 s (lanes 0-31) and k = 2 s + 1 (lanes 32-63), in that order (the instruction's own
//     k order), steps and tiles ascending;
//   * the only padding is k >= c inside the last K tile, as W = -0, X = +0: fmaf(-0, +0, acc) == acc for EVERY acc, -0 included
//     (a +0 * +0 pad would turn an accumulated -0 into +0); rows >= o and columns >= q multiply real data and are never stored;
//   * -ffp-contract=off keeps `acc + bias` a separate, rounded add.
// So a result's bits depend on w[o, :], x[n, :, src(p)] and bias[o] only: not on the tile shape, the grid, n or p.
#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PwArgs {
    const float* x; const float* w; const float* bias; float* y;
    uint32_t c, o, q;                      // input channels, output channels, columns = n * ho * wo
    uint32_t in_plane, out_plane;          // h * w, ho * wo
    uint32_t in_w, stride;
    uint32_t tiles_m;
    FastDiv div_plane, div_wo, div_tiles_m;
};

// Workgroup = 4 waves as WM x WN, each wave TM x TN accumulator tiles of 32 x 32: block tile BM (channels) x BN (columns) x BK.
// LDS, two buffers each:  Ws[BM][BK + 4]: row m holds its even k first, then its odd k (lane half h of MFMA step s reads
//                         k = 2 s + h: BK / 2 contiguous floats per lane, ds_read_b128, rows 16-B aligned and conflict-free at
//                         a stride of 20 / 36 dwords);  Xs[BK][BN]: as in memory, 32 consecutive columns per ds_read_b32 group.
// VEC: 16-byte global loads (stride 1, planes and c multiples of 4, x and w 16-B aligned); otherwise one dword per load.
// The K loop's loads carry no bounds test: a thread whose weight row or column lies past the edge reads the LAST valid one instead
// (its products land in accumulator rows / columns that are never stored), and only the final, partial K tile pads (W = -0, X = +0).
template <int WM, int WN, int TM, int TN, int BK, bool VEC>
__global__ __launch_bounds__(256) void conv1x1_kernel(const PwArgs g) {
    static_assert(WM * WN == 4 && (BK == 16 || BK == 32), "4 waves; BK 16 or 32");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32, RS = BK + 4, HK = BK / 2, LW = VEC ? 4 : 1;
    constexpr int WL = BM * BK / (256 * LW), XL = BK * BN / (256 * LW);        // loads per thread and K tile
    constexpr int WROWS = 256 * LW / BK, XROWS = 256 * LW / BN;               // rows of the tile one pass of the 256 threads covers
    static_assert(BN / LW <= 256 && WL >= 1 && XL >= 1, "tile too small / too wide for the loader");
    typedef float ldv __attribute__((ext_vector_type(LW)));
    __shared__ __attribute__((aligned(16))) float Ws[2][BM * RS];
    __shared__ __attribute__((aligned(16))) float Xs[2][BK * BN];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t tq = fdiv(blockIdx.x, g.div_tiles_m), tm = blockIdx.x - tq * g.tiles_m;      // channel tiles vary fastest: the
    const uint32_t m0 = tm * BM, q0 = tq * BN;                                                   // blocks of one column tile run together

    // loader coordinates: this thread's k (first of LW) of its weight rows, and its ONE column (first of LW) of x
    const uint32_t wk = (t % (BK / LW)) * LW, wm = t / (BK / LW);
    const uint32_t xc = (t % (BN / LW)) * LW, xk = t / (BN / LW);
    uint32_t woff[WL], xoff;
#pragma unroll
    for (int r = 0; r < WL; r++) woff[r] = min(m0 + wm + WROWS * r, g.o - 1u) * g.c + wk;
    {
        const uint32_t qx = min(q0 + xc, g.q - LW);
        const uint32_t img = fdiv(qx, g.div_plane), p = qx - img * g.out_plane;
        uint32_t src = p;
        if (g.stride != 1u) { const uint32_t oh = fdiv(p, g.div_wo), ow = p - oh * g.div_wo.d; src = (oh * g.in_w + ow) * g.stride; }
        xoff = img * g.c * g.in_plane + src + xk * g.in_plane;
    }
    const uint32_t xstep = XROWS * g.in_plane;
    ldv wr[WL], xr[XL];
    auto load_tile = [&](uint32_t k0) {
        if (k0 + BK <= g.c) {                                   // (uniform) a whole K tile
#pragma unroll
            for (int r = 0; r < WL; r++) wr[r] = *reinterpret_cast<const ldv*>(g.w + (woff[r] + k0));
            const float* xp = g.x + (xoff + k0 * g.in_plane);
#pragma unroll
            for (int r = 0; r < XL; r++) xr[r] = *reinterpret_cast<const ldv*>(xp + r * xstep);
        } else {                                                // the last, partial one (c % 4 == 0 under VEC: a vector is in or out)
#pragma unroll
            for (int r = 0; r < WL; r++) {
                ldv pad = -0.0f;
                wr[r] = (k0 + wk < g.c) ? *reinterpret_cast<const ldv*>(g.w + (woff[r] + k0)) : pad;
            }
#pragma unroll
            for (int r = 0; r < XL; r++) {
                ldv pad = 0.0f;
                xr[r] = (k0 + xk + XROWS * r < g.c) ? *reinterpret_cast<const ldv*>(g.x + (xoff + k0 * g.in_plane + r * xstep)) : pad;
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int r = 0; r < WL; r++) {
            float* row = &Ws[buf][(wm + WROWS * r) * RS];
            if constexpr (VEC) {
                *reinterpret_cast<float2*>(row + (wk >> 1)) = make_float2(wr[r][0], wr[r][2]);           // even k
                *reinterpret_cast<float2*>(row + HK + (wk >> 1)) = make_float2(wr[r][1], wr[r][3]);      // odd k
            } else {
                row[(wk & 1u) * HK + (wk >> 1)] = wr[r][0];
            }
        }
#pragma unroll
        for (int r = 0; r < XL; r++) *reinterpret_cast<ldv*>(&Xs[buf][(xk + XROWS * r) * BN + xc]) = xr[r];
    };

    const uint32_t i = lane & 31u, h = lane >> 5;
    const uint32_t row0 = (wave / WN) * (TM * 32), col0 = (wave % WN) * (TN * 32);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int mt = 0; mt < TM; mt++)
#pragma unroll
        for (int nt = 0; nt < TN; nt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][nt][r] = 0.0f;

    const uint32_t tiles_k = (g.c + BK - 1) / BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (uint32_t kt = 0; kt < tiles_k; kt++) {
        const int buf = (int)(kt & 1u);
        const bool more = kt + 1 < tiles_k;
        if (more) load_tile((kt + 1) * BK);                       // in flight while this tile multiplies
        const float* ws = &Ws[buf][(row0 + i) * RS + h * HK];
        const float* xs = &Xs[buf][h * BN + col0 + i];
        float a[TM][HK];
#pragma unroll
        for (int mt = 0; mt < TM; mt++)
#pragma unroll
            for (int v = 0; v < HK / 4; v++) {
                const float4 f = *reinterpret_cast<const float4*>(ws + mt * 32 * RS + 4 * v);
                a[mt][4 * v] = f.x; a[mt][4 * v + 1] = f.y; a[mt][4 * v + 2] = f.z; a[mt][4 * v + 3] = f.w;
            }
#pragma unroll
        for (int s = 0; s < HK; s++) {
            float b[TN];
#pragma unroll
            for (int nt = 0; nt < TN; nt++) b[nt] = xs[2 * s * BN + nt * 32];
#pragma unroll
            for (int mt = 0; mt < TM; mt++)
#pragma unroll
                for (int nt = 0; nt < TN; nt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][s], b[nt], acc[mt][nt], 0, 0, 0);
        }
        if (more) store_tile(buf ^ 1);                            // the buffer the PREVIOUS iteration read: everyone is past its barrier
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): 32 lanes store 128 B along p
    const bool has_bias = g.bias != nullptr;
    float bv[TM][16];                                             // this lane's 16 rows of every row tile: loaded once, ahead of the stores
#pragma unroll
    for (int mt = 0; mt < TM; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++)
            bv[mt][r] = has_bias ? g.bias[min(m0 + row0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, g.o - 1u)] : 0.0f;
#pragma unroll
    for (int nt = 0; nt < TN; nt++) {
        const uint32_t qc = q0 + col0 + nt * 32 + i;
        if (qc >= g.q) continue;
        const uint32_t img = fdiv(qc, g.div_plane), p = qc - img * g.out_plane;
        float* yc = g.y + (img * g.o * g.out_plane + p);
#pragma unroll
        for (int mt = 0; mt < TM; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t row = m0 + row0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= g.o) continue;
                float v = acc[mt][nt][r];
                if (has_bias) v = v + bv[mt][r];                  // (never `+ 0` without a bias: -0 would become +0)
                yc[row * g.out_plane] = v;
            }
    }
}

// The one tile that is instantiated: 64 x 64 x 32, four waves of one 32 x 32 accumulator each.  Measured against 128 x 128 x 16 and
// 64 x 128 x 32 (2 x 2 / 1 x 2 accumulators per wave) and 64 x 128 / 32 x 128 as 1 x 4 waves on all 14 pointwise shape classes of
// ResNet-50 at batch 32, it was the fastest or within 1 % of it on every one (profiles/r18_pointwise_conv.txt): these layers have
// K = 64 .. 2048 and grids of 200 .. 3136 such tiles on 256 CUs, so per-workgroup prologue / epilogue and the last partial round of
// workgroups weigh more than the loads a larger tile saves.
constexpr int kWM = 2, kWN = 2, kTM = 1, kTN = 1, kBK = 32;

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" int ppqhip_conv1x1(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t wd,
                              int64_t o, int64_t stride, void* stream) {
    const char* what = "conv1x1";
    constexpr int64_t kMax = 2147483647;
    if (n < 0 || c <= 0 || h <= 0 || wd <= 0 || o <= 0) { set_error("%s: non-positive size", what); return PPQHIP_ERR_INVALID_VALUE; }
    if (stride != 1 && stride != 2) { set_error("%s: stride must be 1 or 2", what); return PPQHIP_ERR_UNSUPPORTED; }
    if (n == 0) return PPQHIP_OK;
    if (x == nullptr || w == nullptr || y == nullptr) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    const int64_t ho = (h - 1) / stride + 1, wo = (wd - 1) / stride + 1;
    if (n > kMax || c > kMax || h > kMax || wd > kMax || o > kMax || (double)n * (double)c * (double)h * (double)wd > (double)kMax
        || (double)n * (double)o * (double)ho * (double)wo > (double)kMax || (double)o * (double)c > (double)kMax) {
        set_error("%s: more than 2^31 - 1 elements in x, w or y", what); return PPQHIP_ERR_INVALID_VALUE;
    }
    std::vector<Span> ins, outs;
    ins.push_back(span_of(x, n * c * h * wd)); ins.push_back(span_of(w, o * c));
    if (bias != nullptr) ins.push_back(span_of(bias, o));
    outs.push_back(span_of(y, n * o * ho * wo));
    if (int st = check_overlap(what, ins, outs)) return st;
    if (!aligned4(x) || !aligned4(w) || !aligned4(y) || !aligned4(bias)) return PPQHIP_NOT_FUSED;

    PwArgs g;
    g.x = x; g.w = w; g.bias = bias; g.y = y;
    g.c = (uint32_t)c; g.o = (uint32_t)o; g.q = (uint32_t)(n * ho * wo);
    g.in_plane = (uint32_t)(h * wd); g.out_plane = (uint32_t)(ho * wo); g.in_w = (uint32_t)wd; g.stride = (uint32_t)stride;
    g.div_plane = make_fastdiv(g.out_plane); g.div_wo = make_fastdiv((uint32_t)wo);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = stride == 1 && g.out_plane % 4u == 0 && c % 4 == 0 && aligned16(x) && aligned16(w);
    constexpr uint32_t BM = kWM * kTM * 32, BN = kWN * kTN * 32;
    g.tiles_m = (g.o + BM - 1) / BM;
    g.div_tiles_m = make_fastdiv(g.tiles_m);
    const dim3 grid(g.tiles_m * ((g.q + BN - 1) / BN));
    if (vec) hipLaunchKernelGGL((conv1x1_kernel<kWM, kWN, kTM, kTN, kBK, true>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((conv1x1_kernel<kWM, kWN, kTM, kTN, kBK, false>), grid, dim3(256), 0, s, g);
    return finish_launch(what);
}
