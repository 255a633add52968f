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
//
// ppqhip_conv1x1_epilogue (second half of this file): the same GEMM as a persistent launch whose store is the convolution's whole
// epilogue group -- bias, residual Add, ReLU -- and the calibration sinks of epilogue_sinks.hpp (min/max slots, histogram rows), so
// that in a calibration forward the raw convolution output is neither written nor read back.  The chain contract is untouched:
// the epilogue starts from the same accumulator, in epilogue.hip's operand order.  ppqhip_conv1x1 itself is as it was.
#include "common.hpp"
#include "epilogue_sinks.hpp"
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

// ---- the fused form: ppqhip_conv1x1_epilogue ------------------------------------------------------------------------------------
// The same GEMM (same K order, same padding, one accumulator element per output: the chain contract above holds unchanged), whose
// store is the convolution's whole epilogue group: bias, optional residual Add, optional ReLU and the calibration sinks of
// epilogue_sinks.hpp, fed from the accumulators.  The raw convolution output is never written and never read back.
//   FORM 0 (P1):  y = act(acc + bias_a[o])                                           sink: y
//   FORM 1 (P2b): xa = acc + bias_a[o];  r = resid + bias_b[o];  out = act(xa + r)   sinks: xa, r, out
//   FORM 2 (P2):  xa = acc + bias_a[o];  r = resid;              out = act(xa + r)   sinks: xa, out
// in epilogue.hip's operand order (epilogue_vec), every add rounded on its own.  Only y / out is stored.
// The sinks want one owner per slot / row and launch, so the kernel is persistent: at most kEpStatWgPerCu workgroups of
// kEpStatBlock lanes per CU (the shape epilogue.hip's sink launches have, and the one the observers' accumulators are sized
// for), eight waves as 2 x 4 over a 64 x 128 x 32 tile -- per wave the work of conv1x1_kernel.  Workgroup g walks a contiguous
// range of tiles, channel tiles fastest, and folds once, at its end, into slot / row g with a plain read-modify-write: no global
// atomics, nothing synchronises across workgroups, capturable into a HIP graph.  While a tile's stores and sink work drain, the
// first K step of the workgroup's next tile is already in flight; the residual is loaded ahead of the tile's last K step.
struct PwEpArgs {
    const float* bias_b; const float* resid;
    uint32_t tiles, relu;
};

template <int WM, int WN, int BK, bool VEC, int FORM, class SINKS>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN * 64 * kEpStatWgPerCu + 255) / 256)
void conv1x1_epilogue_kernel(const PwArgs g, const PwEpArgs e, const typename SINKS::Args sk) {
    static_assert(BK == 16 || BK == 32, "BK 16 or 32");
    constexpr int NT = WM * WN * 64;
    constexpr bool RESID = FORM != 0, BIAS_B = FORM == 1;
    constexpr int BM = WM * 32, BN = WN * 32, RS = BK + 4, HK = BK / 2, LW = VEC ? 4 : 1;
    constexpr int WL = BM * BK / (NT * LW), XL = BK * BN / (NT * LW);          // loads per thread and K tile
    constexpr int WROWS = NT * LW / BK, XROWS = NT * LW / BN;                 // rows of the tile one pass of the NT threads covers
    static_assert(BN / LW <= NT && WL >= 1 && XL >= 1, "tile too small / too wide for the loader");
    typedef float ldv __attribute__((ext_vector_type(LW)));
    __shared__ __attribute__((aligned(16))) float Ws[2][BM * RS];
    __shared__ __attribute__((aligned(16))) float Xs[2][BK * BN];
    __shared__ float Bs[2][2 * BM];                                            // bias_a, bias_b of the tile's rows, by tile parity
    extern __shared__ int sink_lds[];                                          // the sinks' 32 floats / histogram counters

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t tile, tile_end;
    even_split(e.tiles, gridDim.x, blockIdx.x, tile, tile_end);                // (the host: gridDim.x <= tiles)
    SINKS sinks;
    sinks.init(sk, sink_lds);

    // loader coordinates, as in conv1x1_kernel; (m0, q0, woff, xoff) are those of the tile being LOADED
    const uint32_t wk = (t % (BK / LW)) * LW, wm = t / (BK / LW);
    const uint32_t xc = (t % (BN / LW)) * LW, xk = t / (BN / LW);
    const uint32_t xstep = XROWS * g.in_plane;
    uint32_t m0, q0, woff[WL], xoff;
    float bpre = 0.0f;
    int par = 0;                                                               // parity of the tile being computed: its half of Bs
    auto setup = [&](uint32_t ti) {
        const uint32_t tq = fdiv(ti, g.div_tiles_m), tm = ti - tq * g.tiles_m;                   // channel tiles vary fastest
        m0 = tm * BM; q0 = tq * BN;
#pragma unroll
        for (int r = 0; r < WL; r++) woff[r] = min(m0 + wm + WROWS * r, g.o - 1u) * g.c + wk;
        const uint32_t qx = min(q0 + xc, g.q - LW);
        const uint32_t img = fdiv(qx, g.div_plane), p = qx - img * g.out_plane;
        uint32_t src = p;
        if (g.stride != 1u) { const uint32_t oh = fdiv(p, g.div_wo), ow = p - oh * g.div_wo.d; src = (oh * g.in_w + ow) * g.stride; }
        xoff = img * g.c * g.in_plane + src + xk * g.in_plane;
        // the tile's biases travel with its first K step: thread t < BM brings bias_a of row t, thread BM + t bias_b (rows past
        // the edge: the last one, computed with and dropped)
        if (t < 2 * BM) {
            const uint32_t row = min(m0 + (t & (BM - 1)), g.o - 1u);
            bpre = t < BM ? g.bias[row] : (BIAS_B ? e.bias_b[row] : 0.0f);
        }
    };
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
    const uint32_t row0 = (wave / WN) * 32, col0 = (wave % WN) * 32;
    const uint32_t tiles_k = (g.c + BK - 1) / BK;
    const bool relu = e.relu != 0;

    setup(tile);
    load_tile(0);
    sinks.begin();                                                // (its barrier waits for LDS only: the loads stay in flight)
    for (;;) {
        const uint32_t em0 = m0, eq0 = q0;                        // the tile being computed
        // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Rows and the column past
        // the edge are CLAMPED for the loads of the residual and the addresses of the stores (what they compute is dropped).
        const uint32_t qc = eq0 + col0 + i, rbase = em0 + row0 + 4 * h;
        const bool col_in = qc < g.q;
        const uint32_t qcl = min(qc, g.q - 1u);
        const uint32_t img = fdiv(qcl, g.div_plane), p = qcl - img * g.out_plane;
        const uint32_t ycol = img * g.o * g.out_plane + p;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;

        auto multiply = [&](int buf) {
            const float* ws = &Ws[buf][(row0 + i) * RS + h * HK];
            const float* xs = &Xs[buf][h * BN + col0 + i];
            float a[HK];
#pragma unroll
            for (int v = 0; v < HK / 4; v++) {
                const float4 f = *reinterpret_cast<const float4*>(ws + 4 * v);
                a[4 * v] = f.x; a[4 * v + 1] = f.y; a[4 * v + 2] = f.z; a[4 * v + 3] = f.w;
            }
#pragma unroll
            for (int s = 0; s < HK; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], xs[2 * s * BN], acc, 0, 0, 0);
        };
        store_tile(0);
        if (t < 2 * BM) Bs[par][t] = bpre;                        // read after the K loop's barriers; rewritten two tiles on
        __syncthreads();
        for (uint32_t kt = 0; kt + 1 < tiles_k; kt++) {
            const int buf = (int)(kt & 1u);
            load_tile((kt + 1) * BK);                             // in flight while this tile multiplies
            multiply(buf);
            store_tile(buf ^ 1);                                  // the buffer the PREVIOUS iteration read: everyone is past its barrier
            __syncthreads();
        }
        // the last K step (peeled), with the residual in flight while it multiplies
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; r++)
            rv[r] = RESID ? e.resid[ycol + min(rbase + (r & 3) + 8 * (r >> 2), g.o - 1u) * g.out_plane] : 0.0f;   // (as the stores)
        multiply((int)((tiles_k - 1) & 1u));
        __syncthreads();                                          // before the next tile's first store into buffer 0

        const bool next = tile + 1 < tile_end;                    // (workgroup uniform)
        const bool full = em0 + BM <= g.o && eq0 + BN <= g.q;     // (workgroup uniform) every lane holds 16 outputs
        const float* bs = &Bs[par][row0 + 4 * h];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // the next tile's first K step goes out behind the first half of this tile's epilogue: by then half of the
            // accumulators and of the residual are dead, and their registers hold the loads
            if (j == 2 && next) { setup(tile + 1); load_tile(0); }
            float va[4], vb[4], vo[4], ba[4], bb[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { ba[u] = bs[8 * j + u]; bb[u] = BIAS_B ? bs[BM + 8 * j + u] : 0.0f; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = 4 * j + u;
                const float xa = acc[r] + ba[u];
                if (!RESID) { va[u] = act(xa, relu); vb[u] = 0.0f; vo[u] = 0.0f; continue; }
                va[u] = xa;
                float rr = rv[r];
                if (BIAS_B) rr = rr + bb[u];
                vb[u] = rr;
                vo[u] = act(xa + rr, relu);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {                         // a tile is stored before it is handed to the sinks
                const uint32_t row = rbase + u + 8 * j;
                if (col_in && row < g.o) g.y[ycol + min(row, g.o - 1u) * g.out_plane] = RESID ? vo[u] : va[u];
            }
            if (full) {
                EpStored<float4> s4{};
                s4.a = make_float4(va[0], va[1], va[2], va[3]);
                if (BIAS_B) s4.b = make_float4(vb[0], vb[1], vb[2], vb[3]);
                if (RESID) s4.out = make_float4(vo[0], vo[1], vo[2], vo[3]);
                sinks.template feed4<true>(s4, true, j == 0);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    EpStored<float> s1{};
                    s1.a = va[u]; s1.b = vb[u]; s1.out = vo[u];
                    sinks.feed1(s1, col_in && rbase + u + 8 * j < g.o);
                }
            }
            __builtin_amdgcn_sched_barrier(0);                    // one row group at a time: interleaving the four costs registers
        }
        if (!next) break;
        tile++;
        par ^= 1;
    }
    sinks.finish(sk, blockIdx.x, sink_lds);
}

constexpr int kFWM = 2, kFWN = 4;                                  // the fused launch: 512 lanes = kEpStatBlock, a 64 x 128 x 32 tile
static_assert(kFWM * kFWN * 64 == kEpStatBlock, "the fused launch has the sink launches' workgroup");

template <int FORM, class SINKS>
void launch_fused(bool vec, uint32_t grid, uint32_t lds_bytes, hipStream_t s, const PwArgs& g, const PwEpArgs& e,
                  const typename SINKS::Args& sk) {
    if (vec) hipLaunchKernelGGL((conv1x1_epilogue_kernel<kFWM, kFWN, kBK, true, FORM, SINKS>), dim3(grid), dim3(kEpStatBlock), lds_bytes, s, g, e, sk);
    else hipLaunchKernelGGL((conv1x1_epilogue_kernel<kFWM, kFWN, kBK, false, FORM, SINKS>), dim3(grid), dim3(kEpStatBlock), lds_bytes, s, g, e, sk);
}

template <int FORM>
void launch_fused_hist(bool vec, uint32_t grid, hipStream_t s, const PwArgs& g, const PwEpArgs& e, const EpHistSinks& sk, int asym, int clip) {
    constexpr bool R = FORM != 0, B = FORM == 1;            // (the residual forms read their rows late: no registers to spare)
    const uint32_t lds = sk.lds_ints * (uint32_t)sizeof(int);
    switch ((asym ? 2 : 0) | (clip ? 1 : 0)) {
        case 0: launch_fused<FORM, EpHistSet<R, B, false, false, kEpStatBlock, !R>>(vec, grid, lds, s, g, e, sk); break;
        case 1: launch_fused<FORM, EpHistSet<R, B, false, true, kEpStatBlock, !R>>(vec, grid, lds, s, g, e, sk); break;
        case 2: launch_fused<FORM, EpHistSet<R, B, true, false, kEpStatBlock, !R>>(vec, grid, lds, s, g, e, sk); break;
        default: launch_fused<FORM, EpHistSet<R, B, true, true, kEpStatBlock, !R>>(vec, grid, lds, s, g, e, sk); break;
    }
}

int refuse(const char* what, const char* why) {
    set_error("%s: %s", what, why);
    return PPQHIP_ERR_INVALID_VALUE;
}

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

extern "C" int ppqhip_conv1x1_epilogue(const float* x, const float* w, const float* bias_a, const float* resid, const float* bias_b,
                                       float* out, int64_t n, int64_t c, int64_t h, int64_t wd, int64_t o, int64_t stride, int relu,
                                       int sink_kind, void* dst_a, void* dst_r, void* dst_out, float p0_a, float p1_a, float p0_r,
                                       float p1_r, float p0_out, float p1_out, int64_t num_bins, int asymmetric, int clip_outliers,
                                       int64_t max_workgroups, void* stream) {
    const char* what = "conv1x1_epilogue";
    constexpr int64_t kMax = 2147483647;
    if (n < 0 || c <= 0 || h <= 0 || wd <= 0 || o <= 0) return refuse(what, "non-positive size");
    if (stride != 1 && stride != 2) { set_error("%s: stride must be 1 or 2", what); return PPQHIP_ERR_UNSUPPORTED; }
    if (max_workgroups < 0) return refuse(what, "max_workgroups is negative");
    if (sink_kind != PPQHIP_SINK_NONE && sink_kind != PPQHIP_SINK_MINMAX && sink_kind != PPQHIP_SINK_HIST)
        return refuse(what, "unknown sink kind");
    if (n == 0) return PPQHIP_OK;
    if (x == nullptr || w == nullptr || bias_a == nullptr || out == nullptr) return refuse(what, "null pointer");
    if (resid == nullptr && bias_b != nullptr) return refuse(what, "bias_b without a residual");
    const int64_t ho = (h - 1) / stride + 1, wo = (wd - 1) / stride + 1;
    if (n > kMax || c > kMax || h > kMax || wd > kMax || o > kMax || (double)n * (double)c * (double)h * (double)wd > (double)kMax
        || (double)n * (double)o * (double)ho * (double)wo > (double)kMax || (double)o * (double)c > (double)kMax)
        return refuse(what, "more than 2^31 - 1 elements in x, w or out");
    // the sinks: P1 has one tensor, `out`; the residual is a tensor of its own (the biased r) only with bias_b
    if (resid == nullptr && (dst_a != nullptr || dst_r != nullptr)) return refuse(what, "without a residual only out has a sink");
    if (bias_b == nullptr && dst_r != nullptr) return refuse(what, "without bias_b, the residual is only read: it has no sink");
    const bool hist = sink_kind == PPQHIP_SINK_HIST, minmax = sink_kind == PPQHIP_SINK_MINMAX;
    if (hist && (num_bins <= 0 || num_bins > kMax)) return refuse(what, "histogram is empty or too large");
    // a workgroup reads its slot / row of every sink and writes it back at the end: two sinks on one accumulator would lose counts
    if ((dst_a && (dst_a == dst_r || dst_a == dst_out)) || (dst_r && dst_r == dst_out)) return refuse(what, "two sinks share one accumulator");
    const int64_t ny = n * o * ho * wo;
    std::vector<Span> ins, outs;
    ins.push_back(span_of(x, n * c * h * wd)); ins.push_back(span_of(w, o * c)); ins.push_back(span_of(bias_a, o));
    if (resid != nullptr) ins.push_back(span_of(resid, ny));
    if (bias_b != nullptr) ins.push_back(span_of(bias_b, o));
    outs.push_back(span_of(out, ny));
    if (int st = check_overlap(what, ins, outs)) return st;

    // nothing is wrong from here on, but the kernel may have no path: PPQHIP_NOT_FUSED before anything is written
    if (!aligned4(x) || !aligned4(w) || !aligned4(bias_a) || !aligned4(resid) || !aligned4(bias_b) || !aligned4(out)) return PPQHIP_NOT_FUSED;
    if (!(minmax || hist) || (dst_a == nullptr && dst_r == nullptr && dst_out == nullptr)) return PPQHIP_NOT_FUSED;   // the plain forms: ppqhip_conv1x1
    void* dst[3] = {resid ? dst_a : dst_out, dst_r, resid ? dst_out : nullptr};          // the sets' order: a (P1: y), b, out
    EpMinMaxSinks mm{};
    EpHistSinks hs{};
    if (minmax) for (int k = 0; k < 3; k++) mm.slots[k] = static_cast<float*>(dst[k]);
    if (hist) {
        const float p0[3] = {resid ? p0_a : p0_out, p0_r, p0_out}, p1[3] = {resid ? p1_a : p1_out, p1_r, p1_out};
        hs.bins = (int)num_bins;
        uint64_t ints = 0;
        for (int k = 0; k < 3; k++) {
            hs.rows[k] = static_cast<int*>(dst[k]);
            if (asymmetric) { hs.a0[k] = p0[k]; hs.hs[k] = (p1[k] - p0[k]) / (float)hs.bins; }
            else { hs.a0[k] = 0.f; hs.hs[k] = p0[k]; }
            hs.lds_off[k] = (uint32_t)ints;
            if (hs.rows[k]) ints += (uint64_t)num_bins;
        }
        if (ints > kEpHistLdsInts) return PPQHIP_NOT_FUSED;                              // the counters do not fit
        hs.lds_ints = (uint32_t)ints;
    }

    PwArgs g;
    g.x = x; g.w = w; g.bias = bias_a; g.y = out;
    g.c = (uint32_t)c; g.o = (uint32_t)o; g.q = (uint32_t)(n * ho * wo);
    g.in_plane = (uint32_t)(h * wd); g.out_plane = (uint32_t)(ho * wo); g.in_w = (uint32_t)wd; g.stride = (uint32_t)stride;
    g.div_plane = make_fastdiv(g.out_plane); g.div_wo = make_fastdiv((uint32_t)wo);
    const bool vec = stride == 1 && g.out_plane % 4u == 0 && c % 4 == 0 && aligned16(x) && aligned16(w);
    constexpr uint32_t BM = kFWM * 32, BN = kFWN * 32;
    g.tiles_m = (g.o + BM - 1) / BM;
    g.div_tiles_m = make_fastdiv(g.tiles_m);
    PwEpArgs e;
    e.bias_b = bias_b; e.resid = resid; e.relu = relu ? 1u : 0u;
    e.tiles = g.tiles_m * ((g.q + BN - 1) / BN);
    uint32_t grid = (uint32_t)(num_cu() * kEpStatWgPerCu);                                // one slot / row per workgroup
    if (grid > e.tiles) grid = e.tiles;
    if (max_workgroups > 0 && (int64_t)grid > max_workgroups) grid = (uint32_t)max_workgroups;
    hipStream_t s = (hipStream_t)stream;
    const int form = resid == nullptr ? 0 : bias_b != nullptr ? 1 : 2;
    if (minmax) {
        const uint32_t lds = 32 * sizeof(float);
        if (form == 0) launch_fused<0, EpMinMaxSet<false, false>>(vec, grid, lds, s, g, e, mm);
        else if (form == 1) launch_fused<1, EpMinMaxSet<true, true>>(vec, grid, lds, s, g, e, mm);
        else launch_fused<2, EpMinMaxSet<true, false>>(vec, grid, lds, s, g, e, mm);
    } else {
        if (form == 0) launch_fused_hist<0>(vec, grid, s, g, e, hs, asymmetric, clip_outliers);
        else if (form == 1) launch_fused_hist<1>(vec, grid, s, g, e, hs, asymmetric, clip_outliers);
        else launch_fused_hist<2>(vec, grid, s, g, e, hs, asymmetric, clip_outliers);
    }
    return finish_launch(what);
}
