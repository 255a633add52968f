// int8_gconv.hip -- a grouped linear INT8 convolution (1 < groups < C, or a depthwise layer with a channel multiplier) as an integer
// backend runs it, on v_mfma_i32_16x16x32_i8.  The contract is DESIGN.md sections 9.22 / 9.25 and tests/int8_grouped_reference.py:
// that of int8_conv.hpp with the sum of output o running over the C_g * kh * kw inputs of o's OWN group only, so the result has the
// bits of ppqhip_int8_conv2d on the block-diagonal dense weight -- at 1 / groups of its MFMA work, weight bytes and gathers.
//
// Why the dense frame does not take a group offset: its workgroup owns 64 x 64 outputs and its two wave columns share one A stage; in
// a grouped layer two wave columns generally belong to different groups and need different input channels.  So the tile is the
// frame's other shape (int8_tile.hpp, NA = 4): 128 pixel rows x ONE slice of 32 columns, the four waves stacked along M, all reading
// the same 32 staged rows of B and their own 32 rows of A.  q8_start, q8_chunk, q8_k_loop and q8_epilogue are those of the family.
//
// Slices.  Slice s is the outputs 32 s .. 32 s + 31, wherever the group borders are.  It needs the input channels of the groups
// floor(32 s / O_g) .. floor(min(32 s + 31, O - 1) / O_g); rounded outwards to blocks of 32 channels these are the blocks
// cb0[s] .. cb0[s] + nbs - 1, nbs the largest such count over the slices (one number per layer), cb0 an int32 table [ceil(O / 32)] made
// where the weight is packed.
//
// Operands: x [N, H, W, Cp] as int8_conv.hpp takes it, Cp = 32 nbc.  w [O, kh, kw, 32 nbs]: block j of a tap of row o holds the codes
// of w[o] for the channels 32 (cb0[o / 32] + j) .. + 31 -- the row's own group's channels in their places; a channel of another group,
// a channel at or past C and a block at or past nbc are code 0.  A row of the implicit GEMM has nb = kh kw nbs blocks ordered
// (ky, kx, j).  For block (tap, j) a thread gathers channel block min(cb0[s] + j, nbc - 1) of the tap's input pixel, exactly as
// ConvA of int8_conv.hpp gathers (a tap in the padding: the byte zx, no load); whatever A holds where the weight is 0 does not reach
// the sum, and sums[o], the sum of the row's codes, keeps the zero-point start -zx * sums[o] right.  The clamp keeps every load inside
// x whatever the table holds.
//
// Per chunk of 4 blocks a thread stages four 16-byte segments of A (rows t >> 3 + 32 h) and one of B (row t >> 3 of the slice):
// 128 x 144 + 32 x 144 = 23040 bytes a buffer, 46080 for the double buffer (derived from the layout, not measured); the waves' code
// stages take the first buffer once it is dead, as in q8_tile.
//
// Grid (derived, not measured): ceil(M / 128) x ceil(O / 32) workgroups, the slice the FAST index.  A pixel of x is Cp contiguous
// bytes and a slice reads 32 nbs of them: with nbs = 1 four consecutive slices read the four quarters of the same 128-byte lines, and
// the 16 consecutive workgroups of a ResNeXt row tile (C = 512) together read every line of their 128 x kh x kw pixels once while it
// is fresh in L2; the rows of q (op bytes) are shared by four slices in the same way and a row of y by all of them.  What consecutive
// workgroups would share the other way round is a slice's weight, 32 x nb x 32 bytes (9 KiB at 3 x 3, nbs = 1): small enough to stay
// in L2 for the whole launch whichever way the grid runs.
#include "int8_conv.hpp"

using namespace ppqhip;

namespace ppqhip {

constexpr int kGcNA = 4;                          // 128 rows x 32 columns per workgroup
using GcB = Q8B8Rows<1>;                          // the slice's 32 rows of w, one 16-byte segment per thread and chunk

struct Int8GConvArgs {
    Int8ConvArgs g;                               // w: [o, nb * 32]; nb = kh * kw * nbs; nbc: the channel blocks of x; fnbc divides by nbs
    const int32_t* cb0;                           // [ceil(o / 32)]: the first channel block of a slice
    uint32_t nbs;                                 // channel blocks per tap of a row of w
};

// Where a thread's share of a chunk lies: B by the codec's map on the slice's rows, A by ConvA on the slice's channel blocks.
struct GConvMap {
    const Int8GConvArgs& p;
    ConvA<kGcNA> a;
    uint32_t first;                               // cb0 of the workgroup's slice
    GcB::Map bmap;

    __device__ __forceinline__ GConvMap(const Int8GConvArgs& args, uint32_t row0, uint32_t col0, uint32_t t)
        : p(args), a(args.g, row0, t), first((uint32_t)args.cb0[col0 / kQ8Cols<kGcNA>]), bmap(args.g.w, args.g.nb, args.g.e.n, col0, t) {}

    template <bool TAIL>
    __device__ __forceinline__ void load(uint32_t kb0, Q8Staged<GcB, kGcNA>& st) const {
        uint32_t kb = kb0 + (a.seg >> 1);
        if (TAIL) kb = min(kb, p.g.nb - 1u);                                     // a dead block: a live one's bytes, never multiplied
        const uint32_t tap = fdiv(kb, p.g.fnbc);
        a.load(tap, min(first + (kb - tap * p.nbs), p.g.nbc - 1u), st.a);        // past x's last block: the weight there is 0
        bmap.template load<TAIL>(kb0, st.b);
    }

    __device__ __forceinline__ void store(uint8_t* buf, const Q8Staged<GcB, kGcNA>& st) const { q8_store_staged<GcB, kGcNA>(buf, a.lds_e, bmap, st); }
};

__global__ __launch_bounds__(kBlock) void q8_gconv_kernel(const Int8GConvArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kQ8BufBytes<GcB, kGcNA>];
    q8_tile<GcB, kGcNA>(p.g.e, p.g.nb, stage, [&p](uint32_t row0, uint32_t col0, uint32_t t) { return GConvMap(p, row0, col0, t); });
}

}  // namespace ppqhip

extern "C" int ppqhip_int8_gconv2d(const int8_t* x, const int8_t* w, const int32_t* w_sums, int zx, const float* mul, const float* bias,
                                   const float* residual, int relu, float* y, int8_t* q, float sy, int zy, int qmin, int qmax, int rounding,
                                   int q_nan, int64_t n, int64_t c, int64_t h, int64_t wd, int64_t o, int64_t kh, int64_t kw,
                                   int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w,
                                   int64_t groups, int64_t nbs, const int32_t* cb0, void* stream) {
    const char* what = "int8_gconv2d";
    const Int8TailHost t = {w_sums, zx, mul, bias, residual, relu, y, q, sy, zy, qmin, qmax, rounding, q_nan};
    if (int st = check_int8_tail(what, "y", t)) return st;
    ConvShape z = {n, c, h, wd, o, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
    if (int st = check_conv_shape(what, z, {groups, nbs})) return st;
    if (groups < 1) { set_error("%s: groups must be at least 1, got %lld", what, (long long)groups); return PPQHIP_ERR_INVALID_VALUE; }
    if (c % groups != 0 || o % groups != 0) {
        set_error("%s: c = %lld and o = %lld must both be multiples of groups = %lld", what, (long long)c, (long long)o, (long long)groups);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    if (nbs < 1) { set_error("%s: nbs must be at least 1, got %lld", what, (long long)nbs); return PPQHIP_ERR_INVALID_VALUE; }
    if (cb0 == nullptr) { set_error("%s: null pointer", what); return PPQHIP_ERR_INVALID_VALUE; }
    Int8GConvArgs p;
    p.cb0 = cb0; p.nbs = (uint32_t)nbs;
    const int64_t slices = (o + kQ8Cols<kGcNA> - 1) / kQ8Cols<kGcNA>;
    return launch_q8_conv<GcB, kGcNA>(what, K_INT8_GCONV, x, w, t, z, nbs, {span_of(cb0, slices)}, stream, p.g, [&p](uint32_t blocks, hipStream_t s) {
        hipLaunchKernelGGL(q8_gconv_kernel, dim3(blocks), dim3(kBlock), 0, s, p);
    });
}
