// floating.hip -- low-precision float (FP8 E4M3 / E5M2 / generic E,M) fake-quant for gfx950.
//
// Replaces ppq/csrc/cuda/floating.cu; the scalar algorithm restates QuantizeScalarFloating
// (ppq/csrc/cuda/common.cuh:154-226) bit for bit, including its quirk that an exact mantissa tie
// under ROUND_HALF_EVEN rounds toward zero (nearbyint(0.5) == 0), which is NOT IEEE / OCP RNE --
// so the hardware v_cvt_pk_fp8_f32 conversions are deliberately not used here.
// The walks (tiles, element-wise fallback, backward rows, finish sum) are fq_walk.hpp's, shared with linear.hip; this file
// holds the format, its arithmetic, the scale search and the entry points.
#include "fq_walk.hpp"

namespace ppqhip {

struct FloatFmt {
    float hi, lo;          // min(clip_max, theoretical_max), max(clip_min, -theoretical_max)
    float clip_min, clip_max;
    int exponent_min_p1;   // exponent_min + 1
    float min_subnormal;
    int mantissa;
    // fast path (quant_float_rne_pow2)
    uint32_t half_m1;      // (1 << (22 - mantissa)) - 1: added to |u|'s pattern, a carry out of the dropped bits <=> they exceed one half
    uint32_t keep;         // ~((1 << (23 - mantissa)) - 1)
    uint32_t sub_limit;    // patterns of |u| below this take the subnormal branch: (exponent_min + 1 + 127) << 23
    float sub_scale;       // 1 / min_subnormal (a power of two)
};

static int make_fmt(int exponent, int mantissa, float clip_min, float clip_max, FloatFmt* f, const char* what) {
    if (exponent <= 0 || exponent > 8 || mantissa < 0 || mantissa > 23) {
        set_error("%s: unsupported float format E%dM%d", what, exponent, mantissa);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    const int sub_shift = (1 << (exponent - 1)) + mantissa - 2;
    if (sub_shift < 0 || sub_shift > 30) {
        // `1 << sub_shift` overflows int in the reference (common.cuh:210): undefined there.
        set_error("%s: E%dM%d needs 1 << %d, which the reference cannot represent", what, exponent, mantissa,
                  sub_shift);
        return PPQHIP_ERR_UNSUPPORTED;
    }
    const int exponent_min = -(1 << (exponent - 1)) + 1;
    const int exponent_max = (1 << (exponent - 1));
    union { float v; uint32_t d; } h;
    h.d = (uint32_t)((exponent_max + 127) << 23) + (uint32_t)(~(0x007FFFFF >> mantissa) & 0x007FFFFF);
    const float theo = h.v;
    f->hi = clip_max < theo ? clip_max : theo;
    f->lo = clip_min > -theo ? clip_min : -theo;
    f->clip_min = clip_min; f->clip_max = clip_max;
    f->exponent_min_p1 = exponent_min + 1;
    f->min_subnormal = 1.0f / (float)(1 << sub_shift);
    f->mantissa = mantissa;
    f->half_m1 = mantissa <= 22 ? (1u << (22 - mantissa)) - 1u : 0u;
    f->keep = mantissa <= 22 ? ~((1u << (23 - mantissa)) - 1u) : 0xFFFFFFFFu;
    f->sub_limit = (uint32_t)(exponent_min + 1 + 127) << 23;
    f->sub_scale = (float)(1 << sub_shift);
    return PPQHIP_OK;
}

// QuantizeScalarFloating, common.cuh:154-226 (the format-dependent constants are hoisted into fmt)
template <int R>
__device__ __forceinline__ float quant_float_scalar(float value, float scale, const FloatFmt& fmt, int rounding) {
    const float u = value / scale;
    if (u > fmt.hi) return fmt.hi;
    if (u < fmt.lo) return fmt.lo;
    const uint32_t bits = __float_as_uint(u);
    const uint32_t sign = bits & 0x80000000u;
    const int32_t exp = (int32_t)(bits & 0x7F800000u);
    const uint32_t man = bits & 0x007FFFFFu;
    if (((exp >> 23) - 127) < fmt.exponent_min_p1) {
        const float t = u / fmt.min_subnormal;
        const int r = (R >= 0) ? round2int_t<(R >= 0 ? R : 0)>(t) : round2int(t, rounding);
        return (float)r * fmt.min_subnormal;
    }
    const float frac = __uint_as_float(((man << fmt.mantissa) & 0x007FFFFFu) + 0x3F800000u) - 1;
    const uint32_t round_bit = (uint32_t)((R >= 0) ? round2int_t<(R >= 0 ? R : 0)>(frac) : round2int(frac, rounding));
    const uint32_t m = ((man >> (23 - fmt.mantissa)) + round_bit) << (23 - fmt.mantissa);
    const float v = __uint_as_float(sign + m + (uint32_t)exp);
    return v > fmt.clip_max ? fmt.clip_max : (v < fmt.clip_min ? fmt.clip_min : v);
}

// The same function for the case every shipped FP8 configuration is in -- ROUND_HALF_EVEN and a power-of-two scale
// (FP8Quantizer.py:99,196; the `floating` observer picks from {2^-7 .. 64}, observer/floating.py:97) -- without the two
// IEEE divisions and the data-dependent branches, bit for bit (tests: all 2^32 input patterns):
//   * value / 2^e == value * 2^-e (one exact scaling, rounded once either way; NaN payloads, infinities, underflow alike);
//     u / min_subnormal likewise (min_subnormal = 2^-k);
//   * round2int(frac) under HALF_EVEN with frac in [0, 1) is 1 iff the dropped mantissa bits exceed one half (a tie goes
//     to 0 = the reference's round-toward-zero-on-ties quirk), i.e. a carry out of `dropped + half - 1`; adding on the
//     whole magnitude pattern lets the carry run into the exponent exactly as `sign + m + exp` does (also for the
//     all-ones NaN pattern, where both wrap through the sign bit: hence `+ sign`, not `| sign`);
//   * (float)(int)rint(t) == rint(t) + 0.0f for |t| < 2^31 (the int round trip only loses the sign of a zero).
__device__ __forceinline__ uint32_t pow2_reciprocal_bits(float s) {        // 0 when s is not 2^e with 2^-e normal too
    const uint32_t b = __float_as_uint(s), e = b >> 23;
    return ((b & 0x807FFFFFu) == 0u && e >= 1u && e <= 253u) ? ((254u - e) << 23) : 0u;
}
__device__ __forceinline__ float quant_float_rne_pow2(float value, float rcp, const FloatFmt& fmt) {
    const float u = value * rcp;
    const uint32_t bits = __float_as_uint(u), sign = bits & 0x80000000u, mag = bits & 0x7FFFFFFFu;
    float vn = __uint_as_float(((mag + fmt.half_m1) & fmt.keep) + sign);
    vn = vn > fmt.clip_max ? fmt.clip_max : (vn < fmt.clip_min ? fmt.clip_min : vn);
    const float vs = (__builtin_rintf(u * fmt.sub_scale) + 0.0f) * fmt.min_subnormal;
    float v = mag < fmt.sub_limit ? vs : vn;
    v = u < fmt.lo ? fmt.lo : v;
    v = u > fmt.hi ? fmt.hi : v;
    return v;
}
template <int R>
__device__ __forceinline__ bool float_fast_ok(const FloatFmt& fmt) { return R == ROUND_HALF_EVEN && fmt.mantissa <= 22; }

// The small-float grid as a quantiser policy of fq_walk.hpp.  A state with a power-of-two scale takes quant_float_rne_pow2
// (FAST = false: never, the reference's own arithmetic throughout).
template <int R, bool FAST = true>
struct FloatQ {
    const FloatFmt& fmt;
    int rounding;
    struct State { float s, o; uint32_t rb; };
    __device__ __forceinline__ State make(float s, float o) const {
        return State{s, o, (FAST && float_fast_ok<R>(fmt)) ? pow2_reciprocal_bits(s) : 0u};
    }
    __device__ __forceinline__ bool fast(const State& st) const { return st.rb != 0u; }
    __device__ __forceinline__ float quant1(float v, const State& st) const {
        const float q = st.rb ? quant_float_rne_pow2(v, __uint_as_float(st.rb), fmt) : quant_float_scalar<R>(v, st.s, fmt, rounding);
        return (q - st.o) * st.s;
    }
    __device__ __forceinline__ float4 quant4(const float4& a, const State& st) const {
        return make_float4(quant1(a.x, st), quant1(a.y, st), quant1(a.z, st), quant1(a.w, st));
    }
};

// the fast path is kernel-uniform per tensor; per channel it diverges only where a wave straddles channels of both kinds
template <int R, int U, bool NT>
__global__ __launch_bounds__(kBlock) void fq_float_t_tile_kernel(
    const float4* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ offset,
    float4* __restrict__ out, uint32_t nvec, const float* __restrict__ xtail, float* __restrict__ otail,
    int ntail, FloatFmt fmt, int rounding) {
    fq_tile_t<U, NT, FQ_GUARD_SLOW>(FloatQ<R>{fmt, rounding}, x, scale, offset, out, nvec, xtail, otail, ntail);
}

template <int R, int U, bool NT>
__global__ __launch_bounds__(kBlock) void fq_float_c_tile_kernel(
    const float4* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ offset,
    float4* __restrict__ out, uint32_t nvec, FastDiv vec_per_channel, FastDiv num_channel, FloatFmt fmt,
    int rounding) {
    fq_tile_c<U, NT, FQ_GUARD_SLOW>(FloatQ<R>{fmt, rounding}, x, scale, offset, out, nvec, blockIdx.x, vec_per_channel, num_channel);
}

// element-wise per-tensor (per_channel == 0) / per-channel kernel
template <int R>
__global__ __launch_bounds__(kBlock) void fq_float_scalar_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ offset,
    float* __restrict__ out, uint32_t n, FastDiv elem_per_channel, FastDiv num_channel, int per_channel,
    FloatFmt fmt, int rounding) {
    fq_elems(FloatQ<R, false>{fmt, rounding}, x, scale, offset, out, blockIdx.x * kBlock + threadIdx.x, n, gridDim.x * kBlock,
             per_channel != 0, elem_per_channel, num_channel);
}

// QuantizeTensor_FT_B / _FC_B, floating.cu:133-331: STE + scale gradient with +-1 sentinel clip.
// The reference adds every block-partial divided by sqrtf((float)(n * clip_max)) with one atomic per block; here the
// tensor is cut into (row, chunk) workgroups of one channel each -- rows of elem_per_channel contiguous elements, chunks of
// 4096 -- that leave ONE partial sum per workgroup, and a second launch adds a channel's partials in a fixed order and
// divides once (deterministic; the first version issued one device atomic PER ELEMENT: 44 ms for [32, 512, 56, 56]).
__device__ __forceinline__ float fq_float_bwd_elem(float v, float d, float s, float inv_s, float o, float cmin, float cmax,
                                                   const FloatFmt& fmt_wide, float clip_min, float clip_max, int rounding,
                                                   float* gx) {
    const float qt = quant_float_scalar<-1>(v, s, fmt_wide, rounding);
    const float q = (qt - o) * s;
    if (qt == clip_max + 1) { *gx = 0.f; return cmax * d * inv_s; }
    if (qt == clip_min - 1) { *gx = 0.f; return cmin * d * inv_s; }
    *gx = d;
    return (q - v) * inv_s * d;
}

// fq_float_bwd_elem for the elements of one channel, as the element functor of fq_bwd_row
struct FloatBwdChannel {
    float s, inv_s, o, cmin, cmax;
    const FloatFmt& fmt_wide;
    float clip_min, clip_max;
    int rounding;
    __device__ __forceinline__ FloatBwdChannel(float scale, float offset, const FloatFmt& fmt_wide, float clip_min, float clip_max,
                                               int rounding)
        : s(scale), inv_s(1 / scale), o(offset), cmin(s * (clip_min - o)), cmax(s * (clip_max - o)), fmt_wide(fmt_wide),
          clip_min(clip_min), clip_max(clip_max), rounding(rounding) {}
    __device__ __forceinline__ float operator()(float v, float d, float* gx) const {
        return fq_float_bwd_elem(v, d, s, inv_s, o, cmin, cmax, fmt_wide, clip_min, clip_max, rounding, gx);
    }
};

constexpr uint32_t kFloatBwdChunk = 4096;      // elements per workgroup
template <bool NT>
__global__ __launch_bounds__(kBlock) void fq_float_bwd_row_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ offset,
    const float* __restrict__ dy, float* __restrict__ gx, float* __restrict__ partial, uint32_t epc, int vec_ok,
    FastDiv chunks, FastDiv num_channel, FloatFmt fmt_wide, float clip_min, float clip_max, int rounding) {
    __shared__ float lds[kBlock / kWave];
    const uint32_t row = fdiv(blockIdx.x, chunks);
    const uint32_t chunk = blockIdx.x - row * chunks.d;
    const uint32_t c = row - fdiv(row, num_channel) * num_channel.d;
    const FloatBwdChannel elem(scale[c], offset[c], fmt_wide, clip_min, clip_max, rounding);
    const uint32_t lo = chunk * kFloatBwdChunk, hi = min(lo + kFloatBwdChunk, epc);
    const size_t base = (size_t)row * epc;
    float acc = fq_bwd_row<4, NT>(x + base, dy + base, gx + base, lo, hi, vec_ok != 0, 0.f, elem);
    acc = wave_sum(acc);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) lds[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < kBlock / kWave; w++) t += lds[w];
        partial[blockIdx.x] = t;
    }
}

// short rows (elem_per_channel < 64: [N, C] matrices, channel-last views): fq_bwd_generic
__global__ __launch_bounds__(kBlock) void fq_float_bwd_generic_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ offset,
    const float* __restrict__ dy, float* __restrict__ gx, float* __restrict__ gs, uint32_t n, FastDiv elem_per_channel,
    FastDiv num_channel, int use_lds, FloatFmt fmt_wide, float clip_min, float clip_max, float denom, int rounding) {
    fq_bwd_generic(x, dy, gx, gs, n, elem_per_channel, num_channel, use_lds,
                   [&](uint32_t c, float v, float d, float* g) {
                       return FloatBwdChannel(scale[c], offset[c], fmt_wide, clip_min, clip_max, rounding)(v, d, g);
                   },
                   [&](float sum) { return sum / denom; });
}

// grad_s[c] = (sum of the partials of channel c: rows c, c + C, .. x their chunks, in index order) / denom
__global__ __launch_bounds__(kBlock) void fq_float_bwd_finish_kernel(const float* __restrict__ partial, uint32_t rows, uint32_t chunks,
                                                                     uint32_t C, float denom, float* __restrict__ gs) {
    const uint32_t c = blockIdx.x;
    const double t = fq_finish_sum<kBlock>((rows / C) * chunks, [&](uint32_t at) {
        const uint32_t r = at / chunks, k = at - r * chunks;
        return partial[(size_t)(r * C + c) * chunks + k];
    });
    if (threadIdx.x == 0) gs[c] = (float)t / denom;
}

// ---- many tensors, one launch (fq_walk.hpp) -------------------------------------------------------------------
typedef FqJobOf<FloatFmt> FqFloatJob;
typedef FqMultiArgsOf<FqFloatJob> FqFloatMultiArgs;
static_assert(sizeof(FqFloatJob) == 112, "callers size the device table with ppqhip_fq_float_multi_table_bytes");

template <int R, int U>
__global__ __launch_bounds__(kBlock) void fq_float_multi_kernel(const FqFloatMultiArgs args) {
    uint32_t local;
    const FqFloatJob j = args.jobs[job_of(args, local)];        // uniform address: scalar loads
    fq_multi_tile<U, FQ_GUARD_ALL>(FloatQ<R>{j.fmt, args.rounding}, j.x, j.out, j.scale, j.offset, j.n, j.vec_ok, j.per, j.nc, local);
}

// ---- the scale search of the FP8 'floating' observer, batched ------------------------------------------------
// DirectMSEObserver (observer/floating.py:88-143) fake-quantises its collected values with each of 7 candidate
// scales and keeps the one with the least mean squared error: 7 x (quantise, subtract, square, mean) launches and a
// host synchronisation PER CONFIG -- 148 configs on ViT-B/16, 29 ms of a 100 ms calibration.  Here ONE launch
// serves every config of the graph: a workgroup owns one row (a per-tensor collection, or one channel of a weight),
// reads it once, evaluates all candidates on the value in registers and writes the squared-error sums (double,
// fixed summation order: deterministic).  The dequantised value is formed in float32 exactly as the fake-quant
// kernels form it, so err = float32 result of fq - x as the reference's `qt - fp`.
constexpr int kSearchMaxCandidates = 8;
constexpr int kSearchMaxJobs = 128;
struct FloatSearchJob {
    const float* x;       // rows x row_len, contiguous
    uint32_t row_len;
    FloatFmt fmt;
};
struct FloatSearchArgs {
    uint32_t first_block[kSearchMaxJobs];    // prefix of row counts (one workgroup per row): workgroup -> job
    uint32_t count;
    int rounding, num_candidates;
    float candidate[kSearchMaxCandidates];
    const FloatSearchJob* jobs;
    double* out;                              // [total rows][num_candidates]
    uint32_t out_row0;
};

template <int R>
__global__ __launch_bounds__(kBlock) void float_scale_search_kernel(const FloatSearchArgs args) {
    __shared__ double red[kSearchMaxCandidates][kBlock / kWave];
    uint32_t local;
    const FloatSearchJob j = args.jobs[job_of(args, local)];
    const float* __restrict__ row = j.x + (size_t)local * j.row_len;
    double acc[kSearchMaxCandidates];
    uint32_t rb[kSearchMaxCandidates];
#pragma unroll
    for (int c = 0; c < kSearchMaxCandidates; c++) {
        acc[c] = 0.0;
        rb[c] = (c < args.num_candidates && float_fast_ok<R>(j.fmt)) ? pow2_reciprocal_bits(args.candidate[c]) : 0u;
    }
    for (uint32_t i = threadIdx.x; i < j.row_len; i += kBlock) {
        const float v = row[i];
#pragma unroll
        for (int c = 0; c < kSearchMaxCandidates; c++) {
            if (c < args.num_candidates) {
                const float s = args.candidate[c];
                const float q = rb[c] ? quant_float_rne_pow2(v, __uint_as_float(rb[c]), j.fmt)
                                      : quant_float_scalar<R>(v, s, j.fmt, args.rounding);
                const float e = (q - 0.0f) * s - v;          // offset 0 (floating.py:112,129); float32 like the fake-quant output
                acc[c] += (double)e * (double)e;
            }
        }
    }
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < kSearchMaxCandidates; c++) {
        double v = acc[c];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) red[c][wid] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < args.num_candidates) {
        double v = 0.0;
        for (int w = 0; w < kBlock / kWave; w++) v += red[threadIdx.x][w];
        args.out[(size_t)(args.out_row0 + blockIdx.x) * args.num_candidates + threadIdx.x] = v;
    }
}

template <int R>
static void launch_ft(const float* x, const float* scale, const float* offset, float* out, int64_t n,
                      const FloatFmt& fmt, int rounding, hipStream_t st) {
    if (fq_vec_ok(x, out) && n >= 4) {
        const uint32_t nvec = (uint32_t)(n >> 2);
        const int ntail = (int)(n & 3);
        const float* xt = x + (size_t)nvec * 4;
        float* ot = out + (size_t)nvec * 4;
        with_tile_shape(n, [&](auto u, auto nt) {
            hipLaunchKernelGGL((fq_float_t_tile_kernel<R, decltype(u)::value, decltype(nt)::value>), tile_grid(nvec, u), dim3(kBlock), 0,
                               st, (const float4*)x, scale, offset, (float4*)out, nvec, xt, ot, ntail, fmt, rounding);
        });
    } else {
        hipLaunchKernelGGL((fq_float_scalar_kernel<R>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, x, scale,
                           offset, out, (uint32_t)n, make_fastdiv(1), make_fastdiv(1), 0, fmt, rounding);
    }
}

template <int R>
static void launch_fc(const float* x, const float* scale, const float* offset, float* out, int64_t n, int64_t C,
                      int64_t epc, const FloatFmt& fmt, int rounding, hipStream_t st) {
    const FastDiv nc = make_fastdiv((uint32_t)C);
    if (fq_vec_ok(x, out, epc)) {
        const uint32_t nvec = (uint32_t)(n >> 2);
        const FastDiv vpc = make_fastdiv((uint32_t)(epc / 4));
        with_tile_shape(n, [&](auto u, auto nt) {
            hipLaunchKernelGGL((fq_float_c_tile_kernel<R, decltype(u)::value, decltype(nt)::value>), tile_grid(nvec, u), dim3(kBlock), 0,
                               st, (const float4*)x, scale, offset, (float4*)out, nvec, vpc, nc, fmt, rounding);
        });
    } else {
        hipLaunchKernelGGL((fq_float_scalar_kernel<R>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, x, scale,
                           offset, out, (uint32_t)n, make_fastdiv((uint32_t)epc), nc, 1, fmt, rounding);
    }
}

}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_fq_float_t(const float* x, const float* scale, const float* offset, float* out, int64_t n,
                      int exponent, int mantissa, float clip_min, float clip_max, int rounding,
                      void* stream) {
    if (int st = validate_n(n, "fq_float_t")) return st;
    FloatFmt fmt;
    if (int st = make_fmt(exponent, mantissa, clip_min, clip_max, &fmt, "fq_float_t")) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_FQ_FLOAT_T, 8.0 * (double)n, s);
    if (rounding == ROUND_HALF_EVEN) launch_ft<ROUND_HALF_EVEN>(x, scale, offset, out, n, fmt, rounding, s);
    else launch_ft<-1>(x, scale, offset, out, n, fmt, rounding, s);
    return finish_launch("fq_float_t");
}

int ppqhip_fq_float_c(const float* x, const float* scale, const float* offset, float* out, int64_t n,
                      int64_t num_channel, int64_t elem_per_channel, int exponent, int mantissa,
                      float clip_min, float clip_max, int rounding, void* stream) {
    if (int st = validate_n(n, "fq_float_c")) return st;
    if (int st = validate_channels(n, num_channel, elem_per_channel, "fq_float_c")) return st;
    FloatFmt fmt;
    if (int st = make_fmt(exponent, mantissa, clip_min, clip_max, &fmt, "fq_float_c")) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_FQ_FLOAT_C, 8.0 * (double)n, s);
    if (rounding == ROUND_HALF_EVEN)
        launch_fc<ROUND_HALF_EVEN>(x, scale, offset, out, n, num_channel, elem_per_channel, fmt, rounding, s);
    else launch_fc<-1>(x, scale, offset, out, n, num_channel, elem_per_channel, fmt, rounding, s);
    return finish_launch("fq_float_c");
}

int64_t ppqhip_fq_float_multi_table_bytes(int num_jobs) {
    return num_jobs > 0 ? (int64_t)sizeof(FqFloatJob) * num_jobs : 0;
}

int ppqhip_fq_float_multi(const ppqhip_fq_float_job* jobs, int num_jobs, int rounding, void* device_table, int upload,
                          void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return fq_multi<FloatFmt>(
        "fq_float_multi", K_FQ_FLOAT_C, jobs, num_jobs, rounding, device_table, upload, s,
        [](const ppqhip_fq_float_job& src, FloatFmt* f) {
            return make_fmt(src.exponent, src.mantissa, src.clip_min, src.clip_max, f, "fq_float_multi");
        },
        [&](uint32_t blocks, const FqFloatMultiArgs& args) {
            if (rounding == ROUND_HALF_EVEN)
                hipLaunchKernelGGL((fq_float_multi_kernel<ROUND_HALF_EVEN, kFqMultiU>), dim3(blocks), dim3(kBlock), 0, s, args);
            else
                hipLaunchKernelGGL((fq_float_multi_kernel<-1, kFqMultiU>), dim3(blocks), dim3(kBlock), 0, s, args);
        });
}

int64_t ppqhip_float_scale_search_table_bytes(int num_jobs) {
    return num_jobs > 0 ? (int64_t)sizeof(FloatSearchJob) * num_jobs : 0;
}

int ppqhip_float_scale_search(const ppqhip_float_search_job* jobs, int num_jobs, const float* candidates, int num_candidates,
                              int rounding, void* device_table, double* out, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (jobs == nullptr || candidates == nullptr || device_table == nullptr || out == nullptr) {
        set_error("float_scale_search: null argument"); return PPQHIP_ERR_INVALID_VALUE;
    }
    if (num_candidates <= 0 || num_candidates > kSearchMaxCandidates) {
        set_error("float_scale_search: 1 .. %d candidate scales are supported, got %d", kSearchMaxCandidates, num_candidates);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_float_search_job& j = jobs[k];
        if (j.x == nullptr || j.rows <= 0 || j.row_len <= 0 || j.rows > 0x7fffffffLL || j.row_len > 0x7fffffffLL) {
            set_error("float_scale_search: job %d is empty or too large", k); return PPQHIP_ERR_INVALID_VALUE;
        }
        FloatFmt probe;
        if (int st = make_fmt(j.exponent, j.mantissa, j.clip_min, j.clip_max, &probe, "float_scale_search")) return st;
        bytes += 4.0 * (double)j.rows * (double)j.row_len;
    }
    LaunchScope scope(K_FLOAT_SCALE_SEARCH, bytes, s);
    uint32_t row0 = 0;
    for (int base = 0; base < num_jobs; base += kSearchMaxJobs) {
        const int count = (num_jobs - base) < kSearchMaxJobs ? (num_jobs - base) : kSearchMaxJobs;
        FloatSearchArgs args;
        args.count = (uint32_t)count; args.rounding = rounding; args.num_candidates = num_candidates;
        for (int c = 0; c < kSearchMaxCandidates; c++) args.candidate[c] = c < num_candidates ? candidates[c] : 1.0f;
        args.jobs = (const FloatSearchJob*)device_table + base;
        args.out = out; args.out_row0 = row0;
        std::vector<FloatSearchJob> table(count);
        uint32_t rows = 0;
        for (int k = 0; k < count; k++) {
            const ppqhip_float_search_job& src = jobs[base + k];
            args.first_block[k] = rows;
            rows += (uint32_t)src.rows;
            table[k].x = src.x; table[k].row_len = (uint32_t)src.row_len;
            make_fmt(src.exponent, src.mantissa, src.clip_min, src.clip_max, &table[k].fmt, "float_scale_search");
        }
        if (int st = check_hip(hipMemcpyAsync((FloatSearchJob*)device_table + base, table.data(), sizeof(FloatSearchJob) * count,
                                              hipMemcpyHostToDevice, s), "float_scale_search table upload"))
            return st;
        if (rounding == ROUND_HALF_EVEN) hipLaunchKernelGGL((float_scale_search_kernel<ROUND_HALF_EVEN>), dim3(rows), dim3(kBlock), 0, s, args);
        else hipLaunchKernelGGL((float_scale_search_kernel<-1>), dim3(rows), dim3(kBlock), 0, s, args);
        row0 += rows;
    }
    return finish_launch("float_scale_search");
}

int ppqhip_fq_float_c_bwd(const float* x, const float* scale, const float* offset, const float* grad_y,
                          float* grad_x, float* grad_s, int64_t n, int64_t num_channel,
                          int64_t elem_per_channel, int exponent, int mantissa, float clip_min,
                          float clip_max, int rounding, void* stream) {
    if (int st = validate_n(n, "fq_float_c_bwd")) return st;
    if (int st = validate_channels(n, num_channel, elem_per_channel, "fq_float_c_bwd")) return st;
    FloatFmt fmt;   // the backward quantises against [clip_min - 1, clip_max + 1]: floating.cu:163-164
    if (int st = make_fmt(exponent, mantissa, clip_min - 1, clip_max + 1, &fmt, "fq_float_c_bwd")) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_FQ_FLOAT_BWD, 12.0 * (double)n, s);
    const float denom = sqrtf((float)((float)n * clip_max));
    if (elem_per_channel < 64) {
        if (int st = check_hip(hipMemsetAsync(grad_s, 0, sizeof(float) * (size_t)num_channel, s), "memset grad_s")) return st;
        const int use_lds = num_channel <= 8192;
        hipLaunchKernelGGL(fq_float_bwd_generic_kernel, dim3(stream_grid(n, kBlock * 8, num_cu() * 2)), dim3(kBlock),
                           use_lds ? sizeof(float) * (size_t)num_channel : 0, s, x, scale, offset, grad_y, grad_x, grad_s, (uint32_t)n,
                           make_fastdiv((uint32_t)elem_per_channel), make_fastdiv((uint32_t)num_channel), use_lds, fmt, clip_min,
                           clip_max, denom, rounding);
        return finish_launch("fq_float_c_bwd");
    }
    const uint32_t chunks = (uint32_t)((elem_per_channel + kFloatBwdChunk - 1) / kFloatBwdChunk);
    const int64_t rows = n / elem_per_channel;
    if (rows * chunks > 0x7fffffffLL) { set_error("fq_float_c_bwd: too many rows"); return PPQHIP_ERR_INVALID_VALUE; }
    float* partial = (float*)scratch(s, sizeof(float) * (size_t)(rows * chunks));
    if (partial == nullptr) return PPQHIP_ERR_HIP;
    const int vec_ok = fq_bwd_vec_ok(x, grad_y, grad_x, elem_per_channel) ? 1 : 0;
    // x and dy together exceed cache residency from 96 MiB each: streaming (nontemporal) loads, as the linear backward kernels
    if (n >= (24ll << 20))
        hipLaunchKernelGGL(fq_float_bwd_row_kernel<true>, dim3((uint32_t)(rows * chunks)), dim3(kBlock), 0, s, x, scale, offset, grad_y,
                           grad_x, partial, (uint32_t)elem_per_channel, vec_ok, make_fastdiv(chunks),
                           make_fastdiv((uint32_t)num_channel), fmt, clip_min, clip_max, rounding);
    else
        hipLaunchKernelGGL(fq_float_bwd_row_kernel<false>, dim3((uint32_t)(rows * chunks)), dim3(kBlock), 0, s, x, scale, offset, grad_y,
                           grad_x, partial, (uint32_t)elem_per_channel, vec_ok, make_fastdiv(chunks),
                           make_fastdiv((uint32_t)num_channel), fmt, clip_min, clip_max, rounding);
    hipLaunchKernelGGL(fq_float_bwd_finish_kernel, dim3((uint32_t)num_channel), dim3(kBlock), 0, s, (const float*)partial,
                       (uint32_t)rows, chunks, (uint32_t)num_channel, denom, grad_s);
    return finish_launch("fq_float_c_bwd");
}

}  // extern "C"
