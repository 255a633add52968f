// stats.hip -- the two launches of the statistical reports (ppq_amd/statistics.py): statistical_analyse of
// ppq/quantization/analyse/graphwise.py:186-372, parameter_analyse / variable_analyse of analyse/layerwise.py:137-203.
//
// A job is one float32 SERIES x[n]: either a dense array, or the difference fl32(p[i] - r[i]) of a pair (the noise of a
// quantised series p against its FP32 twin r), and one RECORD of 4-byte words that both kernels fill:
//   rec[0] mean_f   rec[1] std_f   rec[2] min   rec[3] max   rec[4] skewness   rec[5] kurtosis   rec[6] NOISE:SIGNAL   rec[7] 0
//   rec[8 .. 8 + bins)  the histogram counts, int32
//
// 1. ppqhip_stat_moments_multi: n, mean, M2 = sum (x - mean)^2, min and max in ONE read.  A workgroup keeps its piece of the
//    series (<= kStChunk elements) in registers, sums it in double, divides, and sums the squared double differences from that
//    mean: a two-pass (n, mean, M2) per piece, no sum of squares minus squared sum anywhere.  The pieces of a long series are
//    merged Chan-style -- delta = mean_b - mean_a;  mean = mean_a + delta * n_b / n;  M2 = M2_a + M2_b + delta^2 * n_a * n_b / n
//    -- by one wave: lane l folds pieces l, l + 64, ... in order, then the lanes fold in a shift-down tree.
//      mean_f = (float)mean    std_f = (float)sqrt(M2 / (n - 1))   (n = 1: 0 / 0 = NaN, as torch.std)
//    A pair job also gets the two sums of torch_snr_error(p, r) with the arithmetic of measure.hip -- d = p - r, d * d and r * r
//    each ONE fp32 operation, double adds -- and rec[6] = (float)noise / ((float)signal + 1e-7f).
// 2. ppqhip_stat_shape_multi: reads mean_f, std_f, lo = min, hi = max FROM THE RECORD (device memory: no host round trip) and
//    makes, every step ONE IEEE fp32 operation (-ffp-contract=off, correctly rounded division):
//      t = (x - mean_f) / std_f;  t2 = t * t;  t3 = t2 * t;  t4 = t2 * t2
//      skewness = (float)(sum_double t3 / n)     kurtosis = (float)(sum_double t4 / n) - 3.0f     std_f == 0: NaN in both
//      lo == hi: lo -= 1, hi += 1 (torch.histc);   pos = ((x - lo) * bins) / (hi - lo);   bin = min((int)pos, bins - 1)
//    Counts are LDS integer atomics (one copy per wave), exact.  The pieces of a long series write their sums and counts into the
//    stream's scratch and a wave per job adds them in a fixed order.
//
// Element e of a piece belongs to thread (e / 4) % 1024 at trip e / 4096 whether it arrives in a 16-B load or in guarded 4-B loads,
// lanes fold in the xor tree, waves in index order, pieces as above: the bits depend on n alone, not on the pointers, the other
// jobs or the device.  No global atomics.  NaN in a series is not ordered by min / max (v_min / v_max drop it).
//
// Job tables: DESIGN.md, "Job tables" (a first use of the split path on a stream grows its scratch: run it once eagerly before capturing).
#include <algorithm>

#include "common.hpp"
#include "job_table.hpp"
#include "measure_rows.hpp"

namespace ppqhip {
namespace {

constexpr uint32_t kStChunk = 16384;               // elements per workgroup: the analysis' (steps + 1) * 1024 samples fit one
constexpr int kStBlock = 1024;                     // 16 waves: 4 float4 per lane, held in registers between the two passes
constexpr int kStWaves = kStBlock / kWave;
constexpr int kStU = kStChunk / (4 * kStBlock);
constexpr int kStMaxJobs = 88;
constexpr int kStMaxBins = 64;
constexpr int kMoPartial = 8;                      // doubles per piece: n, mean, M2, min, max, noise, signal, -
constexpr int kShPartial = 2 + kStMaxBins / 2;     // doubles per piece: sum t3, sum t4, then 64 uint32 counts

struct StJob {                                     // 40 B
    const float* p;
    const float* r;                                // nullptr: the series is p itself
    float* rec;
    uint32_t n, chunks, partial, bins;             // partial: first piece of this job in the scratch (units of pieces)
};
struct StArgs {
    StJob jobs[kStMaxJobs];
    uint32_t first_block[kStMaxJobs];
    uint32_t count;
    double* scratch;
};
static_assert(sizeof(StArgs) <= 4096, "kernel arguments are limited to 4 KB");

// every thread gets the sum of all threads' v: lanes in the xor tree, waves in index order
__device__ __forceinline__ double block_sum_f64(double v, double* lds) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < kStWaves; w++) t += lds[w];
    return t;
}

// the piece [begin, begin + len) of the series of job j in registers; slots past the end read as 0
template <bool PAIR>
__device__ __forceinline__ void load_piece(const StJob& j, uint32_t begin, uint32_t len, float4 (&v)[kStU], double& noise,
                                           double& signal) {
    const float* p = j.p + begin;                  // kStChunk * 4 B keeps the alignment of the series' start
    const float* r = PAIR ? j.r + begin : nullptr;
    const bool pv = aligned16_d(p), rv = PAIR && aligned16_d(r);
#pragma unroll
    for (int u = 0; u < kStU; u++) {
        const uint32_t e = ((uint32_t)u * kStBlock + threadIdx.x) * 4u;
        float4 a = load4_guarded(p, e, len, pv);
        if (PAIR) {
            const float4 b = load4_guarded(r, e, len, rv);
            a.x = a.x - b.x; a.y = a.y - b.y; a.z = a.z - b.z; a.w = a.w - b.w;
            noise += (double)(a.x * a.x); noise += (double)(a.y * a.y); noise += (double)(a.z * a.z); noise += (double)(a.w * a.w);
            signal += (double)(b.x * b.x); signal += (double)(b.y * b.y); signal += (double)(b.z * b.z); signal += (double)(b.w * b.w);
        }
        v[u] = a;
    }
}

// f(value) for every EXISTING element of the piece, in the order of its index
template <typename F>
__device__ __forceinline__ void for_piece(const float4 (&v)[kStU], uint32_t len, F f) {
#pragma unroll
    for (int u = 0; u < kStU; u++) {
        const uint32_t e = ((uint32_t)u * kStBlock + threadIdx.x) * 4u;
        if (e < len) f(v[u].x);
        if (e + 1 < len) f(v[u].y);
        if (e + 2 < len) f(v[u].z);
        if (e + 3 < len) f(v[u].w);
    }
}

__device__ __forceinline__ float snr_of(double noise, double signal) { return (float)noise / ((float)signal + 1e-7f); }

__device__ __forceinline__ void write_moments(float* rec, double n, double mean, double m2, float lo, float hi, float snr) {
    rec[0] = (float)mean;
    rec[1] = (float)sqrt(m2 / (n - 1.0));
    rec[2] = lo; rec[3] = hi;
    rec[6] = snr; rec[7] = 0.f;
}

template <bool PAIR>
__device__ __forceinline__ void moments_piece(const StJob& j, uint32_t chunk, double* __restrict__ scratch, double* lds,
                                              float (*ext)[kStWaves]) {
    const uint32_t begin = chunk * kStChunk, len = min(kStChunk, j.n - begin);
    float4 v[kStU];
    double noise = 0.0, signal = 0.0;
    load_piece<PAIR>(j, begin, len, v, noise, signal);
    double sum = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for_piece(v, len, [&](float x) { sum += (double)x; lo = fminf(lo, x); hi = fmaxf(hi, x); });
    const double mean = block_sum_f64(sum, lds) / (double)len;
    double m2 = 0.0;
    for_piece(v, len, [&](float x) { const double d = (double)x - mean; m2 += d * d; });
    m2 = block_sum_f64(m2, lds);
    if (PAIR) { noise = block_sum_f64(noise, lds); signal = block_sum_f64(signal, lds); }
    lo = wave_min(lo); hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { ext[0][threadIdx.x >> 6] = lo; ext[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 0; w < kStWaves; w++) { lo = fminf(lo, ext[0][w]); hi = fmaxf(hi, ext[1][w]); }
    if (j.chunks == 1) { write_moments(j.rec, (double)len, mean, m2, lo, hi, PAIR ? snr_of(noise, signal) : 0.f); return; }
    double* o = scratch + ((size_t)j.partial + chunk) * kMoPartial;
    o[0] = (double)len; o[1] = mean; o[2] = m2; o[3] = (double)lo; o[4] = (double)hi; o[5] = noise; o[6] = signal; o[7] = 0.0;
}

__global__ __launch_bounds__(kStBlock) void stat_moments_kernel(const StArgs args) {
    __shared__ double lds[kStWaves];
    __shared__ float ext[2][kStWaves];
    uint32_t local;
    const StJob& j = args.jobs[job_of(args, local)];
    if (j.r != nullptr) moments_piece<true>(j, local, args.scratch, lds, ext);
    else moments_piece<false>(j, local, args.scratch, lds, ext);
}

struct Moments {
    double n, mean, m2, lo, hi, noise, signal;
    __device__ __forceinline__ void merge(const Moments& b) {        // Chan et al.; a side without elements changes nothing
        if (b.n == 0.0) return;
        if (n == 0.0) { *this = b; return; }
        const double total = n + b.n, delta = b.mean - mean;
        mean = mean + delta * b.n / total;
        m2 = m2 + b.m2 + delta * delta * n * b.n / total;
        n = total;
        lo = fmin(lo, b.lo); hi = fmax(hi, b.hi);
        noise += b.noise; signal += b.signal;
    }
};

// one WAVE per split job
__global__ __launch_bounds__(kBlock) void stat_moments_fold_kernel(const StArgs args) {
    const uint32_t k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= args.count) return;
    const StJob& j = args.jobs[__builtin_amdgcn_readfirstlane(k)];
    const uint32_t lane = threadIdx.x & 63;
    Moments a = {0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0, 0.0};
    for (uint32_t c = lane; c < j.chunks; c += kWave) {
        const double* q = args.scratch + ((size_t)j.partial + c) * kMoPartial;
        const Moments b = {q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
        a.merge(b);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        Moments b;
        b.n = __shfl_down(a.n, m, 64); b.mean = __shfl_down(a.mean, m, 64); b.m2 = __shfl_down(a.m2, m, 64);
        b.lo = __shfl_down(a.lo, m, 64); b.hi = __shfl_down(a.hi, m, 64);
        b.noise = __shfl_down(a.noise, m, 64); b.signal = __shfl_down(a.signal, m, 64);
        if (lane < (uint32_t)m) a.merge(b);
    }
    if (lane == 0) write_moments(j.rec, a.n, a.mean, a.m2, (float)a.lo, (float)a.hi, j.r != nullptr ? snr_of(a.noise, a.signal) : 0.f);
}

__device__ __forceinline__ void write_shape(float* rec, double s3, double s4, double n, float std_f) {
    const float skew = (float)(s3 / n), kurt = (float)(s4 / n) - 3.0f;
    rec[4] = std_f == 0.f ? NAN : skew;
    rec[5] = std_f == 0.f ? NAN : kurt;
}

template <bool PAIR>
__device__ __forceinline__ void shape_piece(const StJob& j, uint32_t chunk, double* __restrict__ scratch, double* lds,
                                            uint32_t (*hist)[kStMaxBins]) {
    const uint32_t begin = chunk * kStChunk, len = min(kStChunk, j.n - begin);
    float4 v[kStU];
    double unused0 = 0.0, unused1 = 0.0;
    load_piece<PAIR>(j, begin, len, v, unused0, unused1);
    const float mean_f = j.rec[0], std_f = j.rec[1];
    float lo = j.rec[2], hi = j.rec[3];
    if (lo == hi) { lo = lo - 1.0f; hi = hi + 1.0f; }
    const float width = hi - lo, fbins = (float)j.bins;
    const int last = (int)j.bins - 1;
    for (uint32_t b = threadIdx.x; b < kStWaves * kStMaxBins; b += kStBlock) (&hist[0][0])[b] = 0u;
    __syncthreads();
    uint32_t* mine = hist[threadIdx.x >> 6];
    double s3 = 0.0, s4 = 0.0;
    for_piece(v, len, [&](float x) {
        const float t = (x - mean_f) / std_f;
        const float t2 = t * t;
        s3 += (double)(t2 * t);
        s4 += (double)(t2 * t2);
        if (last >= 0) {
            const float pos = ((x - lo) * fbins) / width;
            atomicAdd(&mine[max(min(f2i_sat(pos), last), 0)], 1u);
        }
    });
    s3 = block_sum_f64(s3, lds);
    s4 = block_sum_f64(s4, lds);                   // (its barriers also order the LDS counts before the reads below)
    if (j.chunks == 1) {
        if (threadIdx.x == 0) write_shape(j.rec, s3, s4, (double)len, std_f);
        if (threadIdx.x < j.bins) {
            uint32_t c = 0;
            for (int w = 0; w < kStWaves; w++) c += hist[w][threadIdx.x];
            reinterpret_cast<int32_t*>(j.rec)[8 + threadIdx.x] = (int32_t)c;
        }
        return;
    }
    double* o = scratch + ((size_t)j.partial + chunk) * kShPartial;
    if (threadIdx.x == 0) { o[0] = s3; o[1] = s4; }
    if (threadIdx.x < kStMaxBins) {
        uint32_t c = 0;
        for (int w = 0; w < kStWaves; w++) c += hist[w][threadIdx.x];
        reinterpret_cast<uint32_t*>(o + 2)[threadIdx.x] = c;
    }
}

__global__ __launch_bounds__(kStBlock) void stat_shape_kernel(const StArgs args) {
    __shared__ double lds[kStWaves];
    __shared__ uint32_t hist[kStWaves][kStMaxBins];
    uint32_t local;
    const StJob& j = args.jobs[job_of(args, local)];
    if (j.r != nullptr) shape_piece<true>(j, local, args.scratch, lds, hist);
    else shape_piece<false>(j, local, args.scratch, lds, hist);
}

// one WAVE per split job: lane l adds the sums of pieces l, l + 64, ... in order, the lanes fold in the xor tree; lane b adds
// the counts of bin b over the pieces
__global__ __launch_bounds__(kBlock) void stat_shape_fold_kernel(const StArgs args) {
    const uint32_t k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= args.count) return;
    const StJob& j = args.jobs[__builtin_amdgcn_readfirstlane(k)];
    const uint32_t lane = threadIdx.x & 63;
    const double* base = args.scratch + (size_t)j.partial * kShPartial;
    double s3 = 0.0, s4 = 0.0;
    uint32_t c = 0;
    for (uint32_t q = lane; q < j.chunks; q += kWave) { s3 += base[(size_t)q * kShPartial]; s4 += base[(size_t)q * kShPartial + 1]; }
    for (uint32_t q = 0; q < j.chunks; q++) c += reinterpret_cast<const uint32_t*>(base + (size_t)q * kShPartial + 2)[lane];
    s3 = wave_sum_f64(s3);
    s4 = wave_sum_f64(s4);
    if (lane == 0) write_shape(j.rec, s3, s4, (double)j.n, j.rec[1]);
    if (lane < j.bins) reinterpret_cast<int32_t*>(j.rec)[8 + lane] = (int32_t)c;
}

int validate(const ppqhip_stat_job* jobs, int num_jobs, bool shape, const char* what, double& bytes) {
    if (int st = check_job_table(what, jobs, num_jobs)) return st;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_stat_job& j = jobs[k];
        if (j.n <= 0 || j.n > 0x7fffffffLL) { set_error("%s: job %d is empty or has more than 2^31 - 1 elements", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!j.p || !j.rec) { set_error("%s: job %d has a null pointer", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if ((reinterpret_cast<uintptr_t>(j.rec) & 3u) != 0) { set_error("%s: job %d: the record is not 4-byte aligned", what, k); return PPQHIP_ERR_INVALID_VALUE; }
        if (j.bins < 0 || j.bins > kStMaxBins) {
            set_error("%s: job %d: %d bins (at most %d)", what, k, j.bins, kStMaxBins); return PPQHIP_ERR_INVALID_VALUE;
        }
        bytes += (double)j.n * (j.r ? 8.0 : 4.0) + 32.0 + (shape ? 4.0 * j.bins : 0.0);
    }
    return PPQHIP_OK;
}

template <typename Main, typename Fold>
int launch_all(const ppqhip_stat_job* jobs, int num_jobs, int partial_doubles, hipStream_t s, Main main_kernel, Fold fold_kernel) {
    for (int base = 0; base < num_jobs; ) {
        StArgs args, fold;
        uint64_t blocks = 0, partials = 0;
        int count = 0, folds = 0;
        for (; count < kStMaxJobs && base + count < num_jobs; count++) {
            const ppqhip_stat_job& src = jobs[base + count];
            const uint32_t chunks = (uint32_t)((src.n + kStChunk - 1) / kStChunk);
            if (blocks + chunks > 0x7fffffffULL && count > 0) break;    // the rest goes into the next launch
            StJob& d = args.jobs[count];
            d.p = src.p; d.r = src.r; d.rec = src.rec;
            d.n = (uint32_t)src.n; d.chunks = chunks; d.partial = (uint32_t)partials; d.bins = (uint32_t)src.bins;
            args.first_block[count] = (uint32_t)blocks;
            blocks += chunks;
            if (chunks > 1) { fold.jobs[folds++] = d; partials += chunks; }
        }
        pad_job_table(args, (uint32_t)count, (uint32_t)blocks);
        args.scratch = nullptr;
        if (folds > 0) {
            args.scratch = (double*)scratch(s, (size_t)partials * partial_doubles * sizeof(double));
            if (!args.scratch) return PPQHIP_ERR_HIP;
        }
        hipLaunchKernelGGL(main_kernel, dim3((uint32_t)blocks), dim3(kStBlock), 0, s, args);
        if (folds > 0) {
            for (int k = folds; k < kStMaxJobs; k++) fold.jobs[k] = fold.jobs[0];
            for (int k = 0; k < kStMaxJobs; k++) fold.first_block[k] = 0;
            fold.count = (uint32_t)folds;
            fold.scratch = args.scratch;
            hipLaunchKernelGGL(fold_kernel, dim3((folds + kWaves - 1) / kWaves), dim3(kBlock), 0, s, fold);
        }
        base += count;
    }
    return PPQHIP_OK;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_stat_moments_multi(const ppqhip_stat_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    double bytes = 0.0;
    if (int st = validate(jobs, num_jobs, false, "stat_moments_multi", bytes)) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_STAT_MOMENTS, bytes, s);
    if (int st = launch_all(jobs, num_jobs, kMoPartial, s, stat_moments_kernel, stat_moments_fold_kernel)) return st;
    return finish_launch("stat_moments_multi");
}

int ppqhip_stat_shape_multi(const ppqhip_stat_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    double bytes = 0.0;
    if (int st = validate(jobs, num_jobs, true, "stat_shape_multi", bytes)) return st;
    hipStream_t s = (hipStream_t)stream;
    LaunchScope scope(K_STAT_SHAPE, bytes, s);
    if (int st = launch_all(jobs, num_jobs, kShPartial, s, stat_shape_kernel, stat_shape_fold_kernel)) return st;
    return finish_launch("stat_shape_multi");
}

}  // extern "C"
