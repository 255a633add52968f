// measure.hip -- the error analysis' three launches (ppq_amd/analyse.py, ppq_amd/measure.py): the batch-wise sample fetch of
// ppq/utils/fetch.py:98-122, the four row sums every measure of ppq/quantization/measure/ is made of, and the per-row measure
// with its running accumulation (MeasureRecorder, ppq/quantization/analyse/util).  Every analysed output of one forward
// shares ONE launch of each.
//
// Arithmetic contract of the row sums.  Per element, each ONE fp32 operation (-ffp-contract=off, Makefile):
//   d = p - r;   d * d;   r * r;   p * p;   p * r
// and every accumulation is a double add.  A product of two floats converts to double exactly, so each sum is the exact sum of
// its fp32 terms up to count * 2^-53 relative (non-negative terms), whatever the order -- and the order is fixed by the SHAPES
// alone: element e of a chunk belongs to lane (e / 4) % lanes at trip e / (4 * lanes); a lane adds its elements in index order,
// the lanes fold in the xor tree of wave_sum_f64, the waves of a workgroup in index order, the chunks of a row as
// measure_fold_kernel says.  Whether a float4 arrives as one 16-B load (row start 16-B aligned) or as four guarded 4-B loads (misaligned row, the count % 4 tail)
// does not move an element to another lane, so the bits do not depend on the pointers either.  No atomics.
//
// Size-dependent paths:  count <= kWaveRow: one WAVE per row (four rows per workgroup, no LDS);  count <= kChunk: one workgroup
// per row;  above: ceil(count / kChunk) workgroups per row write partials into the stream's scratch and a second kernel folds
// them (a wave per row).  kChunk is a constant: the split of a row never depends on the device or on the other jobs.
//
// Jobs: the table travels BY VALUE in the kernel arguments (<= kMsMaxJobs per launch, more are chunked): no upload, no
// synchronisation, capturable into a HIP graph (a first use of the split path on a stream grows its scratch: run it once
// eagerly before capturing, as for the other scratch users).
#include <algorithm>

#include "common.hpp"

namespace ppqhip {
namespace {

constexpr int kMsMaxJobs = 56;                     // 56 x (64 + 4) B of job table: inside the 4 KB of kernel arguments
constexpr uint32_t kWaveRow = 1024;                // rows up to here: one wave each (<= 4 float4 per lane)
constexpr uint32_t kChunk = 8192;                  // elements per workgroup: 8 float4 of p and of r per lane (16384 and 32768
                                                   // measured the same on ResNet-50's outputs: profiles/r09_analyse.txt)
constexpr int kWaves = kBlock / kWave;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct MsJob {                                     // 64 B
    const float* p;
    const float* r;
    const int32_t* index;                          // nullptr: p is dense (row_len == count)
    double* sums;                                  // [rows][4]
    uint32_t rows, row_len, count, chunks;         // chunks = 0: the wave path
    uint32_t partial;                              // chunks > 1: first partial of this job in the scratch (units of 4 doubles)
    uint32_t index_vec;                            // index is 16-B aligned
    uint32_t pad0, pad1;
};
struct MsArgs {
    MsJob jobs[kMsMaxJobs];
    uint32_t first_block[kMsMaxJobs];
    uint32_t count;
    double* scratch;
};
static_assert(sizeof(MsArgs) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ bool aligned16_d(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename A>
__device__ __forceinline__ uint32_t job_of(const A& args, uint32_t& local) {
    uint32_t lo = 0, hi = args.count;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (args.first_block[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    local = blockIdx.x - args.first_block[lo];
    return __builtin_amdgcn_readfirstlane(lo);
}

// four consecutive elements x[e .. e + 4) of a row of `len`; slots past the end read as 0 (they add +0.0 to every sum)
__device__ __forceinline__ float4 load4_guarded(const float* __restrict__ x, uint32_t e, uint32_t len, bool vec) {
    if (vec && e + 4 <= len) return *reinterpret_cast<const float4*>(x + e);
    float4 a;
    a.x = e < len ? x[e] : 0.f;
    a.y = e + 1 < len ? x[e + 1] : 0.f;
    a.z = e + 2 < len ? x[e + 2] : 0.f;
    a.w = e + 3 < len ? x[e + 3] : 0.f;
    return a;
}
// the same through the index table; an index outside the row is clamped into it (never read out of bounds)
__device__ __forceinline__ float4 gather4_guarded(const float* __restrict__ x, const int32_t* __restrict__ index, uint32_t e,
                                                  uint32_t len, bool vec, uint32_t row_len) {
    int4 k = make_int4(0, 0, 0, 0);
    if (vec && e + 4 <= len) k = *reinterpret_cast<const int4*>(index + e);
    else {
        if (e < len) k.x = index[e];
        if (e + 1 < len) k.y = index[e + 1];
        if (e + 2 < len) k.z = index[e + 2];
        if (e + 3 < len) k.w = index[e + 3];
    }
    const uint32_t last = row_len - 1;
    float4 a;
    a.x = e < len ? x[min((uint32_t)k.x, last)] : 0.f;
    a.y = e + 1 < len ? x[min((uint32_t)k.y, last)] : 0.f;
    a.z = e + 2 < len ? x[min((uint32_t)k.z, last)] : 0.f;
    a.w = e + 3 < len ? x[min((uint32_t)k.w, last)] : 0.f;
    return a;
}

struct Sums4 {
    double noise, signal, pp, pr;
    __device__ __forceinline__ void add(float p, float r) {
        const float d = p - r;
        noise += (double)(d * d);
        signal += (double)(r * r);
        pp += (double)(p * p);
        pr += (double)(p * r);
    }
    __device__ __forceinline__ void add4(const float4& p, const float4& r) {
        add(p.x, r.x); add(p.y, r.y); add(p.z, r.z); add(p.w, r.w);
    }
    __device__ __forceinline__ void wave_fold() {
        noise = wave_sum_f64(noise); signal = wave_sum_f64(signal); pp = wave_sum_f64(pp); pr = wave_sum_f64(pr);
    }
};

// elements [0, len) of one row piece over LANES lanes (lane = this thread's index among them), U float4 pairs in flight
template <int LANES, int U, bool GATHER>
__device__ __forceinline__ void sum_piece(const float* __restrict__ p, const float* __restrict__ r, const int32_t* __restrict__ index,
                                          uint32_t len, uint32_t row_len, bool p_vec, bool r_vec, uint32_t lane, Sums4& s) {
    for (uint32_t e0 = lane * 4u; e0 < len; e0 += 4u * LANES * U) {
        float4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t e = e0 + 4u * LANES * u;
            a[u] = GATHER ? gather4_guarded(p, index, e, len, p_vec, row_len) : load4_guarded(p, e, len, p_vec);
            b[u] = load4_guarded(r, e, len, r_vec);
        }
#pragma unroll
        for (int u = 0; u < U; u++) s.add4(a[u], b[u]);
    }
}

template <bool GATHER>
__device__ __forceinline__ void measure_job(const MsJob& j, uint32_t local, double* __restrict__ scratch, double (*lds)[4]) {
    Sums4 s = {0.0, 0.0, 0.0, 0.0};
    if (j.chunks == 0) {                                              // one wave per row
        const uint32_t row = local * kWaves + (threadIdx.x >> 6);
        if (row >= j.rows) return;
        const float* r = j.r + (size_t)row * j.count;
        const float* p = j.p + (size_t)row * j.row_len;
        sum_piece<kWave, 4, GATHER>(p, r, j.index, j.count, j.row_len, GATHER ? j.index_vec != 0 : aligned16_d(p), aligned16_d(r),
                                    threadIdx.x & 63, s);
        s.wave_fold();
        if ((threadIdx.x & 63) == 0) {
            double* o = j.sums + (size_t)row * 4;
            o[0] = s.noise; o[1] = s.signal; o[2] = s.pp; o[3] = s.pr;
        }
        return;
    }
    const uint32_t row = local / j.chunks, chunk = local - row * j.chunks;
    const uint32_t begin = chunk * kChunk, len = min(kChunk, j.count - begin);
    const float* r = j.r + (size_t)row * j.count + begin;
    // gathered: the chunk walks the index table, p stays the row;  dense: p advances with r (kChunk * 4 B keeps the alignment)
    const float* p = j.p + (size_t)row * j.row_len + (GATHER ? 0u : begin);
    sum_piece<kBlock, 4, GATHER>(p, r, GATHER ? j.index + begin : nullptr, len, j.row_len,
                                 GATHER ? j.index_vec != 0 : aligned16_d(p), aligned16_d(r), threadIdx.x, s);
    s.wave_fold();
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { lds[wid][0] = s.noise; lds[wid][1] = s.signal; lds[wid][2] = s.pp; lds[wid][3] = s.pr; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = lds[0][threadIdx.x];
        for (int w = 1; w < kWaves; w++) t += lds[w][threadIdx.x];
        double* o = j.chunks == 1 ? j.sums + (size_t)row * 4 : scratch + ((size_t)j.partial + local) * 4;
        o[threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void measure_rows_kernel(const MsArgs args) {
    __shared__ double lds[kWaves][4];
    uint32_t local;
    const MsJob& j = args.jobs[job_of(args, local)];
    if (j.index != nullptr) measure_job<true>(j, local, args.scratch, lds);
    else measure_job<false>(j, local, args.scratch, lds);
}

// the partials of the split rows of one launch, folded in a fixed order
struct FoldJob {
    double* sums;
    uint32_t rows, chunks, partial, pad;
};
struct FoldArgs {
    FoldJob jobs[kMsMaxJobs];
    uint32_t first_block[kMsMaxJobs];
    uint32_t count;
    const double* scratch;
};
static_assert(sizeof(FoldArgs) <= 4096, "kernel arguments are limited to 4 KB");

// one WAVE per row: lane = 4 * slot + which sum; slot s of 16 adds the partials of chunks s, s + 16, ... in order (consecutive
// lanes read consecutive doubles), then the 16 slots fold in an xor tree -- an order fixed by `chunks` alone
constexpr uint32_t kFoldSlots = kWave / 4;

__global__ __launch_bounds__(kBlock) void measure_fold_kernel(const FoldArgs args) {
    uint32_t local;
    const FoldJob& j = args.jobs[job_of(args, local)];
    const uint32_t row = local * kWaves + (threadIdx.x >> 6);
    if (row >= j.rows) return;
    const uint32_t lane = threadIdx.x & 63, slot = lane >> 2, k = lane & 3u;
    const double* part = args.scratch + ((size_t)j.partial + (size_t)row * j.chunks) * 4 + k;
    double acc = 0.0;
    for (uint32_t c = slot; c < j.chunks; c += kFoldSlots) acc += part[(size_t)c * 4];
#pragma unroll
    for (int m = 32; m >= 4; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (slot == 0) j.sums[(size_t)row * 4 + k] = acc;
}

// ---- fetch ---------------------------------------------------------------------------------------------------------
struct FtJob {                                     // 40 B
    const float* x;
    const int32_t* index;
    float* out;
    uint32_t rows, row_len, count, pieces;         // pieces = ceil(count / (4 * kBlock)) workgroups per row
};
constexpr int kFtMaxJobs = 80;
struct FtArgs {
    FtJob jobs[kFtMaxJobs];
    uint32_t first_block[kFtMaxJobs];
    uint32_t count;
};
static_assert(sizeof(FtArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBlock) void fetch_rows_kernel(const FtArgs args) {
    uint32_t local;
    const FtJob& j = args.jobs[job_of(args, local)];
    const uint32_t row = local / j.pieces, piece = local - row * j.pieces;
    const uint32_t e = (piece * kBlock + threadIdx.x) * 4u;
    if (e >= j.count) return;
    const float4 a = gather4_guarded(j.x + (size_t)row * j.row_len, j.index, e, j.count, aligned16_d(j.index), j.row_len);
    float* o = j.out + (size_t)row * j.count;
    if (e + 4 <= j.count && aligned16_d(o)) { *reinterpret_cast<float4*>(o + e) = a; return; }
    o[e] = a.x;
    if (e + 1 < j.count) o[e + 1] = a.y;
    if (e + 2 < j.count) o[e + 2] = a.z;
    if (e + 3 < j.count) o[e + 3] = a.w;
}

// ---- finish --------------------------------------------------------------------------------------------------------
struct FinArgs {
    ppqhip_measure_finish_job jobs[kMsMaxJobs];
    uint32_t count;
};
static_assert(sizeof(ppqhip_measure_finish_job) == 48, "job layout is part of the ABI");
static_assert(sizeof(FinArgs) <= 4096, "kernel arguments are limited to 4 KB");

// the per-row measure as the reference's fp32 expressions give it (measure/norm.py:42-43, :88-90; torch.cosine_similarity)
__device__ __forceinline__ float row_measure(const double* __restrict__ s, int method, double count) {
    const double noise = s[0], signal = s[1], pp = s[2], pr = s[3];
    if (method == PPQHIP_MEASURE_SNR) return (float)noise / ((float)signal + 1e-7f);
    if (method == PPQHIP_MEASURE_MSE) return (float)(noise / count);
    return (float)(pr / (fmax(sqrt(pp), 1e-8) * fmax(sqrt(signal), 1e-8)));
}

// one wave per job: lane l takes rows l, l + 64, ... in order, the lanes fold in the xor tree
__global__ __launch_bounds__(kBlock) void measure_finish_kernel(const FinArgs args) {
    const uint32_t k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= args.count) return;
    const ppqhip_measure_finish_job& j = args.jobs[__builtin_amdgcn_readfirstlane(k)];
    const uint32_t lane = threadIdx.x & 63, rows = (uint32_t)j.rows;
    double sum = 0.0;
    float top = -INFINITY;
    bool nan = false;
    for (uint32_t row = lane; row < rows; row += kWave) {
        const float v = row_measure(j.sums + (size_t)row * 4, j.method, (double)j.count);
        if (j.row_out) j.row_out[row] = v;
        sum += (double)v;
        nan = nan || v != v;
        top = fmaxf(top, v);
    }
    if (!j.acc) return;
    sum = wave_sum_f64(sum);
    top = wave_max(top);
    nan = __builtin_amdgcn_ballot_w64(nan) != 0ull;
    if (lane != 0) return;
    if (j.reduce == PPQHIP_REDUCE_MEAN) {
        const float mean = (float)(sum / (double)rows);              // torch.mean over the rows, rounded to fp32 as its result is
        j.acc[0] += (double)mean * (double)rows;
    } else {
        const double t = nan ? (double)NAN : (double)top;            // torch.max propagates NaN
        if (t > j.acc[0] || t != t) j.acc[0] = t;
    }
    j.acc[1] += (double)rows;
}

int validate_rows(int64_t rows, int64_t row_len, int64_t count, const char* what, int k) {
    if (rows <= 0 || row_len <= 0 || count <= 0) { set_error("%s: job %d is empty", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    if (row_len > 0x7fffffffLL || count > 0x7fffffffLL || rows > 0x7fffffffLL) {
        set_error("%s: job %d: more than 2^31 - 1 rows or elements per row", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

}  // namespace
}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_fetch_rows_multi(const ppqhip_fetch_rows_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (jobs == nullptr) { set_error("fetch_rows_multi: jobs is null"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_fetch_rows_job& j = jobs[k];
        if (int st = validate_rows(j.rows, j.row_len, j.count, "fetch_rows_multi", k)) return st;
        if (!j.x || !j.index || !j.out) { set_error("fetch_rows_multi: job %d has a null pointer", k); return PPQHIP_ERR_INVALID_VALUE; }
        const int64_t pieces = (j.count + 4 * kBlock - 1) / (4 * kBlock);
        if (j.rows * pieces > 0x3fffffffLL) { set_error("fetch_rows_multi: job %d: too many work items", k); return PPQHIP_ERR_INVALID_VALUE; }
        bytes += (double)j.rows * (double)j.count * 8.0 + 4.0 * (double)j.count;       // one sample in, one out; the table once
    }
    LaunchScope scope(K_FETCH_ROWS, bytes, s);
    for (int base = 0; base < num_jobs; ) {
        FtArgs args;
        uint64_t blocks = 0;
        int count = 0;
        for (; count < kFtMaxJobs && base + count < num_jobs; count++) {
            const ppqhip_fetch_rows_job& src = jobs[base + count];
            const uint32_t pieces = (uint32_t)((src.count + 4 * kBlock - 1) / (4 * kBlock));
            const uint64_t need = (uint64_t)src.rows * pieces;
            if (blocks + need > 0x7fffffffULL && count > 0) break;      // the rest goes into the next launch
            FtJob& d = args.jobs[count];
            d.x = src.x; d.index = src.index; d.out = src.out;
            d.rows = (uint32_t)src.rows; d.row_len = (uint32_t)src.row_len; d.count = (uint32_t)src.count; d.pieces = pieces;
            args.first_block[count] = (uint32_t)blocks;
            blocks += need;
        }
        for (int k = count; k < kFtMaxJobs; k++) { args.jobs[k] = args.jobs[0]; args.first_block[k] = (uint32_t)blocks; }
        args.count = (uint32_t)count;
        hipLaunchKernelGGL(fetch_rows_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
        base += count;
    }
    return finish_launch("fetch_rows_multi");
}

int ppqhip_measure_rows_multi(const ppqhip_measure_rows_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (jobs == nullptr) { set_error("measure_rows_multi: jobs is null"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_measure_rows_job& j = jobs[k];
        if (int st = validate_rows(j.rows, j.row_len, j.count, "measure_rows_multi", k)) return st;
        if (!j.p || !j.r || !j.sums) { set_error("measure_rows_multi: job %d has a null pointer", k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!j.index && j.row_len != j.count) {
            set_error("measure_rows_multi: job %d: a dense p needs row_len == count", k); return PPQHIP_ERR_INVALID_VALUE;
        }
        const int64_t chunks = (j.count + kChunk - 1) / kChunk;
        if (j.rows * chunks > 0x3fffffffLL) { set_error("measure_rows_multi: job %d: too many work items", k); return PPQHIP_ERR_INVALID_VALUE; }
        bytes += (double)j.rows * (double)j.count * 8.0 + (j.index ? 4.0 * (double)j.count : 0.0) + 32.0 * (double)j.rows;
    }
    LaunchScope scope(K_MEASURE_ROWS, bytes, s);
    for (int base = 0; base < num_jobs; ) {
        MsArgs args;
        FoldArgs fold;
        uint64_t blocks = 0, partials = 0, fold_blocks = 0;
        int count = 0, folds = 0;
        for (; count < kMsMaxJobs && base + count < num_jobs; count++) {
            const ppqhip_measure_rows_job& src = jobs[base + count];
            const uint32_t chunks = src.count <= kWaveRow ? 0u : (uint32_t)((src.count + kChunk - 1) / kChunk);
            const uint64_t need = chunks == 0 ? (uint64_t)((src.rows + kWaves - 1) / kWaves) : (uint64_t)src.rows * chunks;
            if (blocks + need > 0x7fffffffULL && count > 0) break;      // the rest goes into the next launch
            MsJob& d = args.jobs[count];
            d.p = src.p; d.r = src.r; d.index = src.index; d.sums = src.sums;
            d.rows = (uint32_t)src.rows; d.row_len = (uint32_t)src.row_len; d.count = (uint32_t)src.count; d.chunks = chunks;
            d.partial = (uint32_t)partials;
            d.index_vec = (src.index && aligned16(src.index)) ? 1u : 0u;
            d.pad0 = d.pad1 = 0;
            args.first_block[count] = (uint32_t)blocks;
            blocks += need;
            if (chunks > 1) {
                FoldJob& f = fold.jobs[folds];
                f.sums = src.sums; f.rows = d.rows; f.chunks = chunks; f.partial = d.partial; f.pad = 0;
                fold.first_block[folds++] = (uint32_t)fold_blocks;
                fold_blocks += ((uint64_t)src.rows + kWaves - 1) / kWaves;
                partials += need;
            }
        }
        for (int k = count; k < kMsMaxJobs; k++) { args.jobs[k] = args.jobs[0]; args.first_block[k] = (uint32_t)blocks; }
        args.count = (uint32_t)count;
        args.scratch = nullptr;
        if (folds > 0) {
            args.scratch = (double*)scratch(s, (size_t)partials * 4 * sizeof(double));
            if (!args.scratch) return PPQHIP_ERR_HIP;
        }
        hipLaunchKernelGGL(measure_rows_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
        if (folds > 0) {
            for (int k = folds; k < kMsMaxJobs; k++) { fold.jobs[k] = fold.jobs[0]; fold.first_block[k] = (uint32_t)fold_blocks; }
            fold.count = (uint32_t)folds;
            fold.scratch = args.scratch;
            hipLaunchKernelGGL(measure_fold_kernel, dim3((uint32_t)fold_blocks), dim3(kBlock), 0, s, fold);
        }
        base += count;
    }
    return finish_launch("measure_rows_multi");
}

int ppqhip_measure_finish_multi(const ppqhip_measure_finish_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (jobs == nullptr) { set_error("measure_finish_multi: jobs is null"); return PPQHIP_ERR_INVALID_VALUE; }
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0.0;
    for (int k = 0; k < num_jobs; k++) {
        const ppqhip_measure_finish_job& j = jobs[k];
        if (j.rows <= 0 || j.rows > 0x7fffffffLL || j.count <= 0) { set_error("measure_finish_multi: job %d is empty or too large", k); return PPQHIP_ERR_INVALID_VALUE; }
        if (!j.sums || (!j.acc && !j.row_out)) { set_error("measure_finish_multi: job %d has a null pointer", k); return PPQHIP_ERR_INVALID_VALUE; }
        if (j.method < PPQHIP_MEASURE_SNR || j.method > PPQHIP_MEASURE_COSINE || j.reduce < PPQHIP_REDUCE_MEAN || j.reduce > PPQHIP_REDUCE_MAX) {
            set_error("measure_finish_multi: job %d: unknown method %d or reduce %d", k, j.method, j.reduce); return PPQHIP_ERR_INVALID_VALUE;
        }
        bytes += (double)j.rows * (32.0 + (j.row_out ? 4.0 : 0.0)) + (j.acc ? 32.0 : 0.0);
    }
    LaunchScope scope(K_MEASURE_FINISH, bytes, s);
    for (int base = 0; base < num_jobs; base += kMsMaxJobs) {
        FinArgs args;
        const int count = std::min(kMsMaxJobs, num_jobs - base);
        for (int k = 0; k < count; k++) args.jobs[k] = jobs[base + k];
        for (int k = count; k < kMsMaxJobs; k++) args.jobs[k] = args.jobs[0];
        args.count = (uint32_t)count;
        hipLaunchKernelGGL(measure_finish_kernel, dim3((count + kWaves - 1) / kWaves), dim3(kBlock), 0, s, args);
    }
    return finish_launch("measure_finish_multi");
}

}  // extern "C"
