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
// Job tables: DESIGN.md, "Job tables" (a first use of the split path on a stream grows its scratch: run it once eagerly before
// capturing, as for the other scratch users).
// The row-sum machinery itself (job layout, guarded loads, Sums4, the walk of a row piece) lives in measure_rows.hpp, which
// ssd.hip shares for its fake-quant-and-measure launch.
#include <algorithm>

#include "common.hpp"
#include "job_table.hpp"
#include "measure_rows.hpp"

namespace ppqhip {
namespace {

struct MsArgs {
    MsJob jobs[kMsMaxJobs];
    uint32_t first_block[kMsMaxJobs];
    uint32_t count;
    double* scratch;
};
static_assert(sizeof(MsArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBlock) void measure_rows_kernel(const MsArgs args) {
    __shared__ double lds[kWaves][4];
    uint32_t local;
    const MsJob& j = args.jobs[job_of(args, local)];
    if (j.index != nullptr) measure_job<true>(j, local, args.scratch, lds, MsIdentity());
    else measure_job<false>(j, local, args.scratch, lds, MsIdentity());
}

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

}  // namespace

void launch_measure_fold(const FoldArgs& fold, uint32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(measure_fold_kernel, dim3(blocks), dim3(kBlock), 0, s, fold);
}

}  // namespace ppqhip

using namespace ppqhip;

extern "C" {

int ppqhip_fetch_rows_multi(const ppqhip_fetch_rows_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (int st = check_job_table("fetch_rows_multi", jobs, num_jobs)) return st;
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
        pad_job_table(args, (uint32_t)count, (uint32_t)blocks);
        hipLaunchKernelGGL(fetch_rows_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
        base += count;
    }
    return finish_launch("fetch_rows_multi");
}

int ppqhip_measure_rows_multi(const ppqhip_measure_rows_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (int st = check_job_table("measure_rows_multi", jobs, num_jobs)) return st;
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
        pad_job_table(args, (uint32_t)count, (uint32_t)blocks);
        args.scratch = nullptr;
        if (folds > 0) {
            args.scratch = (double*)scratch(s, (size_t)partials * 4 * sizeof(double));
            if (!args.scratch) return PPQHIP_ERR_HIP;
        }
        hipLaunchKernelGGL(measure_rows_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, args);
        if (folds > 0) {
            pad_job_table(fold, (uint32_t)folds, (uint32_t)fold_blocks);
            fold.scratch = args.scratch;
            hipLaunchKernelGGL(measure_fold_kernel, dim3((uint32_t)fold_blocks), dim3(kBlock), 0, s, fold);
        }
        base += count;
    }
    return finish_launch("measure_rows_multi");
}

int ppqhip_measure_finish_multi(const ppqhip_measure_finish_job* jobs, int num_jobs, void* stream) {
    if (num_jobs <= 0) return PPQHIP_OK;
    if (int st = check_job_table("measure_finish_multi", jobs, num_jobs)) return st;
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
