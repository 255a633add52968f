/*
 * ppq_hip.h -- C ABI of libppq_hip.so: MI355X (gfx950) kernels for PPQ's quantization-simulation
 * hot path.  This is the drop-in boundary: every entry point replaces one function of the
 * reference's pybind module `PPQ_Cuda_Impls` (ppq/csrc/export.cc:8-34), reached in the reference
 * through `ppq.core.ffi.CUDA.*` (ppq/core/ffi.py:56-350).  Plain pointers and sizes only; no torch
 * types.  The Python binding that presents the pybind names lives in ppq_amd/ffi.py; the stub a
 * PPQ maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers to contiguous fp32 (histograms: int32) unless a
 *     parameter is documented as host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only
 *     enqueues work on that stream and returns -- no call synchronises the device;
 *   - outputs are never aliased with inputs by the library (the reference allocates a fresh
 *     tensor, linear.cu:111); in-place use (out == x) is nevertheless safe for the elementwise ops;
 *   - return value: PPQHIP_OK (0) or a negative ppqhip_status; ppqhip_last_error() returns a
 *     thread-local message.  PPQHIP_ERR_INVALID_VALUE corresponds to the reference's
 *     InvalidValueException (common.cuh:41-48: empty tensor, numel > 0x7fffffff, bad histogram
 *     shape); dtype errors (ValueTypeException, common.cuh:32-39) cannot occur behind a typed C
 *     ABI and are raised by the Python binding instead;
 *   - `rounding` uses the values of ppq.core.RoundingPolicy (quant.py:123-142) /
 *     common.cuh:17-24: 0 HALF_EVEN, 1 HALF_UP, 2 HALF_DOWN, 3 HALF_TOWARDS_ZERO,
 *     4 HALF_FAR_FORM_ZERO, 5 TO_NEAR_INT, 6 UP, 7 DOWN;
 *   - per-channel ops address a contiguous tensor as [outer, num_channel, elem_per_channel]:
 *     channel(i) = (i / elem_per_channel) % num_channel (linear.cu:146, floating.cu:94).
 */
#ifndef PPQ_HIP_H_
#define PPQ_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PPQHIP_OK = 0,
    PPQHIP_ERR_INVALID_VALUE = -1, /* InvalidValueException, common.cuh:41-48 */
    PPQHIP_ERR_UNSUPPORTED = -2,   /* parameter combination the kernels do not implement */
    PPQHIP_ERR_HIP = -3            /* a HIP runtime call failed (launch error, bad pointer ...) */
} ppqhip_status;

#define PPQHIP_ABI_VERSION 4   /* 2: quantile hints (round 3); 3: *_multi LSQ / min-max entry points, quantile sequence (round 4);
                                * 4: ppqhip_minmax_c_multi carries its job table in the kernel arguments (no device table / upload); split per-tensor LSQ
 *    backward (ppqhip_fq_linear_t_bwd_main / ppqhip_lsq_finish_multi) (round 5); the convolution epilogues
 *    (ppqhip_bias_act / ppqhip_bias_add_act) and their statistics variants (ppqhip_bias_act_stats /
 *    ppqhip_bias_add_act_stats, then ppqhip_bias_add_act_stats2 with its elide mask and the histogram-sink
 *    forms ppqhip_bias_act_hist / ppqhip_bias_add_act_hist, then the pooled forms ppqhip_bias_act_pool /
 *    ppqhip_bias_act_pool_stats / ppqhip_bias_act_pool_hist) were ADDED under 4: no existing signature changed,
 *    and a library without them fails at load (_lib.py resolves every declared symbol) */

/* library / device introspection ------------------------------------------------------------- */
const char* ppqhip_last_error(void);
int ppqhip_version(void);                 /* ABI version == PPQHIP_ABI_VERSION; bumped on incompatible change */
int ppqhip_device_arch(char* buf, int n); /* gcnArchName of the current device, e.g. "gfx950:..." */

/* linear (integer) fake quant ---------------------------------------------------------------- */
/* replaces QuantizeTensor_LT, ppq/csrc/cuda/linear.cu:88-130 (CUDA.LinearQuantize_T ffi.py:78-90).
 * out[i] = (clip(round(x[i] / s) + round(o), qmin, qmax) - round(o)) * s ; scale/offset: 1 elem. */
int ppqhip_fq_linear_t(const float* x, const float* scale, const float* offset, float* out,
                       int64_t n, int clip_min, int clip_max, int rounding, void* stream);

/* replaces QuantizeTensor_LC, linear.cu:188-233 (CUDA.LinearQuantize_C ffi.py:92-103). */
int ppqhip_fq_linear_c(const float* x, const float* scale, const float* offset, float* out,
                       int64_t n, int64_t num_channel, int64_t elem_per_channel,
                       int clip_min, int clip_max, int rounding, void* stream);

/* quantise WITHOUT dequantising: PPQLinearQuant_toInt, ppq/quantization/qfunction/linear.py:218-238 (torch ops in the
 * reference; used when an exporter writes integer weights).  q = clamp(ppq_tensor_round(x / s) + o, qmin, qmax)
 * evaluated in float32 with the RAW offset and the float32 rounding formulas of ppq/utils/round.py:9-49, then
 * truncated to out_dtype: 0 = int8, 1 = uint8, 2 = int32 (`out` has n elements of that type).
 * ROUND_TO_NEAR_INT has no tensor form in the reference (round.py:47-49): invalid value here. */
int ppqhip_to_int_t(const float* x, const float* scale, const float* offset, void* out, int64_t n,
                    int clip_min, int clip_max, int rounding, int out_dtype, void* stream);
int ppqhip_to_int_c(const float* x, const float* scale, const float* offset, void* out, int64_t n,
                    int64_t num_channel, int64_t elem_per_channel, int clip_min, int clip_max,
                    int rounding, int out_dtype, void* stream);

/* many tensors, one launch (MI355X-native addition): every job is fake-quantised exactly as
 * ppqhip_fq_linear_c would (a per-tensor job has num_channel = 1, elem_per_channel = n).  Meant for the
 * weights of a graph, which the executor re-quantises on every forward: `jobs` is a HOST array;
 * `device_table` is caller-owned device memory of ppqhip_fq_linear_multi_table_bytes(num_jobs) bytes
 * that holds the converted job table -- pass upload = 1 on the first call and whenever a pointer or
 * shape in `jobs` changed, 0 otherwise (no host-to-device traffic on the steady path). */
typedef struct ppqhip_fq_job {
    const float* x;
    const float* scale;
    const float* offset;
    float* out;
    int64_t n, num_channel, elem_per_channel;
    int32_t clip_min, clip_max;
} ppqhip_fq_job;
int64_t ppqhip_fq_linear_multi_table_bytes(int num_jobs);
int ppqhip_fq_linear_multi(const ppqhip_fq_job* jobs, int num_jobs, int rounding, void* device_table,
                           int upload, void* stream);

/* replaces QuantizeTensor_LT_B, linear.cu:284-324 (CUDA.LinearQuantize_T_B ffi.py:105-118).
 * grad_s (1 elem) is OVERWRITTEN with sum(...) * rsqrt(n * (clip_max - clip_min)). */
int ppqhip_fq_linear_t_bwd(const float* x, const float* scale, const float* offset,
                           const float* grad_y, float* grad_x, float* grad_s, int64_t n,
                           int clip_min, int clip_max, int rounding, void* stream);

/* replaces QuantizeTensor_LC_B, linear.cu:383-433 (CUDA.LinearQuantize_C_B ffi.py:120-134).
 * grad_s (num_channel elems) is OVERWRITTEN; factor rsqrt(n * clip_max) (linear.cu:402). */
int ppqhip_fq_linear_c_bwd(const float* x, const float* scale, const float* offset,
                           const float* grad_y, float* grad_x, float* grad_s, int64_t n,
                           int64_t num_channel, int64_t elem_per_channel,
                           int clip_min, int clip_max, int rounding, void* stream);

/* The same backward in two halves, for callers that back-propagate through SEVERAL per-tensor configs in one sweep (the
 * activation delegators of a block-wise LSQ step): `_main` computes grad_x and leaves ppqhip_fq_linear_t_bwd_partials(n)
 * per-workgroup partial sums of the scale gradient in the caller-owned `partial`; ONE ppqhip_lsq_finish_multi launch at the end
 * of the sweep turns the partials of all jobs into their grad_s (OVERWRITTEN) -- each exactly as ppqhip_fq_linear_t_bwd's own
 * finish would (same lanes, same order, double accumulation: bit-identical).  Job table in the kernel arguments. */
int64_t ppqhip_fq_linear_t_bwd_partials(int64_t n);
int ppqhip_fq_linear_t_bwd_main(const float* x, const float* scale, const float* offset, const float* grad_y, float* grad_x,
                                float* partial, int64_t n, int clip_min, int clip_max, int rounding, void* stream);
typedef struct ppqhip_lsq_finish_job {
    const float* partial;     /* written by ppqhip_fq_linear_t_bwd_main for a tensor of n elements */
    float* grad_s;            /* 1 element */
    int64_t n;
    int32_t clip_min, clip_max;
} ppqhip_lsq_finish_job;
int ppqhip_lsq_finish_multi(const ppqhip_lsq_finish_job* jobs, int num_jobs, void* stream);

/* LSQ backward of MANY per-channel tensors in one launch -- what a block-wise LSQ step needs for all the weights of its
 * block (LearnedStepSizePass.finetune, optim/training.py:728-826, calls CuLSQ_LC.backward -> QuantizeTensor_LC_B once per
 * weight per step, algorithm/training.py:63-90).  Per job exactly ppqhip_fq_linear_c_bwd: grad_x and grad_s OVERWRITTEN.
 * One workgroup owns one channel: no atomics, no memset, fixed summation order (grad_x bit-identical to the per-tensor entry
 * point; grad_s too when outer == 1 and 256 <= elem_per_channel <= 4096, else equal to float-summation tolerance).
 * The job table travels in the kernel arguments (32 jobs per launch): nothing is uploaded, graph-capturable. */
typedef struct ppqhip_lsq_job {
    const float* x;
    const float* scale;
    const float* offset;
    const float* grad_y;
    float* grad_x;
    float* grad_s;
    int64_t n, num_channel, elem_per_channel;
    int32_t clip_min, clip_max;
} ppqhip_lsq_job;
int ppqhip_fq_linear_c_bwd_multi(const ppqhip_lsq_job* jobs, int num_jobs, int rounding, void* stream);

/* low-precision float (FP8 E4M3 / E5M2 / generic E,M) fake quant ------------------------------ */
/* replaces QuantizeTensor_FT, floating.cu:57-75 (CUDA.FloatingQuantize_T ffi.py:272-288);
 * scalar algorithm QuantizeScalarFloating common.cuh:154-226. */
int ppqhip_fq_float_t(const float* x, const float* scale, const float* offset, float* out,
                      int64_t n, int exponent, int mantissa, float clip_min, float clip_max,
                      int rounding, void* stream);

/* replaces QuantizeTensor_FC, floating.cu:102-131 (CUDA.FloatingQuantize_C ffi.py:290-306). */
int ppqhip_fq_float_c(const float* x, const float* scale, const float* offset, float* out,
                      int64_t n, int64_t num_channel, int64_t elem_per_channel,
                      int exponent, int mantissa, float clip_min, float clip_max,
                      int rounding, void* stream);

/* the scale search of the FP8 `floating` observer (DirectMSEObserver, observer/floating.py:88-143), batched
 * (MI355X-native addition): for every row of every job -- a job is `rows` x `row_len` contiguous floats: one row per
 * per-tensor collection, one row per channel of a weight -- and every candidate scale,
 *     out[row][c] = sum over the row of (fake_quant(x; scale = candidates[c], offset = 0) - x)^2      (double)
 * with rows numbered consecutively over the jobs.  ONE launch per 128 jobs; the caller takes the arg-min per row.
 * `jobs`, `candidates` are HOST arrays; `device_table`: ppqhip_float_scale_search_table_bytes(num_jobs) bytes of
 * device scratch; `out`: device, total_rows * num_candidates doubles. */
typedef struct ppqhip_float_search_job {
    const float* x;
    int64_t rows, row_len;
    int32_t exponent, mantissa;
    float clip_min, clip_max;
} ppqhip_float_search_job;
int64_t ppqhip_float_scale_search_table_bytes(int num_jobs);
int ppqhip_float_scale_search(const ppqhip_float_search_job* jobs, int num_jobs, const float* candidates,
                              int num_candidates, int rounding, void* device_table, double* out, void* stream);

/* many tensors, one launch (MI355X-native addition; the FP8 twin of ppqhip_fq_linear_multi): every job is
 * fake-quantised exactly as ppqhip_fq_float_c would (a per-tensor job has num_channel = 1, elem_per_channel = n).
 * Meant for the per-channel FP8 weights the TRT_FP8 policy re-quantises on every forward.  `jobs` is a HOST
 * array; `device_table` is caller-owned device memory of ppqhip_fq_float_multi_table_bytes(num_jobs) bytes; pass
 * upload = 1 on the first call and whenever a pointer, shape or format in `jobs` changed, 0 otherwise. */
typedef struct ppqhip_fq_float_job {
    const float* x;
    const float* scale;
    const float* offset;
    float* out;
    int64_t n, num_channel, elem_per_channel;
    int32_t exponent, mantissa;
    float clip_min, clip_max;
} ppqhip_fq_float_job;
int64_t ppqhip_fq_float_multi_table_bytes(int num_jobs);
int ppqhip_fq_float_multi(const ppqhip_fq_float_job* jobs, int num_jobs, int rounding, void* device_table,
                          int upload, void* stream);

/* replace QuantizeTensor_FT_B / _FC_B, floating.cu:186-221 / :286-331 (ffi.py:308-344; no
 * Python caller in the reference).  grad_s is OVERWRITTEN.  For the per-tensor form pass
 * num_channel = 1, elem_per_channel = n. */
int ppqhip_fq_float_c_bwd(const float* x, const float* scale, const float* offset,
                          const float* grad_y, float* grad_x, float* grad_s, int64_t n,
                          int64_t num_channel, int64_t elem_per_channel,
                          int exponent, int mantissa, float clip_min, float clip_max,
                          int rounding, void* stream);

/* histograms --------------------------------------------------------------------------------- */
/* replaces Histogram_T, sort.cu:91-111 (CUDA.Histogram_T ffi.py:136-145).
 * b = floor(|x| / hist_scale); b > bins-1 is dropped (clip_outliers) or clamped; hist[b] += 1.
 * ACCUMULATES into the caller's int32 hist[num_bins].
 * `workspace`: device scratch of ppqhip_hist_workspace_bytes(n, num_bins) bytes for the two-stage
 * (atomic-free) flush, or NULL to let the library use its own per-stream arena (which allocates on
 * first use and therefore cannot be used while the stream is being captured into a hipGraph). */
int64_t ppqhip_hist_workspace_bytes(int64_t n, int64_t num_bins);
int ppqhip_hist_sym_t(const float* x, int64_t n, float hist_scale, int clip_outliers,
                      int32_t* hist, int64_t num_bins, void* workspace, void* stream);

/* replaces Histogram_Asymmetric_T, sort.cu:141-165 (CUDA.Histogram_Asymmetric_T ffi.py:147-157).
 * hist_scale = (max - min) / bins; b = floor((x - min) / hist_scale). */
int ppqhip_hist_asym_t(const float* x, int64_t n, float min_value, float max_value,
                       int clip_outliers, int32_t* hist, int64_t num_bins, void* workspace,
                       void* stream);

/* replaces Histogram_C, sort.cu:187-218 (CUDA.Histogram_C ffi.py:159-169); hist is
 * [num_channel, num_bins]. */
int ppqhip_hist_sym_c(const float* x, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                      float hist_scale, int clip_outliers, int32_t* hist, int64_t num_bins,
                      void* stream);

/* MI355X-native extension: the same per-channel histogram with ONE hist_scale PER
 * CHANNEL (device float[num_channel]) -- channel c is binned exactly as ppqhip_hist_sym_t would bin the
 * slice of channel c with hist_scales[c].  Feeds the per-channel KL search the reference refuses
 * (range.py:288-289). */
int ppqhip_hist_sym_c_scales(const float* x, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                             const float* hist_scales, int clip_outliers, int32_t* hist,
                             int64_t num_bins, void* stream);
/* ... and the asymmetric rule per channel: channel c is binned exactly as ppqhip_hist_asym_t would bin the slice
 * of channel c with (mins[c], maxs[c]) (device float[num_channel] each).  Feeds the per-channel MSE search
 * (TorchMSEObserver raises on PER_CHANNEL, observer/range.py:496-497). */
int ppqhip_hist_asym_c_ranges(const float* x, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                              const float* mins, const float* maxs, int clip_outliers, int32_t* hist,
                              int64_t num_bins, void* stream);

/* order statistics ---------------------------------------------------------------------------- */
/* replaces Quantile_T, sort.cu:42-59 (CUDA.Quantile ffi.py:171-176): dest[0] = sorted[rn(n*q)],
 * dest[1] = sorted[rn(n*(1-q))], indices clamped to [0, n-1].  Never a sort, never a copy of the data: one
 * streaming pass FILTERS the keys beyond two thresholds into short lists and the order statistics are selected
 * inside them; sides the filter cannot settle go through an exact 3-pass radix select.  The result is exact
 * in every case (quantile.hip).
 * `hint`: NULL, or 8 uint32 words of caller-owned device memory, zero-initialised, that belong to ONE
 * stream of similar tensors (an observer: the same activation, batch after batch).  The library keeps the
 * thresholds that worked in it, and the next call with the same n and q skips the sampling launch that
 * otherwise estimates them (words: [0] hi valid, [1] T_hi key, [2] lo valid, [3] T_lo key, [4] n, [5] k_hi,
 * [6] k_lo, [7] calls settled from the hint; a valid word is 1 in its low byte -- bits 8-9 hold how long a list the side's next
 * threshold is aimed at, raised when a batch used the list up, see quantile.hpp).  A stale or foreign hint costs time, never correctness -- but the words belong
 * to the call until `stream` has passed it: its launches read and write them, so nothing else may touch them meanwhile.
 * One tensor WITH a hint (16-B aligned, n >= 2^18, at most 8192 wanted keys per side) takes two launches: a filter that
 * leaves every workgroup's keys in its own record, and a select that settles both sides from the records or -- no usable
 * hint yet, a list that came up short -- runs the exact radix passes itself and leaves thresholds for the next call.
 * The FIRST call this process makes on a hint address takes the general sequence (it samples its thresholds: 35 us on 6.4 MB
 * where the exact passes take 73) and leaves the hint the two launches then start from.
 * `workspace` is device scratch of ppqhip_quantile_workspace_bytes(n) bytes (>= 8.7 MB: the records and slots of that path). */
int64_t ppqhip_quantile_workspace_bytes(int64_t n);
int ppqhip_quantile_t(const float* x, int64_t n, float q, float* dest, uint32_t* hint, void* workspace,
                      void* stream);

/* many tensors, ONE launch sequence (7 launches, any number of jobs: the job table is device
 * resident): dest_k[0..1] = (q, 1-q) order statistics of job k exactly as ppqhip_quantile_t.  `jobs` is a
 * HOST array; workspace holds ppqhip_quantile_multi_workspace_bytes(num_jobs, total_elems) bytes,
 * total_elems = the sum of the jobs' n (the filter lists are sized n / 128 per job and side, 16384 keys at
 * least). */
typedef struct ppqhip_quantile_job {
    const float* x;   /* device, n floats */
    float* dest;      /* device, 2 floats */
    uint32_t* hint;   /* device, 8 words, or NULL (see ppqhip_quantile_t) */
    int64_t n;
} ppqhip_quantile_job;
int64_t ppqhip_quantile_multi_workspace_bytes(int num_jobs, int64_t total_elems);
int ppqhip_quantile_t_multi(const ppqhip_quantile_job* jobs, int num_jobs, float q, void* workspace,
                            void* stream);
/* developer aid (tools/quantile_diag.py): where a finished call left its per-job state inside `workspace` --
 * out[0] bytes before job 0's state, [1] words per job, [2] side records, [3] filter record, [4] tickets,
 * [5] byte offset of the job table, [6] / [7] word offsets of the list / tie counters in the filter record. */
void ppqhip_quantile_debug_layout(int64_t* out);
/* the same for the two-launch path of one hinted tensor (quantile_hot.hip), in uint32 words: out[0] words of the
 * whole layout, [1] first record, [2] first head, [3] first slot, [4] filter workgroups at most, [5] keys per slot, [6] first word
 * the filter does NOT zero (the header, flags and exact histograms lie below it), [7] keys per head. */
void ppqhip_quantile_hot_layout(int64_t* out);

/* replaces Isotone_T, sort.cu:61-73: dest = [max, 2nd max, min, 2nd min] (with multiplicity).
 * `workspace`: device scratch of ppqhip_quantile_workspace_bytes(n) bytes (shared sizing). */
int ppqhip_isotone_t(const float* x, int64_t n, float* dest, void* workspace, void* stream);

/* range reductions (what TorchMinMaxObserver.observe computes with torch.min/torch.max,
 * ppq/quantization/observer/range.py:86-98; no native twin in the reference) ---------------- */
/* minmax[0] = min(minmax[0], min x), minmax[1] = max(minmax[1], max x): ACCUMULATES, so the
 * caller seeds minmax with {+inf, -inf}.  NaNs are ignored.  `workspace`: device scratch of
 * ppqhip_minmax_workspace_bytes(n) bytes, or NULL (library arena; see ppqhip_hist_sym_t). */
int64_t ppqhip_minmax_workspace_bytes(int64_t n);
int ppqhip_minmax_t(const float* x, int64_t n, float* minmax, void* workspace, void* stream);

/* per channel: mins[c], maxs[c] ACCUMULATE (seed with +inf / -inf). */
int ppqhip_minmax_c(const float* x, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                    float* mins, float* maxs, void* stream);

/* per-channel min / max of MANY tensors in one launch: all the weights ParameterQuantizePass observes
 * (optim/parameters.py:156-215 -> TorchMinMaxObserver.observe per parameter, observer/range.py:99-107).  Per job exactly
 * ppqhip_minmax_c (bit-identical: min / max are order independent).  `fresh` != 0: mins / maxs are OVERWRITTEN instead of
 * accumulated (the caller need not seed them with +-inf); allowed only when n == num_channel * elem_per_channel (channel
 * axis outermost) and elem_per_channel <= 8192, i.e. one wave owns a channel -- refused otherwise.
 * The job table travels in the kernel arguments (<= 64 jobs per launch, more are chunked): no host-to-device copy, no host
 * synchronisation, legal inside a HIP-graph capture -- the tensors of a calibration forward are fresh every call. */
typedef struct ppqhip_minmax_c_job {
    const float* x;
    float* mins;
    float* maxs;
    int64_t n, num_channel, elem_per_channel;
    int32_t fresh, reserved;
} ppqhip_minmax_c_job;
int ppqhip_minmax_c_multi(const ppqhip_minmax_c_job* jobs, int num_jobs, void* stream);

/* per-channel sums in double, deterministic order: sums[c] += sum of channel c.  The DC term of
 * BiasCorrectionPass.collect_bias (ppq/quantization/optim/training.py:438-448: torch.mean over
 * every dim but the channel one); the caller divides by n / num_channel. */
int ppqhip_channel_sum(const float* x, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                       double* sums, void* stream);

/* persistent accumulators for repeated observation (MI355X-native; no twin in the reference) -----
 * An observer that sees many batches keeps one accumulator ROW per workgroup resident in HBM:
 *   rows  : int32 [ppqhip_hist_rows()][num_bins], zero-initialised by the caller
 *   slots : float [ppqhip_minmax_slots()][2],     seeded with {+inf, -inf}
 * Each launch adds into its own row / slot with plain stream-ordered read-modify-writes (no atomics,
 * no per-launch reduction kernel); *_finish folds them into hist[num_bins] (+=) / minmax[2]
 * (running min / max) once, when the statistic is needed.  Bin / range rules as above. */
int64_t ppqhip_hist_rows(void);
int ppqhip_hist_sym_t_rows(const float* x, int64_t n, float hist_scale, int clip_outliers,
                           int32_t* rows, int64_t num_bins, void* stream);
int ppqhip_hist_asym_t_rows(const float* x, int64_t n, float min_value, float max_value,
                            int clip_outliers, int32_t* rows, int64_t num_bins, void* stream);
/* many tensors, one launch: job k folds its tensor into ITS OWN slots exactly as ppqhip_minmax_t_slots.
 * `jobs` is a HOST array, copied into the kernel arguments. */
typedef struct ppqhip_minmax_job {
    const float* x;   /* device, n floats */
    float* slots;     /* device, float [ppqhip_minmax_slots()][2] */
    int64_t n;
} ppqhip_minmax_job;
int ppqhip_minmax_t_slots_multi(const ppqhip_minmax_job* jobs, int num_jobs, void* stream);

/* many tensors, one launch: every job bins its tensor into ITS OWN rows buffer exactly as
 * ppqhip_hist_sym_t_rows (asymmetric = 0: p0 = hist_scale) or ppqhip_hist_asym_t_rows
 * (asymmetric = 1: p0 = min_value, p1 = max_value) would.  `jobs` is a HOST array; it is copied into
 * the kernel arguments, so it may be reused as soon as the call returns. */
typedef struct ppqhip_hist_job {
    const float* x;   /* device, n floats */
    int32_t* rows;    /* device, int32 [ppqhip_hist_rows()][num_bins] */
    int64_t n;
    float p0, p1;
} ppqhip_hist_job;
int ppqhip_hist_t_rows_multi(const ppqhip_hist_job* jobs, int num_jobs, int asymmetric,
                             int clip_outliers, int64_t num_bins, void* stream);
int ppqhip_hist_rows_finish(const int32_t* rows, int64_t num_bins, int32_t* hist, void* stream);
/* test aid (tests/test_gpu_kernels.py: all 2^32 float patterns): the histogram kernels compute floor(a / hist_scale) from a
 * reciprocal multiply with a proven exactness test and a true-division fallback (ppq_amd/csrc/hist.hip: Binner::bins4 / bin1), where
 * the reference divides (sort.cu:84-86 / :133-135).  This runs BOTH forms of that device code on every element of x (n % 4 == 0,
 * 16-B aligned) and counts raw bin indices that differ: out[0] packed path, out[1] scalar-tail path, out[2] one offending bit
 * pattern.  `out`: device, 3 x uint64, zeroed by the caller.  asymmetric = 0: a = |x|; 1: a = x - min_value. */
int ppqhip_check_bin_rule(const float* x, int64_t n, float min_value, float hist_scale, int asymmetric, uint64_t* out, void* stream);
int64_t ppqhip_minmax_slots(void);
int ppqhip_minmax_t_slots(const float* x, int64_t n, float* slots, void* stream);
int ppqhip_minmax_slots_finish(const float* slots, float* minmax, void* stream);

/* clipping searches -------------------------------------------------------------------------- */
/* replaces compute_mse_loss, ppq/csrc/cpu/hist_mse.cc:3-28 (CUDA.compute_mse_loss ffi.py:263-270).
 * HOST function on a HOST histogram, float accumulation exactly as the reference. */
float ppqhip_mse_loss_host(const int64_t* hist, int64_t num_bins, int start, int step, int end);

/* Device-side restatement of TorchMSEObserver.hist_to_scale_offset's candidate sweep
 * (observer/range.py:456-520) for `num_hist` histograms at once.  For histogram h:
 *   hist + h*num_bins : int32[num_bins];  hist_scale[h], min_value[h] : float64 (device)
 * Candidate k's loss is accumulated sequentially in float exactly like hist_mse.cc; the first
 * minimum wins.  Writes best[h*4 + {0,1,2,3}] = {start, end, step, candidate index} (int32).
 * `symmetrical` selects the start==0 sweep (range.py:499-509).  Needs 1 <= num_bins <= 16384 and
 * 1 <= levels = quant_max - quant_min + 1; with num_bins < levels the sweep is empty (range.py:481,
 * 502) and the result is the min-max candidate {0, levels, 1, 0}.  `workspace`: device scratch of
 * ppqhip_mse_search_workspace_bytes(num_hist) bytes. */
int64_t ppqhip_mse_search_workspace_bytes(int64_t num_hist);
int ppqhip_mse_search(const int32_t* hist, int64_t num_hist, int64_t num_bins,
                      const double* hist_scale, const double* min_value,
                      int quant_min, int quant_max, int symmetrical, int32_t* best,
                      void* workspace, void* stream);

/* Device-side KL candidate losses of TorchHistObserver.hist_to_scale_offset
 * (observer/range.py:190-282, torch_KL_divergence measure/statistic.py:3-12) for `num_hist`
 * histograms at once.  losses is float64 [num_hist, num_candidates] with
 * num_candidates = ppqhip_kl_num_candidates(num_bins, num_of_bits); candidate j has
 * bin_range = (j + 1) * 2^(num_of_bits-1).  The caller picks the arg-min (the reference uses a
 * stable sort, range.py:271). */
int64_t ppqhip_kl_num_candidates(int64_t num_bins, int num_of_bits);
int ppqhip_kl_losses(const int32_t* hist, int64_t num_hist, int64_t num_bins, int num_of_bits,
                     double* losses, void* stream);

/* training helpers (exported by the reference, no caller in ppq/) ------------------------------ */
/* replace TensorClip_T / TensorClip_C, train.cu:80-113 / :35-78 (kernel + host wrapper each). */
int ppqhip_tensor_clip_t(const float* value, const float* reference, const float* limit,
                         float* out, int64_t n, void* stream);
int ppqhip_tensor_clip_c(const float* value, const float* reference, const float* limit,
                         float* out, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                         void* stream);
/* replace RoundingLoss_LT / _LC (train.cu:115-168, :220-280): out[0] is OVERWRITTEN.
 * num_channel = 0 selects the per-tensor form. */
int ppqhip_rounding_loss(const float* x, const float* scale, const float* offset, float* out,
                         int64_t n, int64_t num_channel, int64_t elem_per_channel,
                         int clip_min, int clip_max, int rounding, void* stream);
/* replace RoundingLoss_LT_B / _LC_B (train.cu:170-218, :282-338); dy is one device float. */
int ppqhip_rounding_loss_bwd(const float* x, const float* dy, const float* scale,
                             const float* offset, float* dx, int64_t n, int64_t num_channel,
                             int64_t elem_per_channel, int clip_min, int clip_max, int rounding,
                             void* stream);

/* convolution epilogues (MI355X-native addition) ------------------------------------------------ */
/* The elementwise tail of a convolution in one pass, bitwise the PyTorch sequence it replaces:
 * `conv(x, w, None)` then `+ bias[c]` (how PyTorch's MIOpen path applies a conv bias), then the graph's Add(a, b),
 * then F.relu.  Every add is one rounded fp32 add in that operand order; ReLU is clamp_min's
 * `isnan(v) ? v : max(v, 0.f)`.  Tensors are dense in the same layout; channel(i) = (i / elem_per_channel) % num_channel
 * (NCHW: num_channel = C, elem_per_channel = H*W; channels-last: C, 1).  bias vectors have num_channel elements.
 * No atomics, no synchronisation between workgroups: capturable into a HIP graph. */
/* y[i] = act(y[i] + bias[c]) in place; act = ReLU when relu != 0, identity otherwise */
int ppqhip_bias_act(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                    int relu, void* stream);
/* a[i] += bias_a[c] (stored); if bias_b: b[i] += bias_b[c] (stored), else b is read as is (identity);
 * out[i] = act(a[i] + b[i])  -- operand order of the graph's Add(a, b) */
int ppqhip_bias_add_act(float* a, const float* bias_a, float* b, const float* bias_b, float* out,
                        int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu, void* stream);

/* The same two launches for a CALIBRATION forward: what they store is what the observers observe, so every stored tensor may
 * come with a sink -- the observer's own running-range accumulator -- and the values are folded from the registers they are
 * stored from instead of being read back by the observers' end-of-forward launch.
 *   stored   bit for bit what ppqhip_bias_act / ppqhip_bias_add_act store (same arithmetic, same operand order);
 *   folded   every stored element of a tensor, once, into that tensor's slots = float[ppqhip_minmax_slots()][2], as
 *            ppqhip_minmax_t_slots accumulates them (same comparison: NaN dropped, -0.0 < +0.0).  After
 *            ppqhip_minmax_slots_finish the range equals, bit for bit, the one that entry point gives on the stored tensor;
 *            which slot a value lands in is unspecified, as it is there.
 * A null slots pointer folds nothing for that tensor; slots_b needs bias_b (else b is not stored).  Workgroup g folds into
 * slot g by plain read-modify-write: no atomics, nothing synchronises, launches on one stream accumulate in order, capturable
 * into a HIP graph.
 * Returns PPQHIP_NOT_FUSED -- NOTHING was launched and nothing is wrong -- when the kernel has no path for the call: a pointer
 * that is not 16-B aligned, n < 4, no sink at all.  The caller then runs the plain entry point and observes as before. */
#define PPQHIP_NOT_FUSED 1
int ppqhip_bias_act_stats(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                          int relu, float* slots_y, void* stream);
int ppqhip_bias_add_act_stats(float* a, const float* bias_a, float* b, const float* bias_b, float* out,
                              int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                              float* slots_a, float* slots_b, float* slots_out, void* stream);

/* Stores nothing reads.  In a calibration forward `a` and `b` of ppqhip_bias_add_act have two readers, the addition inside the
 * launch and their observers; once an observer's statistic is taken inside the launch the store has no reader left.  `elide`
 * names the tensors that are NOT stored: PPQHIP_ELIDE_A | PPQHIP_ELIDE_B (`out` is always stored).  An elided tensor is computed
 * with the same arithmetic and fed to its sink from registers; its memory keeps the convolution output it held.  An elided
 * tensor without a sink (or ELIDE_B without bias_b) is PPQHIP_ERR_INVALID_VALUE.  elide == 0: ppqhip_bias_add_act_stats. */
#define PPQHIP_ELIDE_A 1
#define PPQHIP_ELIDE_B 2
int ppqhip_bias_add_act_stats2(float* a, const float* bias_a, float* b, const float* bias_b, float* out,
                               int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                               float* slots_a, float* slots_b, float* slots_out, int elide, void* stream);

/* The histogram phase (phase 2 of KL / MSE): the sink of a stored tensor is the observer's persistent accumulator
 * int32 rows[ppqhip_hist_rows()][num_bins] with its bin rule (p0, p1) = (hist_scale, unused) or, asymmetric, (min, max) --
 * the arguments of ppqhip_hist_sym_t_rows / ppqhip_hist_asym_t_rows.  All sinks of one launch share num_bins, asymmetric and
 * clip_outliers.  Stored tensors are bit for bit the plain launches'; every stored (or elided) element of a tensor with a sink
 * is counted once, by the bin rule of those entry points (the same code), so the column sums of rows grow by exactly the
 * counts their launch would add; which row a count lands in is unspecified.  Workgroup g adds into row g by plain
 * read-modify-write: no atomics on global memory, nothing synchronises, capturable into a HIP graph.  A null rows pointer
 * counts nothing for that tensor; rows_b needs bias_b.  The sinks of one launch are DISTINCT accumulators (a workgroup reads its
 * row of each ahead and writes it back at the end): the same rows pointer twice is PPQHIP_ERR_INVALID_VALUE.  Like every
 * epilogue launch these are not booked by the profiling aid (ppqhip_prof_*), whose records name the kernels of the
 * calibration statistics proper.
 * Returns PPQHIP_NOT_FUSED (nothing launched) for: a pointer that is not 16-B aligned, relu == 0, no sink at all, tensors of
 * 2^20 elements or fewer (they stay with the observers' end-of-forward launch, which bins all of them behind one flush),
 * live sinks x num_bins above 6144 counters. */
int ppqhip_bias_act_hist(float* y, const float* bias, int64_t n, int64_t num_channel, int64_t elem_per_channel,
                         int relu, int32_t* rows_y, float p0_y, float p1_y, int64_t num_bins, int asymmetric,
                         int clip_outliers, void* stream);
int ppqhip_bias_add_act_hist(float* a, const float* bias_a, float* b, const float* bias_b, float* out,
                             int64_t n, int64_t num_channel, int64_t elem_per_channel, int relu,
                             int32_t* rows_a, float p0_a, float p1_a, int32_t* rows_b, float p0_b, float p1_b,
                             int32_t* rows_out, float p0_out, float p1_out, int64_t num_bins, int asymmetric,
                             int clip_outliers, int elide, void* stream);

/* The pooled form: Conv(bias) -> Relu -> MaxPool in one launch over contiguous NCHW, y = [n / (C * H * W), C, H, W]:
 *   pool = MaxPool2d(kernel, stride, pad)(act(y + bias[c])),  pool = [.., C, OH, OW], OH = (H + 2 pad - kernel) / stride + 1.
 * The add and the ReLU are those of ppqhip_bias_act; the pool is at::native::max_pool_forward_nchw's rule (start from -inf,
 * scan the window row by row and left to right, skip padding taps, take val when `val > maxval || isnan(val)`), so pool is bit
 * for bit F.max_pool2d(F.relu(y + bias)), signed zeros and NaN payloads included.  ppqhip_bias_act_pool also overwrites y with
 * act(y + bias[c]) as ppqhip_bias_act does.  The _stats / _hist forms feed the Relu tensor to its sink exactly as
 * ppqhip_bias_act_stats / ppqhip_bias_act_hist do (same fold, same bin rule, slot / row of workgroup g), and with
 * store_relu == 0 leave y as it was -- the convolution output: in a calibration forward the Relu tensor's readers are its
 * observer and the pool, both served inside the launch.  store_relu == 0 without a sink is PPQHIP_ERR_INVALID_VALUE.
 * Each workgroup keeps one H x W plane in LDS; no atomics on global memory, nothing synchronises between workgroups:
 * capturable into a HIP graph; not booked by the profiling aid.
 * Returns PPQHIP_NOT_FUSED (nothing launched) for: y or pool not 16-B aligned; H * W no multiple of 4; a plane that does not
 * fit a workgroup's 64 KB of LDS beside the sink's counters (num_bins * 4 B) and 4 KB of staging; kernel > 3, pad > kernel / 2
 * (PyTorch refuses those itself), dilation != 1, ceil_mode != 0; the _stats / _hist forms without a sink; _hist with relu == 0
 * or num_bins above 6144. */
int ppqhip_bias_act_pool(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height,
                         int64_t width, int relu, int kernel, int stride, int pad, int dilation, int ceil_mode,
                         void* stream);
int ppqhip_bias_act_pool_stats(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height,
                               int64_t width, int relu, int kernel, int stride, int pad, int dilation, int ceil_mode,
                               float* slots_y, int store_relu, void* stream);
int ppqhip_bias_act_pool_hist(float* y, const float* bias, float* pool, int64_t n, int64_t num_channel, int64_t height,
                              int64_t width, int relu, int kernel, int stride, int pad, int dilation, int ceil_mode,
                              int32_t* rows_y, float p0_y, float p1_y, int64_t num_bins, int asymmetric,
                              int clip_outliers, int store_relu, void* stream);

/* AdaRound (MI355X-native addition; ppq_amd/adaround.py) ------------------------------------------- */
/* One job per AdaRound weight of a block; a per-tensor job has num_channel = 1, elem_per_channel = n.  `jobs` is a HOST
 * array copied into the kernel arguments (<= 16 jobs per launch, more are chunked): no upload, capturable into a HIP graph.
 * Everything in fp32 with the rounding steps of the torch expressions they replace; clamps keep NaN.  No atomics. */
typedef struct ppqhip_adaround_job {
    const float* w;        /* weight, n floats */
    const float* v;        /* rounding parameter V, n floats */
    const float* scale;    /* num_channel floats */
    const float* offset;   /* num_channel floats, used as is (not rounded) */
    float* out;            /* forward: fake-quantised weight; backward: dV (overwritten) */
    const float* dy;       /* backward: gradient of the forward output; unused by the forward */
    int64_t n, num_channel, elem_per_channel;
    int32_t qmin, qmax;
} ppqhip_adaround_job;
/* AdaRoundDelegator.__call__, ppq/quantization/optim/legacy.py:122-132 with rectified_sigmoid :55-56:
 *   out = (clamp(floor(w / s) + clamp(sigmoid(v) * 1.2f + -0.1f, 0, 1) + o, qmin, qmax) - o) * s */
int ppqhip_adaround_fwd_multi(const ppqhip_adaround_job* jobs, int num_jobs, void* stream);
/* dV of the expression above as torch autograd computes it (legacy.py:122-132; W and the scale get no gradient), plus the
 * gradient of the regulariser AdaroundRegTerm.forward (legacy.py:58-64) scaled by the pass's gamma.  `reg`: DEVICE
 * float[3] = {k, beta, beta - 1} with k = float32(gamma) * float32(alpha) rounded to float32 and beta - 1 formed in double;
 * k == 0 means the reference's term is the integer 0 (warm-up): nothing is added. */
int ppqhip_adaround_bwd_multi(const ppqhip_adaround_job* jobs, int num_jobs, const float* reg, void* stream);

/* round tuning (MI355X-native addition; ppq_amd/roundtune.py) ---------------------------------------- */
/* One job per round-tuned weight of a block, in the launch form of the AdaRound jobs above (HOST array copied into the kernel
 * arguments, <= 16 jobs per launch, more are chunked; a per-tensor job has num_channel = 1, elem_per_channel = n). */
typedef struct ppqhip_roundtune_job {
    const float* w;        /* the pre-floored weight floor(W / s) * s, n floats */
    const float* r;        /* rounding parameter R, n floats */
    const float* scale;    /* num_channel floats */
    const float* offset;   /* num_channel floats, used as is (not rounded) */
    float* out;            /* fake-quantised weight (overwritten) */
    int64_t n, num_channel, elem_per_channel;
    int32_t qmin, qmax;
} ppqhip_roundtune_job;
/* TensorwiseRoundTuningImpl / ChannelwiseRoundTuningImpl.forward, ppq/quantization/algorithm/training.py:490-527:
 *   out = (clamp(w / s + (r > .5 ? 1 : 0) + o, qmin, qmax) - o) * s
 * w / s is the IEEE quotient and is NOT rounded to an integer (the reference does not); r NaN adds 0.  The reference's backward
 * is the identity for w and for r (:502-504), so there is no backward entry point. */
int ppqhip_roundtune_fwd_multi(const ppqhip_roundtune_job* jobs, int num_jobs, void* stream);

/* quantization error analysis (MI355X-native addition; ppq_amd/analyse.py, ppq_amd/measure.py) -------- */
/* All three take a HOST array of jobs that is copied into the kernel arguments (more jobs than fit one launch are chunked):
 * no upload, no synchronisation, no atomics, capturable into a HIP graph.  rows, row_len, count <= 2^31 - 1. */
/* batch_random_fetch (ppq/utils/fetch.py:98-122) of many tensors: out[b * count + i] = x[b * row_len + index[i]] for
 * b < rows, i < count.  `index`: DEVICE int32[count], values in [0, row_len) (a value outside is clamped into the row). */
typedef struct ppqhip_fetch_rows_job {
    const float* x;         /* rows x row_len */
    const int32_t* index;   /* count */
    float* out;             /* rows x count */
    int64_t rows, row_len, count;
} ppqhip_fetch_rows_job;
int ppqhip_fetch_rows_multi(const ppqhip_fetch_rows_job* jobs, int num_jobs, void* stream);
/* Per row b the four sums the measures of ppq/quantization/measure are made of, sums[b] = {noise, signal, pp, pr}:
 *   noise = sum (p - r)^2,  signal = sum r * r,  pp = sum p * p,  pr = sum p * r    over the count elements of the row.
 * r is dense (rows x count).  p is dense too when index == NULL (row_len == count), otherwise element i of row b is
 * p[b * row_len + index[i]]: the fetch above fused into the measure.  Each difference and product is ONE fp32 operation,
 * every accumulation a double add in an order fixed by (rows, count) alone: two calls give identical bits. */
typedef struct ppqhip_measure_rows_job {
    const float* p;
    const float* r;
    const int32_t* index;   /* NULL: p is dense */
    double* sums;           /* rows x 4, overwritten */
    int64_t rows, row_len, count;
} ppqhip_measure_rows_job;
int ppqhip_measure_rows_multi(const ppqhip_measure_rows_job* jobs, int num_jobs, void* stream);
/* The per-row measure of each job's row sums, rounded to fp32 as the reference's expressions are:
 *   snr    (float)noise / ((float)signal + 1e-7f)                       measure/norm.py:88-90
 *   mse    (float)(noise / count)                                       measure/norm.py:42-43
 *   cosine (float)(pr / (max(sqrt(pp), 1e-8) * max(sqrt(signal), 1e-8)))  torch.cosine_similarity
 * row_out (optional): float[rows], the per-row values.  acc (optional): the running state of one MeasureRecorder,
 *   mean: acc[0] += (double)(float)mean_over_rows * rows      max: acc[0] = max(acc[0], max_over_rows)      acc[1] += rows
 * The acc of the jobs of ONE call must be distinct. */
enum { PPQHIP_MEASURE_SNR = 0, PPQHIP_MEASURE_MSE = 1, PPQHIP_MEASURE_COSINE = 2 };
enum { PPQHIP_REDUCE_MEAN = 0, PPQHIP_REDUCE_MAX = 1 };
typedef struct ppqhip_measure_finish_job {
    const double* sums;     /* rows x 4, as ppqhip_measure_rows_multi writes them */
    double* acc;            /* 2 doubles, or NULL */
    float* row_out;         /* rows floats, or NULL */
    int64_t rows, count;
    int32_t method, reduce;
} ppqhip_measure_finish_job;
int ppqhip_measure_finish_multi(const ppqhip_measure_finish_job* jobs, int num_jobs, void* stream);

/* layerwise equalization (ppq_amd/equalization.py; ADDED under ABI 4 like the entries above) ---------- */
/* Both take a HOST array of jobs that is copied into the kernel arguments (chunked when it does not fit one launch): no
 * upload, no synchronisation, no atomics.  Every extent is checked on the host before anything is launched. */
/* One segment = the elements of ONE tensor that belong to the key of channel c:
 *   base[(c / div) * a + (c % div) * b + o * stride + e]   for o < outer, e < run      (all counts in floats, < 2^31)
 * `extent`: floats addressable from base (bounds check).  Covers a contiguous upstream weight row (div = 1, a = row length,
 * outer = 1), a bias / activation-maximum element (a = 1, run = 1), a column of a Gemm weight (a = 1, outer = rows, stride =
 * row length, run = 1) and the slice of a grouped downstream Conv in the reference's (cin_local, group) row order (div = G). */
typedef struct ppqhip_equalize_segment {
    const float* base;
    int64_t extent;
    int64_t div, a, b;
    int64_t outer, stride, run;
    float multiplier;        /* the key reads |x * multiplier| */
    int32_t downstream;      /* 0: the segment belongs to the upstream key, else to the downstream key */
} ppqhip_equalize_segment;
/* EqualizationPair.calculate_scale over reduce_by_axis(ABSOLUTE_MAX), ppq/quantization/algorithm/equalization.py:419-436:
 *   up / down = max |x * m| over the upstream / downstream segments (a NaN wins, as in torch.max)
 *   s = clamp(1.0f / sqrt(up / down), 0.1f, 10.0f)  (each step ONE correctly rounded fp32 operation, NaN kept by the clamp)
 *   s = 1 where up + down < value_threshold                                          scale[c] = s, c < num_channel */
typedef struct ppqhip_equalize_scale_job {
    const ppqhip_equalize_segment* segments;   /* HOST array; at least one upstream and one downstream segment */
    float* scale;                              /* num_channel floats (overwritten) */
    int32_t num_segments, num_channel;
    float value_threshold;
    int32_t reserved;
} ppqhip_equalize_scale_job;
int ppqhip_equalize_scale_multi(const ppqhip_equalize_scale_job* jobs, int num_jobs, void* stream);
/* EqualizationHelper.scale_to_upstream / scale_to_downstream (:139-198), in place on one dense tensor per job:
 *   row = i / run;  k = row % inner + (group_out ? (row / inner / group_out) * inner : 0)
 *   x[i] = divide ? x[i] / scale[k] (IEEE quotient) : x[i] * scale[k]
 * upstream [O, ...]: run = elements per output channel, inner = O; a Gemm weight stored [I, O]: run = 1, inner = O; bias: run = 1;
 * downstream Conv [O, I / G, k...]: run = prod(k), inner = I / G, group_out = O / G; downstream Gemm [O, I]: run = 1, inner = I.
 * The tensors of the jobs of ONE call must not overlap. */
typedef struct ppqhip_equalize_apply_job {
    float* x;
    const float* scale;
    int64_t n, run, inner, group_out;
    int64_t num_scale;       /* elements of scale (bounds check) */
    int32_t divide, reserved;
} ppqhip_equalize_apply_job;
int ppqhip_equalize_apply_multi(const ppqhip_equalize_apply_job* jobs, int num_jobs, void* stream);

/* channelwise split (ppq_amd/channel_split.py; ADDED under ABI 4 like the entries above) -------------- */
/* Both take a HOST array of jobs that is copied into the kernel arguments (chunked when it does not fit one launch): no
 * upload, no synchronisation, no atomics.  Every extent is checked on the host before anything is launched. */
/* The split plan of one pair, EqualizationPair.channel_split (ppq/quantization/algorithm/equalization.py:361-393) up to its mask:
 *   up / down = max |x * m| over the upstream / downstream segments, as in ppqhip_equalize_scale_job: a NaN wins
 *   split[c] = up >= value_threshold && down >= value_threshold                    (a NaN key never splits)
 *   d[c] = exclusive prefix sum of 1 + split[c];   src_of[d[c]] = c;   where split[c]: src_of[d[c] + 1] = c, bit 31 set on both
 *   *count = the new channel count.  Entries of src_of at or beyond *count are unspecified.
 * The src_of and count of the jobs of ONE call must overlap neither each other nor a segment's tensor (checked). */
typedef struct ppqhip_split_plan_job {
    const ppqhip_equalize_segment* segments;   /* HOST array; at least one upstream and one downstream segment */
    int32_t* src_of;                           /* 2 x num_channel int32 (overwritten) */
    int32_t* count;                            /* one int32 (overwritten) */
    int32_t num_segments, num_channel;
    float value_threshold;
    int32_t reserved;
} ppqhip_split_plan_job;
int ppqhip_split_plan_multi(const ppqhip_split_plan_job* jobs, int num_jobs, void* stream);
/* ChannelSplitHelper.split_by_mask (:203-220) of one dense tensor viewed as [outer, num_channel, run], OUT OF PLACE into
 * [outer, count, run] (outer = n / (num_channel * run)):
 *   out[o, d, e] = x[o, src_of[d] & 0x7fffffff, e]      times 0.70710677f -- ONE fp32 multiply -- when bit 31 of src_of[d] is set
 * upstream Conv weight / bias: outer = 1; upstream Gemm weight stored [I, O]: outer = I, run = 1; downstream Conv [O, C, k...]:
 * outer = O, run = prod(k); downstream Gemm [O, I]: outer = O, run = 1; downstream Gemm [I, O]: outer = 1, run = O.
 * `count` is what the plan wrote, read back by the host: num_channel <= count <= 2 * num_channel.  No output may overlap an
 * input (x, src_of) or another output of the same call. */
typedef struct ppqhip_split_apply_job {
    const float* x;
    float* out;              /* n / num_channel * count floats */
    const int32_t* src_of;   /* count entries are read */
    int64_t n, run;          /* n: floats of x */
    int32_t num_channel, count;
} ppqhip_split_apply_job;
int ppqhip_split_apply_multi(const ppqhip_split_apply_job* jobs, int num_jobs, void* stream);

/* SSD equalization (ppq_amd/ssd.py; ADDED under ABI 4 like the entries above) ------------------------- */
/* All three take a HOST array of jobs that is copied into the kernel arguments (chunked when it does not fit one launch): no
 * upload, no synchronisation, no atomics, capturable.  Every extent is checked on the host before anything is launched. */
/* The four candidate scales of one pair, one_step_equalization of ppq/quantization/optim/ssd.py:288-320 on the ranges of
 * prepare_weight_for_equalization (:152-210).  `first`: the key of OUTPUT channel c of the pair's first weight; `last`: the key
 * of INPUT channel c of its last weight, for a grouped Conv in the natural (group, cin_local) order (div = I / G, a = the group
 * stride, b = prod(k), outer = O / G, stride = I / G * prod(k), run = prod(k)); multiplier / downstream are not read.
 *   ranges[0][c] = max |first key|, ranges[1][c] = max |last key|          (a NaN wins, as in torch.max)
 *   scales[0][c] = clamp(sqrt(last / (first + 1e-8f)), 0.1f, 10.0f)
 *   algo 1-3: first / last floored at their max * channel_ratio, act_range floored at 0.01f;
 *             ks = max(first) / (first + 1e-8f), nks = the same of last, as = the same of act_range
 *   scales[1][c] = min(ks, as)
 *   scales[2][c] = clamp(t / min_c(t), 1.0f, 2.0f),  t = min(min(ks / nks, as / nks), 8.0f)
 *   scales[3][c] = clamp(sqrt(as * sqrt(ks / nks)), 1.0f, 2.0f)
 * Each step is ONE correctly rounded fp32 operation in that order; the cross-channel max / min are exact; NaN is kept. */
typedef struct ppqhip_ssd_scales_job {
    ppqhip_equalize_segment first, last;
    const float* act_range;  /* num_channel floats */
    float* scales;           /* 4 x num_channel floats (overwritten) */
    float* ranges;           /* 2 x num_channel floats (overwritten) */
    int32_t num_channel;
    float channel_ratio;
} ppqhip_ssd_scales_job;
int ppqhip_ssd_scales_multi(const ppqhip_ssd_scales_job* jobs, int num_jobs, void* stream);
/* write_back (:212-262) of all four candidates of one dense tensor, OUT OF PLACE (x is only read), geometry as in
 * ppqhip_equalize_apply_job:   row = i / run;  k = row % inner + (group_out ? (row / inner / group_out) * inner : 0)
 *   out[cand * n + i] = divide ? x[i] / scales[cand * num_channel + k] (IEEE quotient) : x[i] * scales[cand * num_channel + k]
 * for cand < 4.  No output may overlap an input or another output of the same call. */
typedef struct ppqhip_ssd_apply_job {
    const float* x;
    float* out;              /* 4 x n floats */
    const float* scales;     /* 4 x num_channel floats */
    int64_t n, run, inner, group_out;
    int64_t num_channel;
    int32_t divide, reserved;
} ppqhip_ssd_apply_job;
int ppqhip_ssd_apply_multi(const ppqhip_ssd_apply_job* jobs, int num_jobs, void* stream);
/* sums[b] = the four row sums of ppqhip_measure_rows_multi between p = fake_quant(y) and r (both dense rows x count), the
 * fake-quant of a linear config done in registers: channel of element e of a row = e / elem_per_channel, count == num_channel *
 * elem_per_channel (per tensor: num_channel = 1).  Bit-identical to ppqhip_fq_linear_t / _c of y (viewed as [rows, num_channel,
 * elem_per_channel]) into a buffer followed by ppqhip_measure_rows_multi on that buffer; y and r are read once, nothing else
 * is written. */
typedef struct ppqhip_fq_measure_rows_job {
    const float* y;
    const float* r;
    const float* scale;      /* num_channel floats */
    const float* offset;     /* num_channel floats */
    double* sums;            /* rows x 4, overwritten */
    int64_t rows, count;
    int64_t num_channel, elem_per_channel;
    int32_t clip_min, clip_max, rounding, reserved;
} ppqhip_fq_measure_rows_job;
int ppqhip_fq_measure_rows_multi(const ppqhip_fq_measure_rows_job* jobs, int num_jobs, void* stream);

/* statistical reports (ppq_amd/statistics.py; ADDED under ABI 4 like the entries above) ------------------ */
/* Both take a HOST array of jobs that is copied into the kernel arguments (chunked when it does not fit one launch): no
 * upload, no synchronisation, no global atomics, capturable.  A job is one float32 series of n <= 2^31 - 1 elements -- p itself
 * (r == NULL) or the differences fl32(p[i] - r[i]) -- and its record of 4-byte words in DEVICE memory:
 *   rec[0] mean  rec[1] std  rec[2] min  rec[3] max  rec[4] skewness  rec[5] kurtosis  rec[6] NOISE:SIGNAL  rec[7] 0
 *   rec[8 .. 8 + bins): int32 histogram counts                                      (bins <= 64; 0: no histogram)
 * Two calls give identical bits, whatever the alignment of p and r. */
typedef struct ppqhip_stat_job {
    const float* p;
    const float* r;          /* NULL: the series is p */
    float* rec;              /* 8 + bins words */
    int64_t n;
    int32_t bins, reserved;
} ppqhip_stat_job;
/* rec[0..3], rec[6..7].  n, mean and M2 = sum (x - mean)^2 are accumulated in double, two-pass inside a piece of 16384
 * elements, the pieces merged as (n, mean, M2) triples in a fixed order:
 *   rec[0] = (float)mean    rec[1] = (float)sqrt(M2 / (n - 1))  (NaN for n = 1, as torch.std)    rec[2], rec[3]: exact
 * With r: rec[6] = (float)sum (p - r)^2 / ((float)sum r * r + 1e-7f), torch_snr_error(p, r) (measure/norm.py:88-90), each
 * difference and product ONE fp32 operation, double adds.  Without r: rec[6] = 0. */
int ppqhip_stat_moments_multi(const ppqhip_stat_job* jobs, int num_jobs, void* stream);
/* rec[4], rec[5] and the counts, from rec[0..3] as ppqhip_stat_moments_multi wrote them (read on the device).  Every step is
 * ONE IEEE fp32 operation; the sums are double:
 *   t = (x - mean) / std;  t2 = t * t;  skewness = (float)(sum t2 * t / n);  kurtosis = (float)(sum t2 * t2 / n) - 3.0f
 *   std == 0: both NaN (analyse/graphwise.py:287-293 divides by it)
 *   lo = min, hi = max; lo == hi: lo - 1, hi + 1 (torch.histc);  pos = ((x - lo) * bins) / (hi - lo);  bin = min((int)pos, bins - 1) */
int ppqhip_stat_shape_multi(const ppqhip_stat_job* jobs, int num_jobs, void* stream);

/* OCP Microscaling (MX) block-scaled fake quant (ppq_amd/mx.py; ADDED under ABI 4 like the entries above) -- */
/* The tensor is addressed as contiguous [outer, axis_len, inner]; a block is up to 32 consecutive elements along the middle axis
 * (the last block of an axis is short when axis_len % 32 != 0 and uses only its own elements).  Per block:
 *   amax = max |v| over the FINITE elements;  se = clamp(floor(log2(amax)) - emax, -127, 127), -127 when amax == 0;  X = 2^se
 *   y = cast(v / X) * X;  cast = the nearest element value of the format (subnormals included), ties to the even encoding,
 *   saturating at +- the largest normal;  zero keeps its sign;  NaN is copied bit for bit;  +-Inf -> +- largest normal * X
 *   scale_codes (optional, NULL: not written): the E8M0 code se + 127 of every block, uint8 [outer, ceil(axis_len / 32), inner]
 * emax / largest normal: E4M3 8 / 448, E5M2 15 / 57344, E3M2 4 / 28, E2M3 2 / 7.5, E2M1 2 / 6, MXINT8 0 / 127/64 (k / 64, |k| <= 127).
 * Every step is exact in float32: two calls, and any two implementations of this contract, give identical bits.  y == x (in place)
 * is allowed; any other overlap of an output with an input or another output is refused.  Sizes of 0 launch nothing. */
enum { PPQHIP_MXFP8_E4M3 = 0, PPQHIP_MXFP8_E5M2 = 1, PPQHIP_MXFP6_E3M2 = 2, PPQHIP_MXFP6_E2M3 = 3, PPQHIP_MXFP4_E2M1 = 4,
       PPQHIP_MXINT8 = 5 };
/* The scale rule travels above the format: `format | (rule << PPQHIP_MX_RULE_SHIFT)`, in the argument of
 * ppqhip_mx_fq / ppqhip_mx_pack and in the `format` field of their jobs; the low byte alone is FLOOR, the rule written above.  With
 * a = the float32 pattern of amax, code_f = the floor code, top = the largest normal and m = the mantissa bits (MXINT8: 6):
 *   CEIL  code_f + 1 when amax * 2^(127 - code_f) > top, else code_f: amax never saturates
 *   EVEN  the floor code of the pattern a + (1 << (22 - m)): amax rounded to the element's precision first
 *   MSE   of c0 = code_f and c1 = code_f + 1 the one with the smaller sum over the block's finite elements of d * d in float64,
 *         d = cast(v / X) * X - v (exact in float32); c1 only when its sum is strictly smaller
 * every code clamped to 254: 0xFF is never made.  Cast, saturation, NaN, Inf and the all-zero block are as above with the X chosen.
 * The entry points that make no scales (unpack, gemm, conv2d and their fused forms, out_format included) refuse a rule byte, and
 * every entry point refuses a rule it does not know, before any launch. */
enum { PPQHIP_MX_RULE_SHIFT = 8 };
enum { PPQHIP_MX_FLOOR = 0, PPQHIP_MX_CEIL = 1, PPQHIP_MX_EVEN = 2, PPQHIP_MX_MSE = 3 };
int ppqhip_mx_fq(const float* x, float* y, uint8_t* scale_codes, int64_t outer, int64_t axis_len, int64_t inner, int format,
                 void* stream);
/* many tensors, one launch: every job exactly as ppqhip_mx_fq.  `jobs` is a HOST array that is copied into the kernel arguments
 * (chunked when it does not fit one launch): no upload, no synchronisation, no atomics, capturable into a HIP graph. */
typedef struct ppqhip_mx_job {
    const float* x;
    float* y;
    uint8_t* scale_codes;    /* or NULL */
    int64_t outer, axis_len, inner;
    int32_t format, reserved;
} ppqhip_mx_job;
int ppqhip_mx_fq_multi(const ppqhip_mx_job* jobs, int num_jobs, void* stream);

/* Round tuning on the MX element grid (ppq_amd/mx_roundtune.py; ADDED under ABI 4) ------------------- */
/* Per element the choice between the element value just below and just above the weight on its block's own grid; the block scale
 * is fixed.  Tensors are addressed [outer, axis_len, inner] and blocks, amax, rule and code c are exactly those of ppqhip_mx_fq
 * (`format | rule << PPQHIP_MX_RULE_SHIFT`, the MSE search included); X = 2^(c - 127), u = v * 2^(127 - c), mag = the pattern of |u|:
 *   lo       the largest element magnitude <= |u|: mag with the dropped mantissa bits cleared, on the fixed-point grid (the format's
 *            subnormals, all of MXINT8) floorf(|u| / quantum) * quantum; at most the largest normal, which also takes Inf
 *   hi       up(lo): lo + quantum on the fixed-point grid, one mantissa step above it (the carry runs into the exponent); at most
 *            the largest normal
 *   floored  (sign | lo) * X        rounding  (|u| - lo) / (hi - lo) in [0, 1) when hi > lo, else 0 (saturated): both exact
 *   a NaN element keeps its bits in floored and gets rounding 0
 * Split reads w once and writes floored, rounding and scale_codes (uint8 [outer, ceil(axis_len / 32), inner], required).
 * Forward, per element with c the block's code:  u = floored * 2^(127 - c) (exact: floored is on the grid);
 *   out = rounding > .5 ? (sign | up(|u|)) * X : floored;   a NaN rounding, a NaN element and a code of 0xFF pass floored through.
 * Its `format` carries no rule byte (the codes are given).  The backward of the forward is the identity for floored and for
 * rounding, so there is no backward entry point.  Both take a HOST array that is copied into the kernel arguments (chunked when
 * it does not fit one launch): no upload, no synchronisation, no atomics, capturable into a HIP graph.  No output may share memory
 * with any other tensor of the call; every size is checked as for ppqhip_mx_fq; sizes of 0 launch nothing. */
typedef struct ppqhip_mx_round_split_job {
    const float* w;
    float* floored;
    float* rounding;
    uint8_t* scale_codes;
    int64_t outer, axis_len, inner;
    int32_t format, reserved;
} ppqhip_mx_round_split_job;
typedef struct ppqhip_mx_round_fwd_job {
    const float* floored;
    const float* rounding;
    const uint8_t* scale_codes;
    float* out;
    int64_t outer, axis_len, inner;
    int32_t format, reserved;
} ppqhip_mx_round_fwd_job;
int ppqhip_mx_round_split_multi(const ppqhip_mx_round_split_job* jobs, int num_jobs, void* stream);
int ppqhip_mx_round_fwd_multi(const ppqhip_mx_round_fwd_job* jobs, int num_jobs, void* stream);

/* Packed MX export (ppq_amd/mx.py mx_quantize / mx_dequantize; ADDED under ABI 4) ------------------ */
/* Blocks, amax, shared exponent, cast and saturation are exactly those of ppqhip_mx_fq.  x is contiguous [outer, axis_len, inner];
 * the packed tensor is two uint8 arrays with the BLOCK AXIS LAST and every block at full size (nb = ceil(axis_len / 32)):
 *   scales    [outer, inner, nb]       the E8M0 code of each block (what ppqhip_mx_fq writes to scale_codes, transposed)
 *   elements  [outer, inner, nb * B]   B bytes per block: 32 (MXFP8, MXINT8), 24 (MXFP6), 16 (MXFP4); the elements a short last
 *                                      block lacks are encoded as +0
 * Element codes (OCP MX v1.0): floats are sign | exponent | mantissa with bias 7 (E4M3), 15 (E5M2), 3 (E3M2), 1 (E2M3), 1 (E2M1),
 * subnormals as the format defines them; MXINT8 is the two's-complement int8 k of the value k / 64.  Element i of a block occupies
 * bits [i * w, i * w + w) (w = 8, 6, 4) of the block's bytes read as one little-endian bit string: FP4 element 2i is the low nibble
 * of byte i, four FP6 elements make three bytes.  These are dense layouts; operand swizzles of particular MFMA instructions are
 * not produced.
 *   +-Inf saturates to the largest normal (the E5M2 Inf codes are never written); zero keeps its sign in the float formats, MXINT8
 *   writes 0;  NaN in MXFP8: the element is S.1111.111 (E4M3) / S.11111.11 (E5M2) with the input's sign, the scale comes from the
 *   finite elements;  NaN in MXFP6 / MXFP4 / MXINT8 (no NaN encoding): the block's scale is 0xFF (the E8M0 NaN) and its element
 *   bytes are zero.
 * Unpack: y = value(code) * 2^(scale - 127) in float32, the tail padding dropped, y contiguous [outer, axis_len, inner].  Scale 0xFF
 * makes the whole block NaN, an MXFP8 NaN code gives NaN, an E5M2 Inf code +-Inf; every NaN is 0x7fc00000, in MXFP8 with the
 * element's sign bit on top.  For inputs without NaN, unpack(pack(x)) has the bits of ppqhip_mx_fq(x) (MXINT8: -0 becomes +0).
 * All three pointers are required; no output may overlap an input or another output (there is no in-place form).  Sizes of 0
 * launch nothing.  The _multi forms take a HOST array that travels in the kernel arguments, as ppqhip_mx_fq_multi does. */
int ppqhip_mx_pack(const float* x, uint8_t* elements, uint8_t* scales, int64_t outer, int64_t axis_len, int64_t inner, int format,
                   void* stream);
typedef struct ppqhip_mx_pack_job {
    const float* x;
    uint8_t* elements;
    uint8_t* scales;
    int64_t outer, axis_len, inner;
    int32_t format, reserved;
} ppqhip_mx_pack_job;
int ppqhip_mx_pack_multi(const ppqhip_mx_pack_job* jobs, int num_jobs, void* stream);
int ppqhip_mx_unpack(const uint8_t* elements, const uint8_t* scales, float* y, int64_t outer, int64_t axis_len, int64_t inner,
                     int format, void* stream);
typedef struct ppqhip_mx_unpack_job {
    const uint8_t* elements;
    const uint8_t* scales;
    float* y;
    int64_t outer, axis_len, inner;
    int32_t format, reserved;
} ppqhip_mx_unpack_job;
int ppqhip_mx_unpack_multi(const ppqhip_mx_unpack_job* jobs, int num_jobs, void* stream);

/* GEMM on packed MX operands (ppq_amd/mx.py mx_matmul / mx_linear; ADDED under ABI 4) --------------- */
/* c[m, n] (float32, row-major) = A[m, k] . B[n, k]^T (+ bias[n]) on v_mfma_scale_f32_16x16x128_f8f6f4.  Both operands are packed
 * along their LAST axis exactly as ppqhip_mx_pack leaves them (inner == 1): elements [rows, nb * B], scales [rows, nb],
 * nb = ceil(k / 32); B as [n, k] is a Gemm weight [out, in].  a_format / b_format: any of the five float formats, independently;
 * PPQHIP_MXINT8 is not an operand type of the instruction and is refused.  The instruction receives the blocks' bytes and scale
 * codes as stored; every product of two element values is exact, every scale a power of two, the sum over k is accumulated in
 * float32 in one fixed order (no atomics, no split-K): two calls give identical bits, and for every output
 *   |c - c_float64| <= k * 2^-23 * sum_k |a_k| |b_k|      (exact wherever every partial sum is representable).
 * bias (may be NULL) is added with one float32 add per output.  An output is the quiet NaN 0x7fc00000 exactly where it sums over a
 * block whose scale code is 0xFF or over an FP8 NaN code; E5M2 Inf codes (never exported) are outside the contract.
 * Refused before any launch: MXINT8 and unknown formats, negative sizes or sizes above 2^31 - 1, null pointers (bias excepted),
 * elements or c not 16-byte aligned, c overlapping any input.  m == 0 or n == 0 launches nothing; k == 0 writes the bias (or 0). */
int ppqhip_mx_gemm(const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
                   const uint8_t* b_scales, int b_format, const float* bias, float* c, int64_t m, int64_t n, int64_t k,
                   void* stream);

/* Convolution on packed MX operands (ppq_amd/mx.py mx_conv2d / mx_conv2d_packed; ADDED under ABI 4) --- */
/* y[n, oh, ow, o] (float32: the channels-last storage of [n, o, oh, ow]) = conv2d(x[n, c, h, w], w[o, c, kh, kw]) (+ bias[o]) on
 * v_mfma_scale_f32_16x16x128_f8f6f4, as an implicit GEMM: no im2col buffer.  Both operands are packed along axis 1 exactly as
 * ppqhip_mx_pack leaves them (the block axis stored last): x elements [n, h, w, nbc * B] and scales [n, h, w, nbc], w elements
 * [o, kh, kw, nbc * B] and scales [o, kh, kw, nbc], nbc = ceil(c / 32).  The reduction runs over (ky, kx, channel block) in that
 * order, one fixed float32 accumulation order (no atomics, no split-K): two calls give identical bits, the bits of ppqhip_mx_gemm
 * on the gathered rows, and |y - y_float64| <= K * 2^-23 * sum |x| |w| with K = kh * kw * 32 * nbc.  oh = (h + 2 pad_h -
 * dil_h (kh - 1) - 1) / stride_h + 1, likewise ow; padding is symmetric and contributes exact zeros (it is not read); groups = 1.
 * An output is the quiet NaN 0x7fc00000 exactly where its window covers a block of x whose scale code is 0xFF or which holds an FP8
 * NaN code, or where its output channel of w holds one.
 * Refused before any launch: MXINT8 and unknown formats; negative sizes; sizes, n oh ow, kh kw nbc, the blocks of x or the workgroup
 * count above 2^31 - 1; kernel size, stride or dilation below 1; a window that does not fit the padded input (oh or ow < 1); null
 * pointers (bias excepted); elements or y not 16-byte aligned; y overlapping any input.  n == 0 or o == 0 launches nothing; c == 0
 * (or an input without a pixel) writes the bias (or 0). */
int ppqhip_mx_conv2d(const uint8_t* x_elements, const uint8_t* x_scales, int x_format, const uint8_t* w_elements,
                     const uint8_t* w_scales, int w_format, const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t w,
                     int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                     int64_t dil_h, int64_t dil_w, void* stream);

/* The same two with a fused epilogue (ppq_amd/mx.py residual= / relu= / out_format=; ADDED under ABI 4) ------ */
/* Operands, sizes, accumulation and NaN flags are those of ppqhip_mx_gemm / ppqhip_mx_conv2d; the K loop is the same code.  Per output,
 * in this order: v = acc + bias (bias set); v = v + residual[row, col] (residual set: float32 [m, n] row-major, for the conv
 * [n, oh, ow, o], 4-byte aligned); v = 0x7fc00000 where the row or column is NaN-flagged (the flag wins over the residual); relu != 0:
 * v = v > 0 ? v : +0 with a NaN staying a NaN (so -0 becomes +0); c / y set: v is stored as float32 in the plain call's layout;
 * out_elements / out_scales set (both or neither): v is packed in out_format along the columns (output channels) in blocks of 32,
 * out_scales [m, nbo] and out_elements [m, nbo * B], nbo = ceil(n / 32), B = 32 / 24 / 16 -- byte for byte what ppqhip_mx_pack makes
 * of the float32 [m, n] along its last axis (for the conv: of [n, o, oh, ow] along axis 1, which is the x of ppqhip_mx_conv2d): a NaN
 * gives the FP8 NaN code resp. scale 0xFF and zero element bytes for the whole block, a short last block holds +0 in the elements it
 * lacks.  out_format: one of the five float formats; it is checked even when nothing is packed.
 * Refused before any launch, beyond what the plain calls refuse: PPQHIP_MXINT8 or an unknown id as out_format; out_elements and
 * out_scales not both set or both null; no output at all (c / y and out_elements null); out_elements not 16-byte aligned (c / y as in
 * the plain call when set); more than 2^31 - 1 output blocks; an output overlapping an input (the residual included) or another
 * output.  m == 0 or n == 0 (n == 0 or o == 0) launches nothing; k == 0 (c == 0) runs the epilogue on bias (or 0) plus residual.
 * Two calls give identical bits.  Booked under "mx_gemm_fused" / "mx_conv_fused": the operands, and 4 m n bytes for each of residual
 * and c, and the packed bytes, where present. */
int ppqhip_mx_gemm_fused(const uint8_t* a_elements, const uint8_t* a_scales, int a_format, const uint8_t* b_elements,
                         const uint8_t* b_scales, int b_format, const float* bias, const float* residual, int relu, float* c,
                         uint8_t* out_elements, uint8_t* out_scales, int out_format, int64_t m, int64_t n, int64_t k, void* stream);
int ppqhip_mx_conv2d_fused(const uint8_t* x_elements, const uint8_t* x_scales, int x_format, const uint8_t* w_elements,
                           const uint8_t* w_scales, int w_format, const float* bias, const float* residual, int relu, float* y,
                           uint8_t* out_elements, uint8_t* out_scales, int out_format, int64_t n, int64_t c, int64_t h, int64_t w,
                           int64_t o, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                           int64_t dil_h, int64_t dil_w, void* stream);

/* ---- pointwise (1x1) convolution on the FP32-input MFMA (ADDED under ABI 4) ---------------------------------
 * y[n, o, oh, ow] = sum_k w[o, k] x[n, k, oh * stride, ow * stride] (+ bias[o]) for contiguous NCHW float32 x [n, c, h, wd],
 * w [o, c] (a [o, c, 1, 1] convolution weight as it lies) and y [n, o, ho, wo], ho = (h - 1) / stride + 1, wo likewise; no padding,
 * no dilation, groups = 1.  One launch on `stream`, no allocation, no synchronisation (capturable into a HIP graph); NOT booked by
 * ppqhip_prof_*.
 * Arithmetic contract: every y[n, o, p] is the float32 fmaf chain over k = 0 .. c - 1 in ASCENDING order starting from +0,
 *     acc = fmaf(w[o, k], x[n, k, src(p)], acc),
 * which is what a k-ordered sequence of v_mfma_f32_32x32x2_f32 computes bit for bit.  With a bias the stored value is acc + bias[o]
 * with one further rounding; the bias never seeds the accumulator.  There is no split-K (across waves or workgroups) and no atomic:
 * a result's bits do not depend on tile shape, grid, batch index or position in the plane, and two calls give identical bits.  NaN,
 * +-Inf and subnormals pass through as the chain gives them (-ffp-contract=off, default denormal mode).
 * Refused before any launch: a null x, w or y, a negative n or a non-positive c, h, wd or o, more than 2^31 - 1 elements in x, w or
 * y, y overlapping x, w or bias (PPQHIP_ERR_INVALID_VALUE); a stride other than 1 or 2 (PPQHIP_ERR_UNSUPPORTED).  n == 0 is
 * PPQHIP_OK with nothing launched.  Returns PPQHIP_NOT_FUSED (nothing launched, nothing wrong) for: x, w, bias or y not aligned
 * to 4 bytes.  Nothing else is required: 16-byte loads are used where stride is 1, h * wd and c are multiples of 4 and x and w are
 * 16-byte aligned, dword loads otherwise (odd planes, stride 2), by the same kernel and with the same bits. */
int ppqhip_conv1x1(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h, int64_t wd,
                   int64_t o, int64_t stride, void* stream);

/* The same GEMM with its convolution epilogue group and the calibration sinks in its store (ADDED under ABI 4).
 * The raw convolution output is never written; each output is finished in registers, in the operand order of ppqhip_bias_add_act,
 * every add a separately rounded float32 add, act = ReLU when `relu` (NaN keeps its payload) else the identity:
 *   resid == NULL             (P1):  out = act(acc + bias_a[o])
 *   resid, bias_b given       (P2b): xa = acc + bias_a[o];  r = resid + bias_b[o];  out = act(xa + r)
 *   resid given, bias_b NULL  (P2):  xa = acc + bias_a[o];  r = resid;              out = act(xa + r)
 * `resid` has the shape of `out`; only `out` is stored -- xa and the biased r exist in registers alone (PPQHIP_ELIDE_A | _B of
 * the unfused launches).  So out, and every value handed to a sink, has the bits of ppqhip_conv1x1(bias = NULL) followed by
 * ppqhip_bias_act / ppqhip_bias_add_act.  bias_a is required.
 * Sinks (`sink_kind`): dst_a takes xa, dst_r the biased r (P2b only), dst_out takes out (P1: the one tensor); NULL: no sink.
 * PPQHIP_SINK_MINMAX: each is an observer's float[ppqhip_minmax_slots()][2]; PPQHIP_SINK_HIST: each is its
 * int32[ppqhip_hist_rows()][num_bins], with (p0, p1) per sink and (num_bins, asymmetric, clip_outliers) shared, as
 * ppqhip_bias_add_act_hist takes them.  The ranges and counts are those of the unfused sink launches, as integers and bit for bit.
 * One persistent launch of at most min(tiles, 2 * CUs, max_workgroups if > 0) workgroups; workgroup g folds once, at its end, into
 * slot / row g: no global atomics, no synchronisation, capturable into a HIP graph.
 * Refused before any launch (PPQHIP_ERR_INVALID_VALUE, in this order): non-positive sizes; [a stride other than 1 or 2:
 * PPQHIP_ERR_UNSUPPORTED]; a negative max_workgroups; an unknown sink kind; [n == 0: PPQHIP_OK]; a null x, w, bias_a or out;
 * bias_b without resid; more than 2^31 - 1 elements; dst_a or dst_r without resid; dst_r without bias_b; histogram sinks with
 * num_bins outside [1, 2^31); two sinks on one accumulator; out overlapping an input (resid included).
 * Returns PPQHIP_NOT_FUSED, with NOTHING written, for: a pointer not aligned to 4 bytes; PPQHIP_SINK_NONE or no sink at all (the
 * plain forms are ppqhip_conv1x1 + ppqhip_bias_act / _add_act); histogram counters (num_bins per sink) above 3 * 2048. */
#define PPQHIP_SINK_NONE 0
#define PPQHIP_SINK_MINMAX 1
#define PPQHIP_SINK_HIST 2
int ppqhip_conv1x1_epilogue(const float* x, const float* w, const float* bias_a, const float* resid, const float* bias_b, float* out,
                            int64_t n, int64_t c, int64_t h, int64_t wd, int64_t o, int64_t stride, int relu, int sink_kind,
                            void* dst_a, void* dst_r, void* dst_out, float p0_a, float p1_a, float p0_r, float p1_r, float p0_out,
                            float p1_out, int64_t num_bins, int asymmetric, int clip_outliers, int64_t max_workgroups, void* stream);

/* profiling aid used by bench.py: when enabled, every kernel launch made through this library
 * on this thread is bracketed by hipEvents on its own stream; ppqhip_prof_collect() synchronises
 * those events and returns, per kernel id, launches / total ms / total algorithmic bytes. */
#define PPQHIP_PROF_MAX_KERNELS 48
typedef struct {
    char name[48];
    int64_t launches;
    double total_ms;
    double total_bytes;
} ppqhip_prof_entry;
int ppqhip_prof_enable(int on);
int ppqhip_prof_collect(ppqhip_prof_entry* entries, int max_entries); /* returns #entries */
/* average elapsed microseconds of `pairs` EMPTY event pairs on `stream` (the bracketing overhead
 * included in every total_ms above); negative on failure. */
double ppqhip_prof_event_overhead_us(void* stream, int pairs);

#ifdef __cplusplus
}
#endif
#endif /* PPQ_HIP_H_ */
