// measure_rows.hpp -- the row-sum machinery of measure.hip, shared with ssd.hip (ppqhip_fq_measure_rows_multi): the job layout,
// the guarded loads, the four double sums and the walk of one row piece.  The arithmetic contract and the size-dependent paths are
// described at the head of measure.hip; every user of this header produces sums in EXACTLY that order.
//
// `XF` is applied to the four p values of a float4 slot before they are summed: `xf(a, e, valid)` with e = the index of a.x in
// its ROW and valid = how many of the four slots exist (<= 0: none).  A transform must hand back 0 in the slots that do not
// exist -- they then add +0.0 to every sum, as the guarded loads make them do.  MsIdentity is the plain measure.
#pragma once

#include "common.hpp"

namespace ppqhip {

constexpr int kMsMaxJobs = 56;                     // 56 x (64 + 4) B of job table: inside the 4 KB of kernel arguments
constexpr uint32_t kWaveRow = 1024;                // rows up to here: one wave each (<= 4 float4 per lane)
constexpr uint32_t kChunk = 8192;                  // elements per workgroup: 8 float4 of p and of r per lane (16384 and 32768
                                                   // measured the same on ResNet-50's outputs: profiles/r09_analyse.txt)
constexpr int kWaves = kBlock / kWave;

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

// the partials of the split rows of one launch, folded in a fixed order (measure.hip: measure_fold_kernel)
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
void launch_measure_fold(const FoldArgs& fold, uint32_t blocks, hipStream_t s);         // measure.hip

#if defined(__HIPCC__)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ bool aligned16_d(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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

struct MsIdentity {
    __device__ __forceinline__ float4 operator()(const float4& a, uint32_t, int) const { return a; }
};

// elements [0, len) of one row piece over LANES lanes (lane = this thread's index among them), U float4 pairs in flight;
// `base`: the index in its row of the piece's first element (what XF is told)
template <int LANES, int U, bool GATHER, typename XF>
__device__ __forceinline__ void sum_piece(const float* __restrict__ p, const float* __restrict__ r, const int32_t* __restrict__ index,
                                          uint32_t len, uint32_t row_len, bool p_vec, bool r_vec, uint32_t lane, Sums4& s,
                                          const XF& xf, uint32_t base) {
    for (uint32_t e0 = lane * 4u; e0 < len; e0 += 4u * LANES * U) {
        float4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t e = e0 + 4u * LANES * u;
            a[u] = GATHER ? gather4_guarded(p, index, e, len, p_vec, row_len) : load4_guarded(p, e, len, p_vec);
            b[u] = load4_guarded(r, e, len, r_vec);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t e = e0 + 4u * LANES * u;
            s.add4(xf(a[u], base + e, (int)len - (int)e), b[u]);
        }
    }
}

template <bool GATHER, typename XF>
__device__ __forceinline__ void measure_job(const MsJob& j, uint32_t local, double* __restrict__ scratch, double (*lds)[4],
                                            const XF& xf) {
    Sums4 s = {0.0, 0.0, 0.0, 0.0};
    if (j.chunks == 0) {                                              // one wave per row
        const uint32_t row = local * kWaves + (threadIdx.x >> 6);
        if (row >= j.rows) return;
        const float* r = j.r + (size_t)row * j.count;
        const float* p = j.p + (size_t)row * j.row_len;
        sum_piece<kWave, 4, GATHER>(p, r, j.index, j.count, j.row_len, GATHER ? j.index_vec != 0 : aligned16_d(p), aligned16_d(r),
                                    threadIdx.x & 63, s, xf, 0u);
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
                                 GATHER ? j.index_vec != 0 : aligned16_d(p), aligned16_d(r), threadIdx.x, s, xf, begin);
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

#endif  // __HIPCC__

// rows, row_len, count of one job (shared by the entry points that take rows)
inline int validate_rows(int64_t rows, int64_t row_len, int64_t count, const char* what, int k) {
    if (rows <= 0 || row_len <= 0 || count <= 0) { set_error("%s: job %d is empty", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    if (row_len > 0x7fffffffLL || count > 0x7fffffffLL || rows > 0x7fffffffLL) {
        set_error("%s: job %d: more than 2^31 - 1 rows or elements per row", what, k); return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

}  // namespace ppqhip
