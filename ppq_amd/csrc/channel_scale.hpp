// channel_scale.hpp -- which scale an element of a weight takes, shared by the two apply kernels (equalize.hip in place, ssd.hip
// four candidates out of place).  The tensor is [outer, inner, run] (grouped: outer = groups x group_out): element i lies in
// row = i / run, takes scale row % inner, and for a grouped Conv scale (row / inner / group_out) * inner + row % inner.
#pragma once

#include <algorithm>

#include "common.hpp"

namespace ppqhip {

constexpr uint32_t kScaleMaxBlocksPerJob = 1024;   // grid-strided beyond

struct ChannelScaleMap {                           // 56 B
    uint32_t n, nvec;                              // nvec: float4 count (0: 4-B accesses); then `run` holds run / 4
    FastDiv run, inner, og;
    uint32_t grouped, divide, blocks;              // blocks: workgroups of this job
};

// n / run / inner / group_out of job k and the last scale it reads; `max_n`: the entry point's bound on n
inline int validate_channel_scale(const char* what, int k, int64_t max_n, int64_t n, int64_t run, int64_t inner, int64_t group_out,
                                  int64_t num_scale) {
    constexpr int64_t kMax = 0x7fffffffLL;
    if (n <= 0 || n > max_n || run <= 0 || inner <= 0 || group_out < 0 || num_scale <= 0 || n % run != 0 || inner > kMax || group_out > kMax) {
        set_error("%s: job %d: bad geometry (n=%lld run=%lld inner=%lld group_out=%lld)", what, k, (long long)n, (long long)run,
                  (long long)inner, (long long)group_out);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    const int64_t rows = n / run;
    const int64_t last = std::min(inner, rows) - 1 + (group_out ? ((rows - 1) / inner / group_out) * inner : 0);
    if (last >= num_scale) {
        set_error("%s: job %d reads scale %lld of %lld", what, k, (long long)last, (long long)num_scale);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

// `aligned`: every pointer the kernel accesses 16 bytes at a time is 16-B aligned
inline ChannelScaleMap pack_channel_scale(bool aligned, int64_t n, int64_t run, int64_t inner, int64_t group_out, int divide) {
    ChannelScaleMap g;
    const bool vec = aligned && run % 4 == 0;
    g.n = (uint32_t)n;
    g.nvec = vec ? (uint32_t)(n >> 2) : 0u;
    g.run = make_fastdiv((uint32_t)(vec ? run / 4 : run));
    g.inner = make_fastdiv((uint32_t)inner);
    g.og = make_fastdiv((uint32_t)(group_out ? group_out : 1));
    g.grouped = group_out ? 1u : 0u; g.divide = divide ? 1u : 0u;
    const uint64_t work = vec ? g.nvec : (uint64_t)n;
    g.blocks = (uint32_t)std::min<uint64_t>((work + kBlock - 1) / kBlock, kScaleMaxBlocksPerJob);
    return g;
}

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t channel_scale_index(const ChannelScaleMap& g, uint32_t unit) {   // unit: element (or float4) index
    const uint32_t row = fdiv(unit, g.run);
    const uint32_t o = fdiv(row, g.inner);
    uint32_t k = row - o * g.inner.d;
    if (g.grouped) k += fdiv(o, g.og) * g.inner.d;
    return k;
}

#endif  // __HIPCC__

}  // namespace ppqhip
