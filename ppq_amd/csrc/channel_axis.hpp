// channel_axis.hpp -- the geometry every entry point with (n, num_channel, elem_per_channel) in its signature shares: the tensor
// is [outer, num_channel, elem_per_channel] (NCHW: C, H*W; channels-last: C, 1; a per-tensor job: 1, n), element i lies in
// row = i / elem_per_channel and belongs to channel row % num_channel.  Used by the weight-map kernels (adaround.hip,
// roundtune.hip: map, pack and walker), the convolution epilogues (epilogue.hip: validator, pack and channel_of) and train.hip
// (channel_of).
#pragma once

#include <algorithm>
#include <cstdio>

#include "common.hpp"

namespace ppqhip {

constexpr uint32_t kAxisMaxBlocksPerJob = 1024;    // grid-strided beyond: 256 K lanes per job cover the largest weights in ~3 trips

struct ChannelAxisMap {                            // 40 B
    uint32_t n, nvec;                              // nvec: float4 count of the vector part (0: element-wise job)
    FastDiv epc, nc;                               // elem_per_channel (plane: elem_per_channel / 4), num_channel
    uint32_t plane;                                // elem_per_channel % 4 == 0: one channel per float4
    uint32_t blocks;                               // workgroups of this job
};

// k >= 0: the geometry of job k of a table (the messages then say which)
inline int validate_channel_axis(const char* what, int64_t n, int64_t num_channel, int64_t elem_per_channel, int k = -1) {
    constexpr int64_t kMax = 0x7fffffffLL;
    char job[24] = "";
    if (k >= 0) snprintf(job, sizeof(job), " job %d:", k);
    if (n <= 0 || n > kMax) {
        set_error("%s:%s n=%lld is empty or has more than 2^31 - 1 elements", what, job, (long long)n);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    if (num_channel <= 0 || elem_per_channel <= 0 || num_channel > kMax || elem_per_channel > kMax ||
        n % (num_channel * elem_per_channel) != 0) {
        set_error("%s:%s n=%lld is not [outer, %lld channels, %lld elem/channel]", what, job, (long long)n, (long long)num_channel,
                  (long long)elem_per_channel);
        return PPQHIP_ERR_INVALID_VALUE;
    }
    return PPQHIP_OK;
}

// `aligned`: every pointer the kernel accesses 16 bytes at a time is 16-B aligned
inline ChannelAxisMap pack_channel_axis(bool aligned, int64_t n, int64_t num_channel, int64_t elem_per_channel) {
    ChannelAxisMap g;
    g.n = (uint32_t)n;
    g.nvec = (aligned && n >= 4) ? (uint32_t)(n >> 2) : 0u;
    g.plane = (g.nvec > 0 && elem_per_channel % 4 == 0) ? 1u : 0u;
    g.epc = make_fastdiv((uint32_t)(g.plane ? elem_per_channel / 4 : elem_per_channel));
    g.nc = make_fastdiv((uint32_t)num_channel);
    const uint64_t work = g.nvec > 0 ? g.nvec : (uint64_t)n;
    g.blocks = (uint32_t)std::min<uint64_t>((work + kBlock - 1) / kBlock, kAxisMaxBlocksPerJob);
    return g;
}

#if defined(__HIPCC__)

// channel of element i (or, with epc = elem_per_channel / 4, of float4 i)
__device__ __forceinline__ uint32_t channel_of(uint32_t i, const FastDiv& epc, const FastDiv& nc) {
    const uint32_t row = fdiv(i, epc);
    return row - fdiv(row, nc) * nc.d;
}

// the channels of the four elements of float4 q of a vector job (g.nvec > 0): one channel_of in the plane form, four otherwise
struct Channels4 {
    uint32_t c0, c1, c2, c3;
};
__device__ __forceinline__ Channels4 channels_of_float4(const ChannelAxisMap& g, uint32_t q) {
    if (g.plane) {                                                   // g.epc holds epc / 4
        const uint32_t c = channel_of(q, g.epc, g.nc);
        return {c, c, c, c};
    }
    const uint32_t i = q * 4u;
    return {channel_of(i, g.epc, g.nc), channel_of(i + 1, g.epc, g.nc), channel_of(i + 2, g.epc, g.nc), channel_of(i + 3, g.epc, g.nc)};
}

// One job, walked by its g.blocks workgroups of kBlock lanes (`local`: this workgroup's index inside the job): elem(i, c) for
// every element of an element-wise job, else vec(q) for every float4 q and elem for the n % 4 tail, which the job's first
// workgroup takes.  The callables load and store, so each kernel keeps its operands; vec asks channels_of_float4 for its
// channels AFTER it has issued its 16-B loads -- the compiler moves no load up across that branch, and loads issued behind the
// channel arithmetic would wait for it.
template <typename Elem, typename Vec>
__device__ __forceinline__ void walk_channel_axis(const ChannelAxisMap& g, uint32_t local, Elem&& elem, Vec&& vec) {
    const uint32_t stride = g.blocks * kBlock;
    const uint32_t first = local * kBlock + threadIdx.x;
    if (g.nvec == 0) {                                               // unaligned pointers or n < 4: element-wise
        for (uint32_t i = first; i < g.n; i += stride) elem(i, channel_of(i, g.epc, g.nc));
        return;
    }
    for (uint32_t q = first; q < g.nvec; q += stride) vec(q);
    if (local == 0 && threadIdx.x < g.n - g.nvec * 4u) {              // the n % 4 tail (never in the plane form: 4 | epc | n)
        const uint32_t i = g.nvec * 4u + threadIdx.x;
        elem(i, channel_of(i, g.epc, g.nc));
    }
}

#endif  // __HIPCC__

}  // namespace ppqhip
