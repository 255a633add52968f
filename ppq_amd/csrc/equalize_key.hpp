// equalize_key.hpp -- the per-channel KEY of an equalization pair, shared by the scale kernel (equalize.hip) and the split-plan
// kernel (split.hip): the packed segment (ssd.hip's ranges kernel reads it too), its host-side validation and the walk of one
// workgroup over the segments of one channel.
//   up = max |x * m| over the upstream segments, down = the same over the downstream ones (reduce_by_axis(ABSOLUTE_MAX) of
//   ppq/quantization/algorithm/equalization.py:428-436; max is order independent, a NaN wins as in torch.max).
#pragma once

#include <algorithm>
#include <cstdio>

#include "common.hpp"

namespace ppqhip {

constexpr int kEqMaxSegs = 72;                     // segments per launch (a ResNet stage pair with bias and activations has ~30)
constexpr int64_t kEqMax = 0x7fffffffLL;

struct EqSeg {                                     // 40 B
    const float* base;
    uint32_t div, a, b;                            // offset of channel c: (c / div) * a + (c % div) * b
    uint32_t outer, stride, run;
    float mult;
    uint32_t flags;                                // bit 0: downstream key; bit 1: 16-B loads (base, a, b, stride, run all 4-aligned)
};

// one segment of job k: every extent, checked against the tensor it reads.  A message names it "<side> segment", or
// "segment <t>" without a side.
inline int validate_segment(const char* what, int k, const char* side, int t, const ppqhip_equalize_segment& g, int64_t C) {
    const bool bad = g.base == nullptr || g.div < 1 || g.a < 0 || g.b < 0 || g.outer < 1 || g.run < 1 || g.stride < 0 || g.extent < 1 ||
                     g.extent > kEqMax || g.div > kEqMax || g.a > kEqMax || g.b > kEqMax || g.outer > kEqMax || g.run > kEqMax ||
                     g.stride > kEqMax || g.outer * g.run > kEqMax;
    const int64_t last = bad ? 0 : ((C - 1) / g.div) * g.a + (std::min<int64_t>(g.div, C) - 1) * g.b + (g.outer - 1) * g.stride + g.run - 1;
    if (!bad && last < g.extent) return PPQHIP_OK;
    char label[32];
    if (side) snprintf(label, sizeof(label), "%s segment", side); else snprintf(label, sizeof(label), "segment %d", t);
    if (bad) set_error("%s: job %d %s: bad geometry", what, k, label);
    else set_error("%s: job %d %s: reads element %lld of a tensor of %lld", what, k, label, (long long)last, (long long)g.extent);
    return PPQHIP_ERR_INVALID_VALUE;
}

// the segments of job k: each one as above; at least one upstream and one downstream segment
inline int validate_segments(const char* what, int k, const ppqhip_equalize_segment* segments, int num_segments, int64_t C) {
    if (num_segments > kEqMaxSegs) {
        set_error("%s: job %d: %d segments, at most %d fit one launch", what, k, num_segments, kEqMaxSegs);
        return PPQHIP_ERR_UNSUPPORTED;
    }
    bool has_up = false, has_down = false;
    for (int t = 0; t < num_segments; t++) {
        if (int st = validate_segment(what, k, nullptr, t, segments[t], C)) return st;
        (segments[t].downstream ? has_down : has_up) = true;
    }
    if (!has_up || !has_down) { set_error("%s: job %d needs an upstream and a downstream segment", what, k); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

inline EqSeg pack_segment(const ppqhip_equalize_segment& g) {
    EqSeg e;
    e.base = g.base; e.div = (uint32_t)g.div; e.a = (uint32_t)g.a; e.b = (uint32_t)g.b;
    e.outer = (uint32_t)g.outer; e.stride = (uint32_t)g.stride; e.run = (uint32_t)g.run; e.mult = g.multiplier;
    const bool vec = aligned16(g.base) && g.run % 4 == 0 && g.a % 4 == 0 && g.b % 4 == 0 && g.stride % 4 == 0;
    e.flags = (g.downstream ? 1u : 0u) | (vec ? 2u : 0u);
    return e;
}

#if defined(__HIPCC__)

// One workgroup of kBlock lanes folds the `seg_count` segments of channel c: lanes stride over the channel's elements of every
// segment, then wave64 shuffle + LDS (`lds`: 4 * kBlock / kWave floats).  up / down are valid on thread 0 alone; a side that
// met a NaN is NaN.
__device__ __forceinline__ void eq_channel_keys(const EqSeg* segs, uint32_t seg_count, uint32_t c, float* lds, float& up, float& dn) {
    float key[2] = {0.f, 0.f}, bad[2] = {0.f, 0.f};                       // [0] upstream, [1] downstream; |x| >= 0, so 0 is neutral
    for (uint32_t k = 0; k < seg_count; k++) {
        const EqSeg& g = segs[k];
        const uint32_t q = c / g.div;
        const float* p = g.base + (size_t)q * g.a + (size_t)(c - q * g.div) * g.b;
        const float mult = g.mult;
        float m = 0.f, nan = 0.f;
        auto fold = [&](float x) {
            const float t = __builtin_fabsf(x * mult);
            m = fmaxf(m, t);                                               // drops a NaN operand: tracked on its own
            nan = (t != t) ? 1.f : nan;
        };
        if (g.flags & 2u) {
            const uint32_t run4 = g.run >> 2, total = g.outer * run4;
            for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
                const uint32_t o = (g.outer == 1) ? 0u : i / run4, e = i - o * run4;
                const float4 v = reinterpret_cast<const float4*>(p + (size_t)o * g.stride)[e];
                fold(v.x); fold(v.y); fold(v.z); fold(v.w);
            }
        } else {
            const uint32_t total = g.outer * g.run;
            for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
                const uint32_t o = (g.outer == 1) ? 0u : (g.run == 1 ? i : i / g.run), e = i - o * g.run;
                fold(p[(size_t)o * g.stride + e]);
            }
        }
        const uint32_t side = g.flags & 1u;                                // wave-uniform
        key[side] = fmaxf(key[side], m);
        bad[side] = fmaxf(bad[side], nan);
    }
    up = wave_max(key[0]); dn = wave_max(key[1]);
    float up_nan = wave_max(bad[0]), dn_nan = wave_max(bad[1]);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { lds[4 * wid] = up; lds[4 * wid + 1] = dn; lds[4 * wid + 2] = up_nan; lds[4 * wid + 3] = dn_nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; w++) {
            up = fmaxf(up, lds[4 * w]); dn = fmaxf(dn, lds[4 * w + 1]);
            up_nan = fmaxf(up_nan, lds[4 * w + 2]); dn_nan = fmaxf(dn_nan, lds[4 * w + 3]);
        }
        if (up_nan > 0.f) up = __builtin_nanf("");
        if (dn_nan > 0.f) dn = __builtin_nanf("");
    }
}

#endif  // __HIPCC__

}  // namespace ppqhip
