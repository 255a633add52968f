// epilogue_sinks.hpp -- what a convolution epilogue hands to the calibration observers, shared by every kernel that holds an
// epilogue's values in registers: epilogue.hip's statistics and pooled launches (which read the convolution output back from
// HBM) and pointwise_conv.hip's fused launch (which holds it in MFMA accumulators).  One definition of the activation, of the
// record of what one position computes and of the two sink sets, so that a value is folded / binned alike whoever computed it.
// BLOCK is the workgroup size of the kernel that uses a set (kEpStatBlock unless said otherwise).
#pragma once
#include "common.hpp"
#include "hist_bin.hpp"
#include "minmax_fold.hpp"

namespace ppqhip {

__device__ __forceinline__ float act(float v, bool relu) {
    return (relu && !__builtin_isnan(v)) ? __builtin_fmaxf(v, 0.f) : v;
}

// What one position stores (for the statistics variants): a (bias_act: y), b (BIAS_B only), out (RESID only).
template <typename T>
struct EpStored { T a, b, out; };

// One sink per stored tensor: index 0 = a (bias_act: y), 1 = b (BIAS_B only), 2 = out (RESID only); nullptr: absent.
// A sink is live when the kernel computes its tensor and the caller gave it a destination (workgroup uniform).
constexpr int kEpStatBlock = 512;              // lanes per workgroup
constexpr int kEpStatWgPerCu = 2;              // co-resident workgroups per CU: the grid cap (2 * CUs <= minmax slots, hist rows)

// Min/max sinks: slots[k] is the observer's float[minmax_slots][2]; workgroup g folds once, at its end, into slot g.
struct EpMinMaxSinks { float* slots[3]; };
template <bool RESID, bool BIAS_B>
struct EpMinMaxSet {
    using Args = EpMinMaxSinks;
    static constexpr int NS = RESID ? 3 : 1;
    bool live[NS];
    float mn[NS], mx[NS];
    __device__ __forceinline__ void init(const Args& sk, int*) {
#pragma unroll
        for (int k = 0; k < NS; k++) {
            live[k] = sk.slots[k] != nullptr && (k != 1 || BIAS_B);
            mn[k] = INFINITY; mx[k] = -INFINITY;
        }
    }
    __device__ __forceinline__ void begin() {}
    // FULL: every lane holds a value; else `in` says which do.  (`elect`: the histogram sinks' hot-bin election.)
    template <bool FULL>
    __device__ __forceinline__ void feed4(const EpStored<float4>& s, bool in, bool /*elect*/) {
        if (!FULL && !in) return;
        if (live[0]) minmax_fold4(mn[0], mx[0], s.a);
        if (RESID) {
            if (BIAS_B && live[1]) minmax_fold4(mn[1], mx[1], s.b);
            if (live[NS - 1]) minmax_fold4(mn[NS - 1], mx[NS - 1], s.out);
        }
    }
    __device__ __forceinline__ void feed1(const EpStored<float>& s, bool in) {
        if (!in) return;
        if (live[0]) minmax_fold1(mn[0], mx[0], s.a);
        if (RESID) {
            if (BIAS_B && live[1]) minmax_fold1(mn[1], mx[1], s.b);
            if (live[NS - 1]) minmax_fold1(mn[NS - 1], mx[NS - 1], s.out);
        }
    }
    __device__ __forceinline__ void finish(const Args& sk, uint32_t g, int* lds) {
        float* red = reinterpret_cast<float*>(lds);                     // 32 floats
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (!live[k]) continue;
            minmax_block_fold(mn[k], mx[k], red);
            if (threadIdx.x == 0) minmax_slot_fold(sk.slots[k] + 2 * g, mn[k], mx[k]);
            __syncthreads();                                            // red is reused by the next sink
        }
    }
};

// Histogram sinks (phase 2 of KL / MSE): rows[k] is the observer's int32[hist_rows][bins] accumulator, (a0, hs) its bin
// rule as hist.hip's launches take it (sym: 0, hist_scale; asym: min, (max - min) / bins), lds_off[k] the start of its
// counters in the workgroup's LDS (lds_ints in all).  Every value goes through hist.hip's own Binner (hist_bin.hpp: the
// same reciprocal, exactness test, true-division fallback, clip / clamp rule and hot bin), so the counts are the integers
// the observers' own launch gives.  Workgroup g adds its counters, once, at its end, into row g of every live sink with a
// plain read-modify-write (one owner per row and launch, stream ordered): no global atomics.
constexpr uint32_t kEpHistLdsInts = 3 * 2048;      // counters per workgroup: three sinks of 2048 bins, 24 KB (48 KB per CU)
struct EpHistSinks { int* rows[3]; float a0[3], hs[3]; uint32_t lds_off[3]; uint32_t lds_ints; int bins; };
template <bool RESID, bool BIAS_B, bool ASYM, bool CLIP, int BLOCK = kEpStatBlock, bool EARLY = true>
struct EpHistSet {
    using Args = EpHistSinks;
    static constexpr int NS = RESID ? 3 : 1;
    // Up to kRowRegs * BLOCK bins (2048) a lane's share of its workgroup's row is READ AT THE START of the launch and
    // kept in registers: the row has one owner per launch, and the read latency then hides behind the stream instead of
    // standing, once per launch, between the last tile and the end of the kernel.  EARLY = false (a kernel that has no
    // registers to spare for the whole launch): the same reads are issued at the head of finish(), ahead of its flush and barrier.
    static constexpr int kRowRegs = 2048 / BLOCK;
    bool live[NS];
    Binner<ASYM, CLIP, true> acc[NS];
    int* row[NS];
    int old[NS][kRowRegs];
    bool early;
    int* lds;
    uint32_t lds_ints;
    __device__ __forceinline__ void init(const Args& sk, int* l) {
        lds = l; lds_ints = sk.lds_ints;
        early = sk.bins <= kRowRegs * BLOCK;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            live[k] = sk.rows[k] != nullptr && (k != 1 || BIAS_B);
            row[k] = sk.rows[k] + (size_t)blockIdx.x * sk.bins;
            acc[k].init(l + sk.lds_off[k], sk.bins);
            acc[k].set_rule(sk.a0[k], sk.hs[k]);
        }
    }
    // Issue the row reads and zero the counters; called with the first tile's loads in flight, so the barrier is the bare
    // s_barrier behind an LDS-only wait (as in hist_persistent_kernel: __syncthreads() would also wait for those loads).
    __device__ __forceinline__ void begin() {
#pragma unroll
        for (int k = 0; k < NS; k++) {
#pragma unroll
            for (int r = 0; r < kRowRegs; r++) {
                const int b = (int)threadIdx.x + r * BLOCK;
                old[k][r] = (EARLY && early && live[k] && b <= acc[k].last) ? row[k][b] : 0;
            }
        }
        for (uint32_t i = threadIdx.x; i < lds_ints; i += BLOCK) lds[i] = 0;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    template <bool FULL>
    __device__ __forceinline__ void bin4(Binner<ASYM, CLIP, true>& a, const float4& v, bool in, bool elect) {
        int b[4];
        a.bins4(v, b);
        if (elect) a.elect(b[0], FULL || in);
        if (FULL && CLIP) a.commit4_exec(b);
        else {
            a.template commit<FULL>(b[0], in); a.template commit<FULL>(b[1], in);
            a.template commit<FULL>(b[2], in); a.template commit<FULL>(b[3], in);
        }
    }
    // every lane of the wave calls these together (the commits use wave ballots)
    template <bool FULL>
    __device__ __forceinline__ void feed4(const EpStored<float4>& s, bool in, bool elect) {
        if (live[0]) bin4<FULL>(acc[0], s.a, in, elect);
        if (RESID) {
            if (BIAS_B && live[1]) bin4<FULL>(acc[1], s.b, in, elect);
            if (live[NS - 1]) bin4<FULL>(acc[NS - 1], s.out, in, elect);
        }
    }
    __device__ __forceinline__ void bin1(Binner<ASYM, CLIP, true>& a, float v, bool in) {
        const int b = a.bin1(v);
        a.elect(b, in);
        a.template commit<false>(b, in);
    }
    __device__ __forceinline__ void feed1(const EpStored<float>& s, bool in) {
        if (live[0]) bin1(acc[0], s.a, in);
        if (RESID) {
            if (BIAS_B && live[1]) bin1(acc[1], s.b, in);
            if (live[NS - 1]) bin1(acc[NS - 1], s.out, in);
        }
    }
    __device__ __forceinline__ void finish(const Args& sk, uint32_t g, int*) {
        if (!EARLY) {
#pragma unroll
            for (int k = 0; k < NS; k++) {
#pragma unroll
                for (int r = 0; r < kRowRegs; r++) {
                    const int b = (int)threadIdx.x + r * BLOCK;
                    old[k][r] = (early && live[k] && b <= acc[k].last) ? row[k][b] : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NS; k++)
            if (live[k]) acc[k].flush_hot();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the inline-assembly ds_adds are invisible to the compiler's counters
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (!live[k]) continue;
            const int* h = acc[k].h;
            if (early) {
#pragma unroll
                for (int r = 0; r < kRowRegs; r++) {
                    const int b = (int)threadIdx.x + r * BLOCK;
                    if (b >= sk.bins) break;
                    const int c = h[b];
                    if (c) row[k][b] = old[k][r] + c;
                }
            } else {
                for (int b = threadIdx.x; b < sk.bins; b += BLOCK) {
                    const int c = h[b];
                    if (c) row[k][b] += c;
                }
            }
        }
    }
};

}  // namespace ppqhip
