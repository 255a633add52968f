// quantile.hpp -- what the two quantile paths share: the general multi-job sequence (quantile.hip) and the two-launch path of
// ONE hinted tensor (quantile_hot.hip).
//
// ---- the hint: words and state machine ---------------------------------------------------------------------------------
// A hint is 8 uint32 words of caller-owned device memory that belong to one stream of similar tensors (ppq_hip.h); all zero = no
// knowledge.  Words: [0] hi valid, [1] T_hi key, [2] lo valid, [3] T_lo key, [4] n, [5] k_hi, [6] k_lo, [7] calls settled from the
// hint.  A side is usable when the low byte of its valid word is 1 and words 4-6 match the call (every path checks all of them).
//
//   who writes     select A of the general sequence (every side it decides: keep / drop, the threshold it used, words 4-6, word
//                  7 + 1 when the hint settled the hi side); F2's tail (the threshold it computes, below); F3's tail (a heavy tie);
//                  in the two-launch path the OWNER of each side in quantile_hot_select_kernel (the hi side's owner also words
//                  4-7).  Nothing else touches the words while the call's launches are in flight.
//   level          Bits 8-9 of a valid word: how long a list the side's NEXT threshold is aimed at (quantile_hot.hip: qh_target).
//                  The wanted keys sit 3.7 sigma out (q = 0.9999): the number of keys beyond a FIXED threshold moves with the 14th
//                  power of the activation's scale, so a list of 1.5 x the wanted keys -- the shortest, fastest choice: six keys
//                  per filter workgroup, inline in the records -- is used up by a batch whose scale is 3 % smaller, and the call
//                  then pays the exact passes (5 % jitter between batches -> one call in three, 31 us per call instead of 10.7).
//                  Level 0 aims at 1.5 x wanted, level 3 at the geometric middle of [wanted, what the select holds in registers]
//                  (as much room below as above), 1 and 2 in between.  Only the two-launch path sets it: a call the hint could not
//                  settle raises the side to level 3, a list that came within a quarter of failing raises it by one, every 64th
//                  settled call lowers it by one -- a stationary stream works with the short lists, a restless one with the long
//                  ones.  The general sequence writes valid words of 1 (level 0) and ignores bits 8-9 when it reads them.
//   first call     The first call this process makes on a hint ADDRESS takes the general sequence (quantile_hint_met_before,
//                  quantile_hot.hip): such a hint is almost always fresh (an observer's first batch), and the two-launch path has
//                  only its exact passes for a tensor without usable thresholds -- 73 us on B / 221 us on B x 32 where the sequence
//                  (sample, thresholds, filter, select) takes 35 / 73 us and leaves the same kind of hint behind.  The memo only
//                  chooses between two exact paths: an address met again after its tensor was freed and zeroed costs one call of
//                  exact passes, a valid hint met for the first time (written by the multi-tensor entry point) one call of the
//                  sequence from its hint.  Every later call with one tensor takes the two launches.
//   re-centring    A side settled by its list keeps the hint.  Select A keeps it only while the list is neither nearly too short
//                  (count - wanted >= wanted / 8 + 8) nor longer than q_list_limit, and keeps its threshold.  The two-launch path
//                  keeps every settled side and re-centres its threshold on this batch, so that the next list holds what
//                  qh_target asks for at the side's level (dropping a hint costs three exact passes on the next batch there).
//                  A side settled on the tie value itself keeps its level.
//   after F2 / F3  A side the lists could not settle goes through the exact passes, which leave a hint that works: F2's rule -- a
//                  threshold with an exactly known number of keys beyond it, about the target (1.5 x wanted + 32 in the sequence,
//                  qh_target at the side's level in the two-launch path) and at most q_list_limit; F3's
//                  rule -- the threshold ON the answer when its exact multiplicity is heavy (mult / 16 >= wanted + 16: one key in
//                  eight is counted as a tie), so select A settles it from the tie count next time.  The two-launch path applies
//                  both rules after its own exact passes and gives the side level 3 when a usable hint failed it.
#pragma once
#include <cmath>
#include "common.hpp"
#include "stream_walk.hpp"

namespace ppqhip {

// order-preserving key: ascending uint32 order == ascending float order
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// (explicit unsigned min / max: `max` resolves to the int overload in the host pass of this translation unit)
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
// Wave64 inclusive scan / reductions on the DPP path (row_shr 1,2,4,8 inside each row of 16 lanes, then row_bcast 15 / 31 across
// the rows): six VALU instructions.  The __shfl_up / __shfl_xor forms compile to ds_bpermute_b32 -- a ~120-cycle LDS-crossbar round
// trip each, and a scan is six of them in a dependent chain.
template <typename Op>
__device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t v, const uint32_t identity, Op op) {
#define PPQ_DPP(ctrl, rows) (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, ctrl, rows, 0xf, false)
    v = op(v, PPQ_DPP(0x111, 0xf));        // row_shr:1
    v = op(v, PPQ_DPP(0x112, 0xf));        // row_shr:2
    v = op(v, PPQ_DPP(0x114, 0xf));        // row_shr:4
    v = op(v, PPQ_DPP(0x118, 0xf));        // row_shr:8
    v = op(v, PPQ_DPP(0x142, 0xa));        // row_bcast:15 into rows 1 and 3
    v = op(v, PPQ_DPP(0x143, 0xc));        // row_bcast:31 into rows 2 and 3
#undef PPQ_DPP
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) { return wave_scan_dpp(v, 0u, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_all_min(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_dpp(v, 0xFFFFFFFFu, [](uint32_t a, uint32_t b) { return a < b ? a : b; }), 63);
}
__device__ __forceinline__ uint32_t wave_all_max(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_dpp(v, 0u, [](uint32_t a, uint32_t b) { return a > b ? a : b; }), 63);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(v), 63); }
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return wave_all_min(v); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_all_max(v); }
__device__ __forceinline__ int popc_mask(unsigned long long m) {
    return __builtin_popcount((unsigned)m) + __builtin_popcount((unsigned)(m >> 32));
}

// the hint's words (the state machine: top of this file)
enum { kHValidHi = 0, kHTHi = 1, kHValidLo = 2, kHTLo = 3, kHN = 4, kHKHi = 5, kHKLo = 6, kHUses = 7 };

// radix digits of a key: 12 + 12 + 8 bits (F1 / F2 / F3 of the general sequence, the three exact levels of the two-launch path)
constexpr int kQ1 = 4096, kQ2 = 4096, kQ3 = 256;
constexpr int kQTrash = 64;                 // per-lane trash counters behind an LDS histogram (HotCounter)
constexpr int64_t kQSpeculateMinElems = 1ll << 18;   // smaller sequences go straight to F1..F3; smaller hinted tensors take the sequence

// capacity (keys per side) of a job's filter lists; they live behind the fixed parts of all jobs
__host__ __device__ inline uint32_t quantile_spec_cap(uint64_t n) {
    uint64_t c = n / 128;
    if (c < 16384) c = 16384;
    if (c > (1u << 20)) c = 1u << 20;
    return (uint32_t)((c + 31) & ~31ull);           // lists and their 8 segments stay 16-B aligned
}
// the longest list a hint may keep producing: a few thousand keys cost select A nothing, whatever multiple of `wanted`
__device__ __forceinline__ uint32_t q_list_limit(uint32_t wanted, uint32_t cap) { return umin(cap / 2u, umax(16u * wanted + 1024u, 8192u)); }

// Tensor pointers come out of the device-resident job table, so the compiler cannot tell they are global memory and would
// emit FLAT loads -- which tick both vmcnt and lgkmcnt and return out of order with LDS traffic, so every wait becomes
// vmcnt(0) and the ping-pong prefetch of the streaming loops is lost.  These loads name the address space.
typedef __attribute__((address_space(1))) const v4f* gv4f_ptr;
typedef __attribute__((address_space(1))) const float* gf32_ptr;
template <bool NT>
__device__ __forceinline__ float4 gload4(const float4* p) {
    gv4f_ptr g = (gv4f_ptr)p;
    const v4f t = NT ? __builtin_nontemporal_load(g) : *g;
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float gload1(const float* p) { return *(gf32_ptr)p; }
template <bool NT>
struct GlobalLoads {                // how the filters' walks read (stream_walk.hpp)
    static __device__ __forceinline__ float4 v4(const float4* p) { return gload4<NT>(p); }
    static __device__ __forceinline__ float v1(const float* p) { return gload1(p); }
};

// ---- block-wide helpers (THREADS = blockDim.x, a multiple of 64) --------------------------------------------------
// exclusive prefix of v over the workgroup + the total; scratch: THREADS / 64 words.  All threads call this.
template <int THREADS>
__device__ __forceinline__ void block_scan_excl(uint32_t v, uint32_t* scratch, uint32_t& excl, uint32_t& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t inc = wave_scan_add(v);
    __syncthreads();                  // scratch may still be read from a previous call
    if (lane == 63) scratch[wid] = inc;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) {
        const uint32_t s = scratch[w];
        woff += w < wid ? s : 0u;
        tot += s;
    }
    excl = woff + inc - v;
    total = tot;
}

// find the bin of `hist[0..nbins)` that holds rank k (0-based) and the rank inside it; nbins in {256, 4096}, THREADS threads:
// thread t owns `per` consecutive bins (threads past the last bin own none).  Result: sel[0], sel[1] (LDS), valid after
// the call for every thread.  scratch: THREADS / 64 words.
template <int THREADS>
__device__ void select_bin(const uint32_t* __restrict__ hist, int nbins, uint32_t k, uint32_t* scratch, uint32_t* sel) {
    constexpr int kMaxPer = kQ1 / THREADS;                          // 16 (256 threads) or 4 (1024)
    const int per = nbins >= THREADS ? nbins / THREADS : 1;
    const int t = threadIdx.x;
    const bool owner = t * per < nbins;
    uint32_t mine[kMaxPer];
    uint32_t local = 0;
#pragma unroll
    for (int j = 0; j < kMaxPer; j++) {
        mine[j] = (owner && j < per) ? hist[t * per + j] : 0u;
        local += mine[j];
    }
    uint32_t excl, total;
    block_scan_excl<THREADS>(local, scratch, excl, total);
    const uint32_t kk = k < total ? k : (total ? total - 1 : 0u);   // k < n always; guard anyway
    if (total == 0u && t == 0) { sel[0] = 0u; sel[1] = 0u; }
    if (kk >= excl && kk < excl + local) {
        uint32_t run = excl;
        int j = 0;
#pragma unroll
        for (int jj = 0; jj < kMaxPer - 1; jj++) {
            if (jj < per - 1 && j == jj && run + mine[jj] <= kk) { run += mine[jj]; j = jj + 1; }
        }
        sel[0] = (uint32_t)(t * per + j);
        sel[1] = kk - run;
    }
    __syncthreads();
}

// index rule of _Quantile_T, sort.cu:13-19: __float2int_rn(num_of_elements * q), clipped to [0, n-1]
static uint32_t quantile_pos(int64_t n, float f) {
    float p = nearbyintf((float)n * f);
    if (!(p > 0.f)) return 0u;                      // also NaN
    if (p >= (float)(n - 1)) return (uint32_t)(n - 1);
    return (uint32_t)p;
}

// ---- the two-launch path's workspace (uint32 words; ppqhip_quantile_hot_layout reports it) ----------------------------------
constexpr uint32_t kQHStage = 2048;                 // keys a workgroup can stage per side (== its slot)
constexpr uint32_t kQHMaxWg = 512;                  // filter grid limit (records, slots)
constexpr uint32_t kQHThreadKeys = 32;              // keys of one filter workgroup and side a thread of the select holds in registers
enum { kQHEnabled = 0, kQHTHi = 1, kQHTLo = 2, kQHUses = 3,      // written by the filter's workgroup 0 (uses: hint word 7 as it found it)
       kQHZero0 = 4,                                // first word the filter zeroes
       kQHLoFlag = 4,                               // the lo side's decision, published by its owner: 0 pending, 1 settled, 2 open
       kQHRoleTicket = 10,                          // arrival ticket of the select launch: the first arrival selects (the second: the lo side of a split select)
       kQHLoClaim = 9,                              // who owns the lo side of a split select: 0 nobody yet, 1 the second arrival, 2 the first
       kQHDecision = 7,                             // the hi side's decision, published by its owner: 0 pending, 1 settled, 2 open
       kQHNext = 12,                                // [3] next chunk of each exact level
       kQHDone = 16 };                              // [3] chunks counted per exact level
constexpr uint32_t kQHOffH0 = 64;                                   // hist of key >> 20 (both sides select from it)
constexpr uint32_t kQHOffH1 = kQHOffH0 + kQ1;                       // [2][4096]: (key >> 8) & 0xFFF of the side's bucket
constexpr uint32_t kQHOffH2 = kQHOffH1 + 2 * kQ2;                   // [2][256]: key & 0xFF of the side's 24-bit prefix
constexpr uint32_t kQHZeroEnd = kQHOffH2 + 2 * kQ3;
constexpr uint32_t kQHOffRec = kQHZeroEnd;                          // [kQHMaxWg][2][8]: per side count, tie count, the first six keys (one 64-B line per workgroup)
constexpr uint32_t kQHOffHeads = kQHOffRec + kQHMaxWg * 16;         // [kQHMaxWg][2][32]: the first 32 keys of every slot, contiguous; read when a side holds more than six
constexpr uint32_t kQHOffSlots = kQHOffHeads + kQHMaxWg * 2 * 32;   // [kQHMaxWg][2][kQHStage]: the whole slot, read when it holds more than 32 keys
constexpr size_t kQHWords = (size_t)kQHOffSlots + (size_t)kQHMaxWg * 2 * kQHStage;
static_assert(kQHOffRec % 4 == 0 && kQHOffHeads % 4 == 0 && kQHOffSlots % 4 == 0, "16-B alignment of records and slots");

// the two-launch path of one hinted tensor (quantile_hot.hip): launches it and returns true when the call qualifies (16-B aligned
// x, n >= kQSpeculateMinElems, at most kQHWantedMax wanted keys per side, a hint met before); false: nothing was launched
bool quantile_hot_try(const float* x, int64_t n, float q, float* dest, uint32_t* hint, uint32_t* ws, hipStream_t s);

}  // namespace ppqhip
