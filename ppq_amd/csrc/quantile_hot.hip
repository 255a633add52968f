// quantile_hot.hip -- ONE hinted tensor in two launches (ppqhip_quantile_t; the hint's state machine: quantile.hpp).
//
// What the reference's percentile observer does per tensor per batch (observer/range.py:349 -> CUDA.Quantile -> sort.cu:42-59)
// arrives here as ONE tensor with the hint of its observer.  The general sequence (quantile.hip) spends five launches on it -- init,
// sample (returns on one load), filter, select A, F1..F3 (return on one load): 26 us of device time on [1,512,56,56], of which
// the filter's read is 5 -- because each launch decides on the DEVICE what the next one has to do (is the hint usable? did the
// lists settle both sides?), and the host cannot know without a synchronisation.  This path keeps every decision on the device
// and still launches only twice:
//   quantile_hot_filter_kernel   the filter with its arguments by value (no job table, no prefix arrays, no init launch).  The
//                                hint is read by every workgroup; a usable one filters the tensor in one pass and every workgroup
//                                leaves its keys in ITS OWN record (count, tie count, six keys inline; more keys in its slot) --
//                                no reservation atomics, nothing shared, no fences: the kernel boundary publishes the records.
//                                It also publishes the thresholds it used and zeroes the state of the launch behind it.
//   quantile_hot_select_kernel   one workgroup per CU.  The workgroup that ARRIVES first (a ticket; big lists: the first two, one side
//                                each -- never "workgroup 0": see the kernel) reads the records -- thread t holds the keys of filter
//                                workgroup t in registers, sweeps a slot of 33-256 keys itself --, counts ONE histogram round on
//                                fixed bit positions of (key - T - 1), picks the 2^11-key-wide bin of the wanted rank, collects the
//                                handful of keys of that bin and lets one wavefront finish on them (select A's rules decide
//                                settled / keep-the-hint); the other workgroups poll ONE word.
//                                Settled (the common case): that workgroup writes dest and the hint, everybody returns.  Not
//                                settled (no usable hint yet, a list that overflowed or came up short): the SAME launch runs
//                                the exact radix select over the whole tensor -- 12 + 12 + 8 key bits, three levels whose chunks
//                                are handed out through a counter, so nothing waits for a workgroup that is not resident --
//                                and leaves a hint computed from the exact histograms (quantile.hpp, "after F2 / F3"), so the
//                                next batch is settled by the filter.
// The FIRST call on a hint does not come here: it takes the general sequence, which samples its thresholds (quantile.hpp).
// What shaped the select (s_memrealtime stamps of a developer build, last at commit 2888c39): a single workgroup's chain of barrier-separated
// LDS stages costs 0.3-0.6 us per stage whatever it computes; __shfl-based scans are ds_bpermute round trips (DPP instead); 512
// LDS atomics on one address serialise (one per wavefront instead); values that are wave uniform but live in vector registers
// turn every test into an EXEC-mask branch (readfirstlane); one CU pulls ~64 B/clk, so what it reads must be compact.
// Results are exact in every case, as in the general sequence: the hint only decides how much is read.
#include <mutex>
#include <type_traits>
#include <unordered_set>
#include "quantile.hpp"

namespace ppqhip {

constexpr int kQHPollSleep = 2;                     // s_sleep argument of the workgroups that wait for the decision
constexpr int kQHPollFirst = 32;                    // .. before their first look
constexpr int kQHBlock = 512;                       // both kernels
constexpr uint32_t kQHInline = 6;                   // keys per side inside the record
constexpr uint32_t kQHListMax = 65536;              // longest list a hint may keep producing
constexpr uint32_t kQHWantedMax = 8192;             // the host routes here only when both wanted counts are at most this
constexpr uint32_t kQHThreadMore = 256;             // beyond kQHThreadKeys (quantile.hpp), up to this many keys a thread sweeps straight from the workgroup's slot (longer slots: through LDS)
constexpr uint32_t kQHRoomPerWg = 128;              // keys per filter workgroup and side the thresholds may count on (half of that: slots are uneven)
// How long a list the NEXT call's threshold is aimed at, by the side's level (quantile.hpp: "level").
__device__ __forceinline__ uint32_t qh_target(uint32_t wanted, uint32_t wgs, uint32_t level) {
    const uint32_t least = wanted + (wanted >> 1);
    const uint32_t room = umin(kQHRoomPerWg * wgs, kQHListMax);
    const uint32_t middle = (uint32_t)sqrtf((float)room * (float)wanted);
    const uint32_t most = umax(least, umin(middle, room / 2u));
    return least + (most - least) * umin(level, 3u) / 3u + 32u;
}

struct QHot {
    const float* x;
    float* dest;
    uint32_t* hint;
    uint32_t* ws;
    uint32_t n, k_hi, k_lo, wgs;     // wgs: grid of the filter (records to gather)
    uint32_t split, heads, pad0, pad1;   // split: two selecting workgroups, one per side; heads: the slots' first 32 keys are requested with the records
};

template <int K, bool PING, bool NT>
__global__ __launch_bounds__(kQHBlock) void quantile_hot_filter_kernel(const QHot a) {
    __shared__ uint32_t staged[2][kQHStage];
    __shared__ uint32_t staged_n[2], ties[2];
    const uint32_t G = gridDim.x, g = blockIdx.x, n = a.n;
    uint32_t t_hi = 0, t_lo = 0, span = 0;
    int tie_hi = 0, tie_lo = 0;                                        // wave uniform
    auto rare = [&](uint32_t key) {
        const int w = key > t_hi ? 0 : 1;
        const uint32_t at = atomicAdd(&staged_n[w], 1u);
        if (at < kQHStage) staged[w][at] = key;
    };
    const bool enabled = row_walk<kQHBlock, K, PING, GlobalLoads<NT>>(
        a.x, n,
        [&] {   // the first rows are in flight while the hint is read
            // the hint: ONE scalar load of its eight words (a short-circuit && chain compiles to five dependent round trips)
            const uint32_t* __restrict__ H = a.hint;
            const uint32_t h0 = H[kHValidHi], h1 = H[kHTHi], h2 = H[kHValidLo], h3 = H[kHTLo], h4 = H[kHN], h5 = H[kHKHi], h6 = H[kHKLo], h7 = H[kHUses];
            const bool usable = (((h0 & 0xFFu) == 1u) & ((h2 & 0xFFu) == 1u) & (h4 == n) & (h5 == a.k_hi) & (h6 == a.k_lo) & (h3 <= h1)) != 0;   // the same in every workgroup
            t_hi = h1; t_lo = h3;
            if (threadIdx.x < 2) { staged_n[threadIdx.x] = 0; ties[threadIdx.x] = 0; }
            {   // the state of the launch behind this one: flags, barrier counter, exact histograms (zeroed whether needed or not)
                constexpr uint32_t words = kQHZeroEnd - kQHZero0;
                for (uint32_t i = g * kQHBlock + threadIdx.x; i < words; i += G * kQHBlock) a.ws[kQHZero0 + i] = 0u;
                // (word 0: enabled | the sides' list-length levels, qh_target)
                if (g == 0 && threadIdx.x == 0) *reinterpret_cast<uint4*>(a.ws) = make_uint4(usable ? (1u | (h0 & 0x300u) | ((h2 & 0x300u) << 8)) : 0u, t_hi, t_lo, h7);
            }
            if (!usable) return false;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS counters are zero; the loads stay in flight
            span = t_hi - t_lo;                                            // key - t_lo > span <=> outside [t_lo, t_hi]
            return true;
        },
        [&](const float4 (&buf)[K], uint32_t cnt) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                if ((uint32_t)k < cnt) {                                   // block uniform
                    const uint32_t q0 = f2key(buf[k].x), q1 = f2key(buf[k].y), q2 = f2key(buf[k].z), q3 = f2key(buf[k].w);
                    const uint32_t d0 = q0 - t_lo, d1 = q1 - t_lo, d2 = q2 - t_lo, d3 = q3 - t_lo;
                    if ((k & 1) == 0) {        // ties on the thresholds: a lower bound is all the select needs -> one element in eight
                        tie_hi += popc_mask(__builtin_amdgcn_ballot_w64(q0 == t_hi));
                        tie_lo += popc_mask(__builtin_amdgcn_ballot_w64(q0 == t_lo));
                    }
                    if (umax(umax(d0, d1), umax(d2, d3)) > span) {
                        if (d0 > span) rare(q0);
                        if (d1 > span) rare(q1);
                        if (d2 > span) rare(q2);
                        if (d3 > span) rare(q3);
                    }
                }
            }
        },
        [&](float v, bool in, uint32_t) {
            if (in) {
                const uint32_t key = f2key(v);
                if (key - t_lo > span) rare(key);
            }
        });
    if (!enabled) return;
    if ((threadIdx.x & 63) == 0) {
        if (tie_hi) atomicAdd(&ties[0], (uint32_t)tie_hi);
        if (tie_lo) atomicAdd(&ties[1], (uint32_t)tie_lo);
    }
    __syncthreads();
    if (threadIdx.x < 16) {                                            // the record of both sides: one 64-B store
        const uint32_t side = threadIdx.x >> 3, j = threadIdx.x & 7u, c = staged_n[side];
        a.ws[kQHOffRec + g * 16u + threadIdx.x] = j == 0 ? c : (j == 1 ? ties[side] : ((j - 2u) < umin(c, kQHInline) ? staged[side][j - 2u] : 0u));
    }
    if (threadIdx.x < 64) {                                            // the heads of both slots: one 256-B store (read when a side holds more than the record does)
        const uint32_t side = threadIdx.x >> 5, i = threadIdx.x & 31u, c = staged_n[side];
        if ((c > kQHInline || a.heads) && i < c) a.ws[kQHOffHeads + g * 64u + threadIdx.x] = staged[side][i];
    }
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const uint32_t c = umin(staged_n[side], kQHStage);
        if (c > 32u) {
            uint32_t* slot = a.ws + kQHOffSlots + ((size_t)g * 2 + side) * kQHStage;
            for (uint32_t i = threadIdx.x; i < c; i += kQHBlock) slot[i] = staged[side][i];
        }
    }
}

constexpr uint32_t kQHBins = 2048;                  // the select's one histogram round: 11-bit digits ..
constexpr int kQHDigitShift = 11;                   // .. of (key - T - 1) >> 11, saturating: bins of 2^-12 relative width over the half binade above T
                                                    // (the answer is the wanted-th largest of ~1.5 x wanted keys: it lies in the dense third next to T)
constexpr uint32_t kQHSurvCap = 2048;               // keys of the chosen bin ("survivors") a wavefront finishes on
constexpr uint32_t kQHBigCap = 8192;                // LDS room per side for the keys of slots longer than that
constexpr uint32_t kQHWaveKeys = kQHSurvCap;
struct QHSelLds {
    uint32_t hist[2][kQHBins + 64];                 // + one trash counter per lane: the adds of a pass are unconditional
    uint32_t surv[2][kQHSurvCap];
    uint32_t big[2][kQHBigCap];
    uint32_t bigdesc[2][kQHMaxWg][2];               // slots copied into `big`: (workgroup << 16 | count), offset
    uint32_t wavehist[2][320];                      // wave_select: 256 counters + 64 trash counters per wave
    uint32_t total[2], tie[2], nsurv[2], nbig[2], nbigdesc[2], flags;
    uint32_t bin[2], rin[2], result[2];
    uint32_t bin_up[2], bin_q[2];                    // re-centring the thresholds: the bin of rank total - target, of rank total / 4
    uint32_t sc[2][8];
};
struct QHExactLds {
    uint32_t h[2 * (kQ1 + kQTrash)];
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The rank-th smallest (0-based) of keys[0..count) in LDS, 1 <= count <= kQHWaveKeys, by ONE wavefront and without a barrier.
// Up to 64 keys: one key per lane, its rank counted against the other lanes' keys (v_readlane).  More: <= 32 keys per lane in
// registers, radix select on (key - min) with 8-bit digits over a 256-counter LDS histogram private to the wave (`hist`: 320
// words, 16-B aligned).  count / rank must be wave uniform (they are made scalar here: values picked by wave index arrive in
// vector registers, and every test on them would become an EXEC-mask branch with its own LDS wait).
__device__ __forceinline__ uint32_t wave_select(const uint32_t* keys, uint32_t count, uint32_t rank, uint32_t* hist) {
    count = rfl(count); rank = rfl(rank);
    const uint32_t lane = threadIdx.x & 63u;
    if (count <= 64u) {
        const uint32_t mine = keys[umin(lane, count - 1u)];
        uint32_t below = 0u;
        for (uint32_t i = 0; i < count; i++) {                          // scalar trip count
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)i);
            below += (o < mine || (o == mine && i < lane)) ? 1u : 0u;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(lane < count && below == rank);      // exactly one lane
        return (uint32_t)__builtin_amdgcn_readlane((int)mine, m ? __builtin_ctzll(m) : 0);
    }
    constexpr int S = (int)(kQHWaveKeys / 64u);
    const int slots = (int)((count + 63u) >> 6);        // wave uniform: registers in use
    uint32_t d[S];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
    for (int j = 0; j < S; j++) d[j] = keys[umin((uint32_t)j * 64u + lane, count - 1u)];       // unconditional: one pipelined burst
#pragma unroll
    for (int j = 0; j < S; j++) { mn = umin(mn, d[j]); mx = umax(mx, d[j]); }                   // (clamped slots repeat the last key)
    mn = wave_all_min(mn); mx = wave_all_max(mx);
    if (mn == mx) return mn;
    int pos = 32 - __builtin_clz(mx - mn);
    uint32_t prefix = 0u;
    uint4* hist4 = reinterpret_cast<uint4*>(hist);
    const uint32_t trash = 256u + lane;                 // per-lane counter for "not this round": the adds stay unconditional
    while (pos > 0) {                                   // wave uniform
        const int w = pos > 8 ? 8 : pos, shift = pos - w;
        hist4[lane] = make_uint4(0u, 0u, 0u, 0u);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < S; j++) {
            if (j < slots) {
                const uint32_t dj = d[j] - mn;
                const bool in = (uint32_t)j * 64u + lane < count;
                const uint32_t head = pos >= 32 ? 0u : dj >> pos;
                const bool match = in && head == prefix;
                atomicAdd(&hist[match ? ((dj >> shift) & ((1u << w) - 1u)) : trash], 1u);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint4 c = hist4[lane];
        const uint32_t sum = c.x + c.y + c.z + c.w;
        const uint32_t inc = wave_scan_add(sum);
        const uint32_t excl = inc - sum;
        const bool hit = rank >= excl && rank < inc;    // exactly one lane (rank < the number of matching keys)
        uint32_t digit = lane * 4u, rin = rank - excl;
        if (rin >= c.x) { rin -= c.x; digit++; if (rin >= c.y) { rin -= c.y; digit++; if (rin >= c.z) { rin -= c.z; digit++; } } }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        const int src = m ? __builtin_ctzll(m) : 0;
        digit = (uint32_t)__builtin_amdgcn_readlane((int)digit, src);
        rank = (uint32_t)__builtin_amdgcn_readlane((int)rin, src);
        prefix = (prefix << w) | digit;
        pos = shift;
    }
    return mn + prefix;
}

// Both sides of the filter's records -> settled?  (select A's rules.)  All 512 threads of ONE workgroup call; the results are
// block uniform.  Thread t holds the keys of workgroup t's slots in registers (both sides: the record and the first 32 keys of each
// slot are requested together, ONE round trip; longer slots go through LDS).  The lo side runs on ~key, so that both sides read
// "the rank-th smallest of the keys ABOVE a threshold".  One histogram round on fixed bit positions of (key - T - 1) finds the
// 2^13-key-wide bin of the answer; the keys of that bin are few and one wavefront per side finishes on them.
// What thread t of a selecting workgroup holds of filter workgroup t: its 64-B record.  Requested BEFORE the workgroup knows whether it
// selects at all (see the kernel): one round trip for the arrival ticket, the header and these.  (The heads of big tensors --
// 164 KB -- are fetched by the selecting workgroups only: requested up front they held the ticket back by 3 us.)
struct QHRecs {
    uint4 r4[4];
    uint4 head[kQHThreadKeys / 4];      // split select of a big tensor: the heads of side `head_side` (2: none held)
    uint32_t head_side;
};
// `guess`: the side this workgroup will probably select (split select: the first arrival takes hi, the second lo -- in practice
// workgroups 0 and 1); 2: no guess.  A wrong guess costs the reload inside hot_select_records, nothing else.
__device__ __forceinline__ void hot_load_records(const QHot& a, QHRecs& R, uint32_t guess) {
    R.r4[0] = R.r4[1] = R.r4[2] = R.r4[3] = make_uint4(0u, 0u, 0u, 0u);
    R.head_side = 2u;
    if (threadIdx.x < a.wgs) {
        const uint4* rec = reinterpret_cast<const uint4*>(a.ws + kQHOffRec) + (size_t)threadIdx.x * 4;
        R.r4[0] = rec[0]; R.r4[1] = rec[1]; R.r4[2] = rec[2]; R.r4[3] = rec[3];
    }
    if (a.heads && guess < 2u) {
        R.head_side = guess;
        if (threadIdx.x < a.wgs) {
            const uint4* head = reinterpret_cast<const uint4*>(a.ws + kQHOffHeads) + ((size_t)threadIdx.x * 2 + guess) * (kQHThreadKeys / 4);
#pragma unroll
            for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) R.head[i] = head[i];
        }
    }
}

// keep[w]: the side's valid word for the hint -- 0: drop it, else 1 | level << 8 (qh_target); level[w] / uses: as the filter found them
__device__ __forceinline__ void hot_select_records(const QHot& a, QHRecs& R, const uint32_t (&T)[2], const uint32_t sides, QHSelLds& L, uint32_t (&key_out)[2],
                                                   bool (&done)[2], uint32_t (&keep)[2], uint32_t (&T_next)[2], const uint32_t (&level)[2], const uint32_t uses) {
    const uint32_t n = a.n, t = threadIdx.x, lane = t & 63u;
    uint4 (&r4)[4] = R.r4;
    uint4 k4[2][kQHThreadKeys / 4];
    if (a.heads && t < a.wgs) {                                        // big tensors: the filter wrote every head; this workgroup's sides only
#pragma unroll
        for (int w = 0; w < 2; w++) {
            if (!(sides & (1u << w))) continue;
            if (R.head_side == (uint32_t)w) {                          // (block uniform) requested with the ticket
#pragma unroll
                for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) k4[w][i] = R.head[i];
                continue;
            }
            const uint4* head = reinterpret_cast<const uint4*>(a.ws + kQHOffHeads) + ((size_t)t * 2 + w) * (kQHThreadKeys / 4);
#pragma unroll
            for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) k4[w][i] = head[i];
        }
    }
    if (t < 2) { L.total[t] = 0u; L.tie[t] = 0u; L.nsurv[t] = 0u; L.nbig[t] = 0u; L.nbigdesc[t] = 0u; L.flags = 0u; }
    {
        uint4* z = reinterpret_cast<uint4*>(&L.hist[0][0]);           // (2 x 2112 words = 1056 uint4)
        z[t] = make_uint4(0u, 0u, 0u, 0u); z[kQHBlock + t] = make_uint4(0u, 0u, 0u, 0u);
        if (t < 2u * (kQHBins + 64u) / 4u - 2u * kQHBlock) z[2 * kQHBlock + t] = make_uint4(0u, 0u, 0u, 0u);
    }
    uint32_t cnt[2] = {r4[0].x, r4[2].x}, tie[2] = {r4[0].y, r4[2].y};
    uint32_t c[2] = {umin(cnt[0], kQHStage), umin(cnt[1], kQHStage)};
#pragma unroll
    for (int w = 0; w < 2; w++) {
        if (!(sides & (1u << w))) { c[w] = 0u; tie[w] = 0u; cnt[w] = 0u; continue; }                   // (block uniform: the other workgroup's side)
        // six keys came with the record; a longer slot's first 32 were requested with it (big tensors: `heads`) or are fetched
        // now (a second round trip, only for the threads that need it)
        if (!a.heads) {
            k4[w][0] = make_uint4(r4[2 * w].z, r4[2 * w].w, r4[2 * w + 1].x, r4[2 * w + 1].y);
            k4[w][1] = make_uint4(r4[2 * w + 1].z, r4[2 * w + 1].w, 0u, 0u);
            if (c[w] > kQHInline && c[w] <= kQHThreadKeys) {
                const uint4* head = reinterpret_cast<const uint4*>(a.ws + kQHOffHeads) + ((size_t)t * 2 + w) * (kQHThreadKeys / 4);
#pragma unroll
                for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) k4[w][i] = head[umin(i, (c[w] - 1u) >> 2)];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 2; w++) {
        // (one LDS atomic per wavefront: 512 adds on one address serialise at ~5 cycles each -- 4 us measured)
        const uint32_t wc = wave_scan_add(c[w]), wt = wave_scan_add(tie[w]);
        if (lane == 63u) { if (wc) atomicAdd(&L.total[w], wc); if (wt) atomicAdd(&L.tie[w], wt); }
        if (cnt[w] > kQHStage) atomicOr(&L.flags, 1u << w);                              // the workgroup could not stage all its keys
        if (c[w] > kQHThreadMore) {
            const uint32_t base = atomicAdd(&L.nbig[w], c[w]);
            if (base + c[w] <= kQHBigCap) {
                const uint32_t at = atomicAdd(&L.nbigdesc[w], 1u);
                L.bigdesc[w][at][0] = (t << 16) | c[w]; L.bigdesc[w][at][1] = base;
            } else atomicOr(&L.flags, 1u << w);
        }
    }
    const uint32_t Tp[2] = {T[0], ~T[1]};
    // every key this thread holds of side w: f(key', valid), key' = the key (hi) / ~key (lo); straight-line code up to the
    // wave's longest slot (a scalar trip count)
    auto for_my_keys = [&](int w, auto f) {
        const uint32_t cw = c[w] <= kQHThreadKeys ? c[w] : 0u;
        const uint32_t cmax = wave_all_max(cw);
        const uint32_t flip = w ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) {
            if (4u * i < cmax) {
                f(k4[w][i].x ^ flip, 4u * i + 0u < cw); f(k4[w][i].y ^ flip, 4u * i + 1u < cw);
                f(k4[w][i].z ^ flip, 4u * i + 2u < cw); f(k4[w][i].w ^ flip, 4u * i + 3u < cw);
            }
        }
    };
    // a slot of 33 .. kQHThreadMore keys: its thread sweeps it straight from the workspace, sixteen keys per trip (every lane its own
    // lines, L2-resident: a restless stream's lists -- qh_target -- are a few dozen keys per filter workgroup, not six)
    auto for_slot_keys = [&](int w, auto f) __attribute__((always_inline)) {
        const uint32_t cw = (c[w] > kQHThreadKeys && c[w] <= kQHThreadMore) ? c[w] : 0u;
        const uint32_t cmax = wave_all_max(cw);
        if (cmax == 0u) return;
        const uint32_t flip = w ? 0xFFFFFFFFu : 0u;
        const uint4* slot = reinterpret_cast<const uint4*>(a.ws + kQHOffSlots + ((size_t)t * 2 + w) * kQHStage);
#pragma nounroll
        for (uint32_t i = 0; 4u * i < cmax; i += 4u) {                    // (scalar trip count; the slot is kQHStage keys long: no clamp needed)
            const uint4 q0 = slot[i], q1 = slot[i + 1u], q2 = slot[i + 2u], q3 = slot[i + 3u];
            const uint32_t at = 4u * i;
            f(q0.x ^ flip, at + 0u < cw); f(q0.y ^ flip, at + 1u < cw); f(q0.z ^ flip, at + 2u < cw); f(q0.w ^ flip, at + 3u < cw);
            f(q1.x ^ flip, at + 4u < cw); f(q1.y ^ flip, at + 5u < cw); f(q1.z ^ flip, at + 6u < cw); f(q1.w ^ flip, at + 7u < cw);
            f(q2.x ^ flip, at + 8u < cw); f(q2.y ^ flip, at + 9u < cw); f(q2.z ^ flip, at + 10u < cw); f(q2.w ^ flip, at + 11u < cw);
            f(q3.x ^ flip, at + 12u < cw); f(q3.y ^ flip, at + 13u < cw); f(q3.z ^ flip, at + 14u < cw); f(q3.w ^ flip, at + 15u < cw);
        }
    };
    auto digit_of = [&](int w, uint32_t kp) { return umin((kp - Tp[w] - 1u) >> kQHDigitShift, kQHBins - 1u); };
    const uint32_t trash = kQHBins + lane;
    // the histogram round does not wait for the totals (whether a side selects at all is decided behind the next barrier)
#pragma unroll
    for (int w = 0; w < 2; w++)
        if (sides & (1u << w)) {
            for_my_keys(w, [&](uint32_t kp, bool valid) { atomicAdd(&L.hist[w][valid ? digit_of(w, kp) : trash], 1u); });
            for_slot_keys(w, [&](uint32_t kp, bool valid) { atomicAdd(&L.hist[w][valid ? digit_of(w, kp) : trash], 1u); });
        }
    __syncthreads();
    uint32_t nbigkeys[2] = {0u, 0u};
    if (L.nbigdesc[0] | L.nbigdesc[1]) {                               // block uniform: long slots, wavefront v copies the v-th, (v + 8)-th ..
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const uint32_t nb = L.nbigdesc[w];
            for (uint32_t b = t >> 6; b < nb; b += kQHBlock / kWave) {
                const uint32_t g = L.bigdesc[w][b][0] >> 16, cg = L.bigdesc[w][b][0] & 0xFFFFu;
                const uint32_t* slot = a.ws + kQHOffSlots + ((size_t)g * 2 + w) * kQHStage;
                uint32_t* dst = L.big[w] + L.bigdesc[w][b][1];
                for (uint32_t i = lane; i < cg; i += 4u * kWave) {
                    uint32_t k[4];
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) k[u] = slot[umin(i + u * kWave, cg - 1u)];
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) if (i + u * kWave < cg) dst[i + u * kWave] = k[u];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; w++) {
            nbigkeys[w] = umin(L.nbig[w], kQHBigCap);
            for (uint32_t i = t; i < nbigkeys[w]; i += kQHBlock) atomicAdd(&L.hist[w][digit_of(w, L.big[w][i] ^ (w ? 0xFFFFFFFFu : 0u))], 1u);
        }
        __syncthreads();
    }
    const uint32_t flags = L.flags;
    uint32_t total[2], rank[2], wanted[2];
    int how[2];                                                        // 0: open, 1: the threshold itself, 2: select
#pragma unroll
    for (int w = 0; w < 2; w++) {
        const uint32_t k = w ? a.k_lo : a.k_hi;
        total[w] = L.total[w];
        wanted[w] = w ? k + 1u : n - k;
        // hi: the (k - (n - total))-th smallest listed key; lo: the k-th smallest = the (total - 1 - k)-th smallest of the ~keys
        rank[w] = w ? total[w] - 1u - k : k - (n - total[w]);
        done[w] = false; keep[w] = 0u; key_out[w] = T[w]; how[w] = 0;
        if ((flags & (1u << w)) || !(sides & (1u << w))) continue;
        if (total[w] >= wanted[w]) {
            // settled by the list.  The hint is KEPT and its threshold re-centred on this batch (below): select A's rule -- drop a hint
            // whose list came out nearly too short or needlessly long -- costs three exact passes on the next batch here.  The level
            // goes up when the list came within a quarter of failing, down on every 64th settled call.
            how[w] = 2; done[w] = true;
            uint32_t lv = level[w];
            if (total[w] - wanted[w] < (wanted[w] >> 2)) lv = umin(lv + 1u, 3u);
            else if ((uses & 63u) == 63u && lv > 0u) lv -= 1u;
            keep[w] = 1u | (lv << 8);
        } else if (wanted[w] - total[w] <= L.tie[w]) { how[w] = 1; done[w] = true; keep[w] = 1u | (level[w] << 8); }     // the tie value itself
    }
    uint32_t target[2];
#pragma unroll
    for (int w = 0; w < 2; w++) target[w] = qh_target(wanted[w], a.wgs, keep[w] >> 8);                  // keys the NEXT list should hold
    if (t < 2) { L.bin_up[t] = 0u; L.bin_q[t] = 0u; }
    {   // the bin of the rank: half h of the workgroup scans side h (thread lt owns bins [8 lt, 8 lt + 8))
        const uint32_t half = rfl(t >> 8), lt = t & 255u, wl = rfl(lt >> 6);
        const uint4* h4 = reinterpret_cast<const uint4*>(&L.hist[half][0]);       // ((kQHBins + 64) * 4 B: 16-B aligned rows)
        const uint4 c0 = h4[2u * lt], c1 = h4[2u * lt + 1u];
        const uint32_t b[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const uint32_t sum = b[0] + b[1] + b[2] + b[3] + b[4] + b[5] + b[6] + b[7];
        const uint32_t inc = wave_scan_add(sum);
        if (lane == 63u) L.sc[half][wl] = inc;
        __syncthreads();
        uint32_t woff = 0u;
#pragma unroll
        for (uint32_t ww = 0; ww < 4; ww++) woff += ww < wl ? L.sc[half][ww] : 0u;
        const uint32_t excl = woff + inc - sum, r = half ? rank[1] : rank[0];
        if ((half ? how[1] : how[0]) == 2 && r >= excl && r < excl + sum) {             // one thread of the half
            uint32_t rin = r - excl, digit = lt * 8u;
#pragma unroll
            for (int j = 0; j < 7; j++) if (digit == lt * 8u + (uint32_t)j && rin >= b[j]) { rin -= b[j]; digit++; }
            L.bin[half] = digit; L.rin[half] = rin;
        }
        // the same prefix sums place two more ranks: total - target (everything from that bin up is what the next list should be)
        // and total / 4 (how densely the keys lie just above the threshold, should the list have to grow)
        const uint32_t tot = half ? total[1] : total[0], tgt = half ? target[1] : target[0];
        if ((half ? how[1] : how[0]) == 2 && sum != 0u) {
            auto place = [&](uint32_t rr) {
                uint32_t rin = rr - excl, digit = lt * 8u;
#pragma unroll
                for (int j = 0; j < 7; j++) if (digit == lt * 8u + (uint32_t)j && rin >= b[j]) { rin -= b[j]; digit++; }
                return digit;
            };
            if (tot > tgt && tot - tgt >= excl && tot - tgt < excl + sum) L.bin_up[half] = place(tot - tgt);
            if (tot < tgt && tot / 4u >= excl && tot / 4u < excl + sum) L.bin_q[half] = place(tot / 4u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 2; w++) {                                       // next call's thresholds (on the key' axis, then back)
        T_next[w] = T[w];
        if (how[w] != 2) continue;
        uint32_t Tpn = Tp[w];
        if (total[w] > target[w]) Tpn = Tp[w] + (L.bin_up[w] << kQHDigitShift);         // exact: the hist says how many keys lie above
        else if (total[w] < target[w]) {                                   // extrapolated from the density of the lowest quarter of the list
            const float span = (float)((L.bin_q[w] + 1u) << kQHDigitShift);                 // (< 2^22: exact; the rest is an estimate anyway)
            const float want_more = (float)(target[w] - total[w]) * span * 4.f / (float)umax(total[w], 1u);
            const uint32_t delta = (uint32_t)fminf(want_more, 8.f * span);
            Tpn = Tp[w] > delta ? Tp[w] - delta : 0u;
        }
        T_next[w] = w ? ~Tpn : Tpn;
    }
#pragma unroll
    for (int w = 0; w < 2; w++) {
        if (how[w] != 2) continue;
        const uint32_t bin = L.bin[w];
        // key' lies in the bin <=> key' - (T' + 1 + (bin << shift)) < 2^shift (the saturating last bin: no upper end)
        const uint32_t lo = Tp[w] + 1u + (bin << kQHDigitShift), width = bin == kQHBins - 1u ? 0xFFFFFFFFu - lo : (1u << kQHDigitShift) - 1u;
        auto take = [&](uint32_t kp) { const uint32_t at = atomicAdd(&L.nsurv[w], 1u); if (at < kQHSurvCap) L.surv[w][at] = kp; };
        {
            const uint32_t cw = c[w] <= kQHThreadKeys ? c[w] : 0u;
            const uint32_t cmax = wave_all_max(cw);
            const uint32_t flip = w ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (uint32_t i = 0; i < kQHThreadKeys / 4; i++) {
                if (4u * i < cmax) {
                    const uint32_t k0 = k4[w][i].x ^ flip, k1 = k4[w][i].y ^ flip, k2 = k4[w][i].z ^ flip, k3 = k4[w][i].w ^ flip;
                    const bool m0 = k0 - lo <= width && 4u * i + 0u < cw, m1 = k1 - lo <= width && 4u * i + 1u < cw;
                    const bool m2 = k2 - lo <= width && 4u * i + 2u < cw, m3 = k3 - lo <= width && 4u * i + 3u < cw;
                    if (m0 | m1 | m2 | m3) {                               // rare: one divergent region per four keys
                        if (m0) take(k0);
                        if (m1) take(k1);
                        if (m2) take(k2);
                        if (m3) take(k3);
                    }
                }
            }
        }
        for_slot_keys(w, [&](uint32_t kp, bool valid) { if (valid && kp - lo <= width) take(kp); });
        for (uint32_t i = t; i < nbigkeys[w]; i += kQHBlock) { const uint32_t kp = L.big[w][i] ^ (w ? 0xFFFFFFFFu : 0u); if (kp - lo <= width) take(kp); }
    }
    __syncthreads();
    {   // wavefront 0 finishes the hi side, wavefront 4 (another SIMD) the lo side
        const uint32_t wid = rfl(t >> 6), side = wid >> 2;
        const uint32_t ns = side ? L.nsurv[1] : L.nsurv[0];
        if ((wid & 3u) == 0u && (side ? how[1] : how[0]) == 2 && ns >= 1u && ns <= kQHSurvCap) {
            const uint32_t kp = wave_select(L.surv[side], ns, side ? L.rin[1] : L.rin[0], L.wavehist[side]);
            if (lane == 0u) L.result[side] = side ? ~kp : kp;
        }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 2; w++) {
        if (how[w] != 2) continue;
        const uint32_t ns = L.nsurv[w];
        if (ns >= 1u && ns <= kQHSurvCap) key_out[w] = L.result[w];
        else { done[w] = false; keep[w] = 0u; }                        // a bin too crowded for one wavefront (ties, saturation): exact passes
    }
}

// One CHUNK of the tensor: `rows` rows of kQHBlock float4 starting at row c * rows (a multiple of four rows; the last chunk also
// owns the n % 4 elements behind the last float4): on_tile(sample, valid) once per four rows, on_elem(value, valid) for every
// slot -- trip counts are block uniform.  Two register tiles of four rows ping-pong.
template <typename FT, typename FE>
__device__ __forceinline__ void hot_walk_chunk(const float* __restrict__ x, uint32_t n, uint32_t c, uint32_t chunks, uint32_t rows, FT on_tile, FE on_elem) {
    const uint32_t nvec = n >> 2;
    const float4* xv = reinterpret_cast<const float4*>(x);
    const uint32_t v_begin = c * rows * kQHBlock + threadIdx.x, groups = rows / 4u;
    float4 ba[4], bb[4];
    auto fetch = [&](float4 (&b)[4], uint32_t grp) {
        const uint32_t v0 = v_begin + umin(grp, groups - 1u) * 4u * kQHBlock;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) b[u] = gload4<false>(xv + umin(v0 + u * kQHBlock, nvec - 1u));        // nvec >= 1: n >= 2^18
    };
    auto consume = [&](const float4 (&b)[4], uint32_t grp) {
        const uint32_t v0 = v_begin + grp * 4u * kQHBlock;
        on_tile(b[0].x, v0 < nvec);
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const bool in = v0 + u * kQHBlock < nvec;
            on_elem(b[u].x, in); on_elem(b[u].y, in); on_elem(b[u].z, in); on_elem(b[u].w, in);
        }
    };
    fetch(ba, 0);
    for (uint32_t grp = 0;;) {
        fetch(bb, grp + 1);
        consume(ba, grp);
        if (++grp >= groups) break;
        fetch(ba, grp + 1);
        consume(bb, grp);
        if (++grp >= groups) break;
    }
    if (c == chunks - 1u) {                                            // block uniform
        const uint32_t i = (nvec << 2) + threadIdx.x;
        const bool in = i < n;
        const float v = in ? gload1(x + i) : 0.f;
        on_tile(v, in);
        on_elem(v, in);
    }
}

// The exact passes do not depend on which workgroups are resident: they hand out their chunks through a counter, so a level is
// complete when its chunks are -- whoever counted them.  (A grid barrier that waits for WORKGROUPS would hang as soon as two of
// these launches, from two streams, share the chip.)
__global__ __launch_bounds__(kQHBlock) void quantile_hot_select_kernel(const QHot a) {
    __shared__ union { QHSelLds s; QHExactLds e; } L;
    __shared__ uint32_t scratch[32], sel[2], bcast[4];
    const uint32_t n = a.n;
    uint32_t* ws = a.ws;
    // The selecting role goes to the workgroup that ARRIVES first (a ticket), the second side of a split select to the second.
    // Rounds of measurements with "workgroup 0 selects, the others wait" ended in launches of 7 .. 55 s: with three queues busy
    // (two of these launches on two streams beside a copy on a third) workgroup 0 of a grid is NOT always resident when its
    // siblings are, and two launches whose pollers hold each other's CUs only move again when the queue scheduler time-slices
    // them (tools/quantile_soak.py single, profiles/r06_quantile_soak.txt).  Nothing here depends on dispatch order now.
    const uint4 hdr = *reinterpret_cast<const uint4*>(ws);
    if (threadIdx.x == 0) bcast[0] = __hip_atomic_fetch_add(&ws[kQHRoleTicket], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    QHRecs R;
    __syncthreads();
    const uint32_t arrival = bcast[0];
    __syncthreads();
    const uint32_t role = arrival == 0u ? 0u : ((a.split && arrival == 1u) ? 1u : 0xFFFFFFFFu);
    // the records are requested once the role is known, the owner's own side's heads with them.  (Until the round's last day the 16
    // lowest workgroups requested them together with the ticket, "in practice the first to arrive": the stamps say the first arrivals
    // are workgroups 5, 47, 101, 135, 149, 237 .. -- hardly ever one of those; 0 / 8 / 16 / 32 / 64 speculators measured alike.)
    if (role < 2u) hot_load_records(a, R, role);
    else { R.r4[0] = R.r4[1] = R.r4[2] = R.r4[3] = make_uint4(0u, 0u, 0u, 0u); R.head_side = 2u; }
    const bool enabled = hdr.x != 0u;
    const uint32_t T[2] = {hdr.y, hdr.z};
    uint32_t key_sel[2] = {T[0], T[1]};
    bool done_sel[2] = {false, false};
    uint32_t keep_sel[2] = {0u, 0u};                                 // the sides' valid words for the hint (0: drop; 1 | level << 8)
    const uint32_t level[2] = {(hdr.x >> 8) & 3u, (hdr.x >> 16) & 3u};
    uint32_t T_next[2] = {T[0], T[1]};
    // ---- the decisions: every side has an OWNER that selects it, writes its results and publishes one word; everybody else polls ----
    // One selecting workgroup owns both sides; of two, the first arrival owns the hi side and the second the lo side -- if it is
    // there: it claims the side FIRST (a compare-and-swap), and the first arrival, done with its own side, claims the lo side for the
    // exact passes should nobody have (a workgroup that is not resident must never be waited for).  Nothing is handed from one
    // owner to the other: each writes its side of `dest` and of the hint itself (the hi side's owner also the words they share), and an
    // owner whose sides are settled returns at once.  (Until round 6's last day the lo side's result travelled to the first arrival
    // through a flag: 3.4 us of waiting on B x 32, profiles/r06_quantile_select_stamps.txt.)
    uint32_t open_mask;
    uint32_t own = role == 0u ? (a.split ? 1u : 3u) : 0u;            // sides this workgroup owns (block uniform)
    if (role == 1u) {
        if (threadIdx.x == 0) {
            uint32_t expected = 0u;
            bcast[0] = __hip_atomic_compare_exchange_strong(&ws[kQHLoClaim], &expected, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
        }
        __syncthreads();
        own = bcast[0] ? 2u : 0u;
        __syncthreads();
    }
    // ONE call site for both roles (the function is a few thousand instructions, inlined: a second copy costs registers and scratch)
    if (own != 0u && enabled) hot_select_records(a, R, T, own, L.s, key_sel, done_sel, keep_sel, T_next, level, hdr.w);
    if (role == 0u) {
        if (a.split) {                               // is the lo side taken?  If the second arrival has not even started, it stays OPEN and is
            if (threadIdx.x == 0) {                  // this workgroup's: the exact passes settle it (never seen outside a chip shared with other queues)
                uint32_t expected = 0u;
                bcast[0] = __hip_atomic_compare_exchange_strong(&ws[kQHLoClaim], &expected, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
            }
            __syncthreads();
            if (bcast[0]) own |= 2u;
            __syncthreads();
        }
    }
    if (own != 0u && threadIdx.x == 0) {
        // the decisions FIRST (a few hundred workgroups are waiting for them; the stores behind them queue in order), then the settled
        // sides' results and hint words -- nobody reads those before the launch ends; open sides: after the exact passes (below)
        if (own & 1u) __hip_atomic_store(&ws[kQHDecision], done_sel[0] ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (own & 2u) __hip_atomic_store(&ws[kQHLoFlag], done_sel[1] ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t* H = a.hint;
        if ((own & 1u) && done_sel[0]) { a.dest[0] = key2f(key_sel[0]); H[kHValidHi] = keep_sel[0]; H[kHTHi] = keep_sel[0] ? T_next[0] : T[0]; }
        if ((own & 2u) && done_sel[1]) { a.dest[1] = key2f(key_sel[1]); H[kHValidLo] = keep_sel[1]; H[kHTLo] = keep_sel[1] ? T_next[1] : T[1]; }
        if (role == 0u) {
            H[kHN] = n; H[kHKHi] = a.k_hi; H[kHKLo] = a.k_lo;
            if (enabled && done_sel[0]) H[kHUses] = hdr.w + 1u;
        }
    }
    {
        const uint32_t mine_open = ((own & 1u) && !done_sel[0] ? 1u : 0u) | ((own & 2u) && !done_sel[1] ? 2u : 0u);
        if (own != 0u && mine_open == 0u) return;   // an owner with nothing open is done: the exact passes (if the other side needs
                                                                     // them) hand their chunks out through a counter, whoever is there takes them
        if (threadIdx.x == 0) {                      // everybody else needs BOTH decisions: one open mask for all who count
            uint32_t dh, dl;
            if (own == 0u) __builtin_amdgcn_s_sleep(kQHPollFirst);           // the decisions are microseconds away
            while ((dh = __hip_atomic_load(&ws[kQHDecision], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) __builtin_amdgcn_s_sleep(kQHPollSleep);
            while ((dl = __hip_atomic_load(&ws[kQHLoFlag], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) __builtin_amdgcn_s_sleep(kQHPollSleep);
            bcast[3] = (dh == 2u ? 1u : 0u) | (dl == 2u ? 2u : 0u);
        }
        __syncthreads();
        open_mask = bcast[3];
        if (open_mask == 0u) return;
    }
    // ---- not settled: exact radix select over the whole tensor (12 + 12 + 8 key bits) ----
    // prefix / rank per side after each level; every workgroup arrives at the same numbers from the same global histograms
    uint32_t top[2] = {0u, 0u}, r0k[2] = {0u, 0u}, p24[2] = {0u, 0u}, r24[2] = {0u, 0u}, low[2] = {0u, 0u};
    if (open_mask != 0u) {
        __syncthreads();
        uint32_t* he = L.e.h;
        const uint32_t kk[2] = {a.k_hi, a.k_lo};
        // chunks of 8 .. 256 rows (64 KB .. 2 MB), about four per workgroup, handed out by a counter (a returning device atomic is
        // a 1.8 us round trip: one per 64 KB, not overlapped, held the passes at 3.5 TB/s)
        const uint32_t G = gridDim.x, total_rows = ((n >> 2) + kQHBlock - 1u) / kQHBlock;
        uint32_t chunk_rows = (total_rows + 4u * G - 1u) / (4u * G);
        chunk_rows = umin(256u, umax(8u, (chunk_rows + 3u) & ~3u));
        const uint32_t chunks = (total_rows + chunk_rows - 1u) / chunk_rows;
        for (int level = 0; level < 3; level++) {
            for (uint32_t i = threadIdx.x; i < 2u * (kQ1 + kQTrash); i += kQHBlock) he[i] = 0u;
            __syncthreads();
            uint32_t mine = 0;
            const int shift = level == 1 ? 8 : 0, pshift = level == 1 ? 20 : 8;
            const uint32_t dmask = level == 1 ? 0xFFFu : 0xFFu;
            const int nb = level == 2 ? kQ3 : kQ1;
            // a settled side matches nothing: no prefix has bit 31 set after the shift
            const uint32_t p_hi = (open_mask & 1u) ? (level == 1 ? top[0] : p24[0]) : 0xFFFFFFFFu;
            const uint32_t p_lo = (open_mask & 2u) ? (level == 1 ? top[1] : p24[1]) : 0xFFFFFFFFu;
            WaveBinCounter<false, true, true> acc;
            acc.init(reinterpret_cast<int*>(he), kQ1);
            HotCounter hi_c, lo_c;
            hi_c.init(he, nb);
            lo_c.init(he + kQ1 + kQTrash, nb);
            // every chunk comes from the counter (a chunk owned by a workgroup that is not resident would stall the level); the NEXT
            // ticket is requested before the current chunk is walked, so only the first round trip of a level is exposed
            uint32_t ticket = 0;
            if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(&ws[kQHNext + level], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                if (threadIdx.x == 0) bcast[0] = ticket;
                __syncthreads();
                const uint32_t c = bcast[0];
                __syncthreads();
                if (c >= chunks) break;
                if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(&ws[kQHNext + level], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mine++;
                if (level == 0) {
                    hot_walk_chunk(a.x, n, c, chunks, chunk_rows,
                                   [&](float v, bool in) { acc.elect((int)(f2key(v) >> 20), in); },
                                   [&](float v, bool in) { acc.template commit<false>((int)(f2key(v) >> 20), in); });
                } else {
                    hot_walk_chunk(a.x, n, c, chunks, chunk_rows,
                                   [&](float v, bool in) {
                                       const uint32_t key = f2key(v);
                                       hi_c.elect((int)((key >> shift) & dmask), in && (key >> pshift) == p_hi);
                                       lo_c.elect((int)((key >> shift) & dmask), in && (key >> pshift) == p_lo);
                                   },
                                   [&](float v, bool in) {
                                       const uint32_t key = f2key(v);
                                       const int d = (int)((key >> shift) & dmask);
                                       if (in && (key >> pshift) == p_hi) hi_c.add(d);
                                       if (in && (key >> pshift) == p_lo) lo_c.add(d);
                                   });
                }
            }
            if (level == 0) acc.flush_hot(); else { hi_c.flush(); lo_c.flush(); }
            __syncthreads();
            if (mine) {                             // this workgroup's counts -> the global histograms of the level
                for (int i = threadIdx.x; i < nb; i += kQHBlock) {
                    const uint32_t c0 = he[i], c1 = he[kQ1 + kQTrash + i];
                    if (level == 0) { if (c0) atomicAdd(&ws[kQHOffH0 + i], c0); }
                    else {
                        uint32_t* Hg = ws + (level == 1 ? kQHOffH1 : kQHOffH2);
                        if (c0) atomicAdd(&Hg[i], c0);
                        if (c1) atomicAdd(&Hg[nb + i], c1);
                    }
                }
            }
            // the level is complete when all its chunks are counted: publish mine, wait for the rest
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) {
                // (what this workgroup published are device atomics, drained above: no L2 write-back to wait for -- agent atomics on both
                //  sides of a hand-off are a valid form, MI355X_MICROARCH.md "Valid forms"; a release fence here was 1.7 us per level)
                if (mine) __hip_atomic_fetch_add(&ws[kQHDone + level], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (__hip_atomic_load(&ws[kQHDone + level], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < chunks) __builtin_amdgcn_s_sleep(8);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            __syncthreads();
            {   // the bin of each open side's rank: half h of the workgroup scans side h's histogram of the level (both at once)
                const uint32_t half = rfl(threadIdx.x >> 8), lt = threadIdx.x & 255u, wl = rfl(lt >> 6), lane = threadIdx.x & 63u;
                const uint32_t nbins = level == 2 ? (uint32_t)kQ3 : (uint32_t)kQ1, per = nbins / 256u;          // 16 or 1 bins per thread
                const uint32_t* Hs = level == 0 ? ws + kQHOffH0 : (level == 1 ? ws + kQHOffH1 + half * kQ2 : ws + kQHOffH2 + half * kQ3);
                const uint32_t want = level == 0 ? (half ? kk[1] : kk[0]) : (level == 1 ? (half ? r0k[1] : r0k[0]) : (half ? r24[1] : r24[0]));
                // the histogram goes through LDS: 16-B loads at consecutive addresses (thread t reading its 16 bins straight from
                // global memory is sixteen loads of 64 scattered lines each -- this stage took 6.6 us of a 20 us level)
                {
                    const uint4* H4 = reinterpret_cast<const uint4*>(Hs);
                    uint4* he4 = reinterpret_cast<uint4*>(he + half * (kQ1 + kQTrash));
                    for (uint32_t i = lt; i < nbins / 4u; i += 256u) he4[i] = H4[i];
                }
                __syncthreads();
                const uint32_t* hl = he + half * (kQ1 + kQTrash);
                uint32_t b[16], sum = 0u;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) { b[j] = j < per ? hl[lt * per + j] : 0u; sum += b[j]; }
                const uint32_t inc = wave_scan_add(sum);
                if (lane == 63u) scratch[half * 4u + wl] = inc;
                __syncthreads();
                uint32_t woff = 0u;
#pragma unroll
                for (uint32_t ww = 0; ww < 4; ww++) woff += ww < wl ? scratch[half * 4u + ww] : 0u;
                const uint32_t excl = woff + inc - sum;
                if (want >= excl && want < excl + sum) {                // one thread per half
                    uint32_t rin = want - excl, digit = lt * per;
#pragma unroll
                    for (uint32_t j = 0; j < 15; j++) if (j + 1u < per && digit == lt * per + j && rin >= b[j]) { rin -= b[j]; digit++; }
                    scratch[8u + half * 2u] = digit; scratch[9u + half * 2u] = rin;
                }
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 2; w++) {
                    if (!(open_mask & (1u << w))) continue;
                    const uint32_t digit = scratch[8 + 2 * w], rin = scratch[9 + 2 * w];
                    if (level == 0) { top[w] = digit; r0k[w] = rin; }
                    else if (level == 1) { p24[w] = (top[w] << 12) | digit; r24[w] = rin; }
                    else low[w] = digit;
                }
                __syncthreads();
            }
        }
    }
    if ((own & open_mask) == 0u) return;
    // ---- the owner of a side that went through the exact passes writes its result and its half of the hint ----
    uint32_t out_key[2], out_valid[2], out_T[2];
    // (one body, instantiated per side: as a loop the compiler stopped unrolling it once the select grew, and every array indexed by
    //  the side -- thresholds, keys, valid words -- moved to scratch)
    auto side_out = [&](auto W) __attribute__((always_inline)) {
        constexpr int w = decltype(W)::value;
        if (!(own & open_mask & (1u << w))) { out_key[w] = 0u; out_valid[w] = 0u; out_T[w] = 0u; return; }      // (block uniform; written above, or another owner's)
        // the side went through the exact passes: leave a threshold that works (rules of F2's and F3's tails)
        const uint32_t V = (p24[w] << 8) | low[w];
        out_key[w] = V;
        const uint32_t k = w ? a.k_lo : a.k_hi;
        const uint32_t inb = ws[kQHOffH0 + top[w]];
        const uint32_t outer = w ? k - r0k[w] : n - (k - r0k[w]) - inb;
        const uint32_t wanted = w ? k + 1u : n - k;
        // a hint that was in use and did not settle this side: the stream is restless, the longest lists from here on (qh_target)
        const uint32_t lv = enabled ? 3u : 0u;
        const uint32_t target = qh_target(wanted, a.wgs, lv);
        const uint32_t limit = umin(q_list_limit(wanted, quantile_spec_cap(n)), kQHListMax);
        const uint32_t need_in = target > outer ? target - outer : 1u;
        const uint32_t r = w ? umin(inb, need_in) - 1u : (inb > need_in ? inb - need_in : 0u);
        select_bin<kQHBlock>(ws + kQHOffH1 + w * kQ2, kQ2, r, scratch, sel);
        const uint32_t m = sel[0], q24 = (top[w] << 12) | m;
        uint32_t listed, Tn;
        bool ok;
        if (w) { listed = outer + (r - sel[1]) + ws[kQHOffH1 + kQ2 + m]; ok = q24 < 0xFFFFFFu; Tn = (q24 + 1u) << 8; }
        else { listed = outer + inb - (r - sel[1]); ok = q24 > 0u; Tn = (q24 << 8) - 1u; }
        ok = ok && listed <= limit;
        if (need_in > inb) {
            // the bucket of the answer (1/8 of a binade) does not hold the list this level asks for: whole first-level buckets beyond
            // it, as many as it takes (coarse -- a bucket can double the list -- and exact again after the next settled call)
            uint32_t cum = outer + inb, b = top[w];
            for (int step = 0; step < 16 && cum < target; step++) {
                if (w ? b >= 0xFFEu : b <= 1u) break;
                b = w ? b + 1u : b - 1u;
                cum += ws[kQHOffH0 + b];
            }
            // (never a list the select could not hold even if it were spread evenly: the same data would fail again, and again)
            const uint32_t room = umin(kQHRoomPerWg * a.wgs, kQHListMax);
            if (b != top[w] && cum <= umin(limit, room - room / 4u)) { listed = cum; ok = true; Tn = w ? (b + 1u) << 20 : (b << 20) - 1u; }
        }
        const uint32_t mult = ws[kQHOffH2 + w * kQ3 + low[w]];
        if (mult / 16u >= wanted + 16u) { Tn = V; ok = true; }          // a heavy tie: the threshold ON the value (1 key in 8 is counted)
        out_valid[w] = ok ? (1u | (lv << 8)) : 0u; out_T[w] = Tn;
        __syncthreads();
    };
    side_out(std::integral_constant<int, 0>{});
    side_out(std::integral_constant<int, 1>{});
    if (threadIdx.x == 0) {
        uint32_t* H = a.hint;
        if (own & open_mask & 1u) { a.dest[0] = key2f(out_key[0]); H[kHValidHi] = out_valid[0]; H[kHTHi] = out_T[0]; }
        if (own & open_mask & 2u) { a.dest[1] = key2f(out_key[1]); H[kHValidLo] = out_valid[1]; H[kHTLo] = out_T[1]; }
    }
}

constexpr long long kQHSmallElems = 4ll << 20;   // up to here every load of a workgroup's share is issued up front (<= 8 per lane)
constexpr int kQHSplitWanted = 2048;
constexpr unsigned kQHHeadsMin = 4u;              // expected keys per filter workgroup and side from which the heads travel with the records
constexpr long long kQHNtElems = 48ll << 20;
// the first call on a hint address takes the general sequence (quantile.hpp: "first call")
static bool quantile_hint_met_before(const uint32_t* hint) {
    static std::mutex lock;
    static std::unordered_set<const void*> met;
    std::lock_guard<std::mutex> guard(lock);
    if (met.size() > (1u << 16)) met.clear();
    return !met.insert((const void*)hint).second;
}
static void quantile_hot_launch(const QHot& a0, hipStream_t s) {
    QHot a = a0;
    const uint32_t full_rows = (a.n >> 2) / kQHBlock;
    uint32_t cap = (uint32_t)num_cu() * 2u;
    if (cap > kQHMaxWg) cap = kQHMaxWg;
    if ((int64_t)a.n <= kQHSmallElems) {
        with_row_share(full_rows, (full_rows + 1) / 2, cap, [&](uint32_t g, auto k) {
            a.wgs = g;
            hipLaunchKernelGGL((quantile_hot_filter_kernel<decltype(k)::value, false, false>), dim3(g), dim3(kQHBlock), 0, s, a);
        });
    } else {
        const uint32_t g = clamp_grid(full_rows / 4, cap);
        a.wgs = g;
        // a filter workgroup is expected to list ~1.5 x wanted / g keys per side: more than the record holds -> the heads travel with
        // the records; lists of thousands of keys -> the two sides are selected by two workgroups
        const uint32_t wanted = a.n - a.k_hi > a.k_lo + 1u ? a.n - a.k_hi : a.k_lo + 1u;
        a.heads = (wanted + wanted / 2u) / g >= kQHHeadsMin ? 1u : 0u;
        a.split = (wanted >= kQHSplitWanted && num_cu() >= 2) ? 1u : 0u;
        if ((int64_t)a.n >= kQHNtElems) hipLaunchKernelGGL((quantile_hot_filter_kernel<2, true, true>), dim3(g), dim3(kQHBlock), 0, s, a);
        else hipLaunchKernelGGL((quantile_hot_filter_kernel<2, true, false>), dim3(g), dim3(kQHBlock), 0, s, a);
    }
    // one workgroup per CU -- the exact passes need the chip -- but half of that for tensors of a few MB: 128 tickets and pollers
    // instead of 256 retire 0.4 us earlier on B, and its exact passes are FASTER with them (61 instead of 73 us: fewer flushes into
    // the shared histograms); from B x 8 up the smaller grid costs the exact passes dearly (B x 32: 219 -> 319 us)
    uint32_t gs = (uint32_t)num_cu();
    if ((int64_t)a.n <= kQHSmallElems && gs > 128u) gs = 128u;
    hipLaunchKernelGGL(quantile_hot_select_kernel, dim3(gs), dim3(kQHBlock), 0, s, a);
}

bool quantile_hot_try(const float* x, int64_t n, float q, float* dest, uint32_t* hint, uint32_t* ws, hipStream_t s) {
    if (hint == nullptr || dest == nullptr || !aligned16(x) || n < kQSpeculateMinElems) return false;
    QHot a;
    a.x = x; a.dest = dest; a.hint = hint; a.ws = ws; a.n = (uint32_t)n;
    a.k_hi = quantile_pos(n, q); a.k_lo = quantile_pos(n, 1 - q); a.wgs = 0; a.split = 0; a.heads = 0; a.pad0 = a.pad1 = 0;
    if (a.n - a.k_hi > kQHWantedMax || a.k_lo + 1u > kQHWantedMax || !quantile_hint_met_before(hint)) return false;
    quantile_hot_launch(a, s);
    return true;
}

}  // namespace ppqhip
