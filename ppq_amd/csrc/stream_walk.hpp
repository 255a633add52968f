// stream_walk.hpp -- THE walks of the calibration statistics: min/max (reduce.hip), histograms (hist.hip)
// and the quantile filters (quantile.hip, quantile_hot.hip) stream their tensors with the templates below and bring only what
// differs: what happens to a float4, to a lone element, and at the begin and the end of a job.
//
//   ping_pong   two register tiles; the next one is in flight while the current one is consumed
//   tile_walk   MANY tensors, one launch: the concatenated tiles of all jobs, split evenly over a chip-sized persistent grid
//   row_walk    ONE tensor with its arguments by value: the latency-bound sizes, and the ping-pong form without a job table
//
// What shaped them (MI355X; every finding is stated here once):
//   * Loads are CLAMPED, never predicated: the index of a prefetch past the end is clamped to the last tile / row (wave uniform),
//     which is fetched again and not consumed.  A load under `if (k < cnt)` lands in its own basic block and the compiler waits
//     for ALL earlier loads in front of it.
//   * The first tile is requested BEFORE anything else a workgroup has to do (`ready`: zeroing its LDS histogram, reading a
//     hint, deriving thresholds): on a tensor of a few MB a launch is one latency chain and nothing else hides that work.  What
//     runs there must not drain vmcnt: an LDS-only wait and the bare s_barrier, not __syncthreads().
//   * Everything handed to a walk must be INLINED into its loop: behind a call the compiler no longer knows the state of vmcnt,
//     and every wait of the loop becomes vmcnt(0) -- also for the tile just prefetched.
//   * Loads through a pointer that comes out of a device-resident table must name the address space (GlobalLoads, quantile.hpp):
//     the compiler would emit FLAT loads, which tick lgkmcnt too and return out of order with LDS traffic -- vmcnt(0) again.
//   * Job fields reach a walk by value (begin returns them), and the walk's pointers carry no __restrict__: see fq_walk.hpp.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "job_table.hpp"

namespace ppqhip {

// ---- host -----------------------------------------------------------------------------------------------------------------------
// tiles of `tile_vec` float4 a job of n elements takes in a tile walk: its full tiles and one ragged tail tile, or -- a tensor
// that is not 16-B aligned -- every tile through the masked 4-B path
__host__ __device__ inline uint32_t stream_job_tiles(uint32_t n, bool vec_ok, uint32_t tile_vec) {
    const uint32_t tile_elems = tile_vec * 4;
    if (!vec_ok) return (n + tile_elems - 1) / tile_elems;
    const uint32_t full = (n >> 2) / tile_vec;
    return full + (n > full * tile_elems ? 1u : 0u);
}

// One launch's chunk of a job list: args.job[k] <- jobs[base + k] (x, n and first_tile here, the rest by set(dst, src)), count and
// total_tiles.  Returns the elements of the chunk (the streaming-load threshold looks at them).
template <typename Args, typename Job, typename Set>
inline int64_t fill_stream_jobs(Args& args, const Job* jobs, int base, int num_jobs, uint32_t tile_vec, Set set) {
    constexpr int capacity = sizeof(args.job) / sizeof(args.job[0]);
    args.count = (uint32_t)((num_jobs - base) < capacity ? (num_jobs - base) : capacity);
    uint32_t tiles = 0;
    int64_t elems = 0;
    for (uint32_t k = 0; k < args.count; k++) {
        const Job& src = jobs[base + k];
        args.job[k].x = src.x; args.job[k].n = (uint32_t)src.n; args.job[k].first_tile = tiles;
        set(args.job[k], src);
        tiles += stream_job_tiles((uint32_t)src.n, aligned16(src.x), tile_vec);
        elems += src.n;
    }
    args.total_tiles = tiles;
    return elems;
}

inline uint32_t clamp_grid(uint32_t want, uint32_t cap) { return want > cap ? cap : (want < 1 ? 1u : want); }

// The row walk's latency-bound form: launch(grid, std::integral_constant<int, K>) with the grid the caller wants, clamped to
// [1, cap], and K = 2 | 4 | 8 rows per lane so that the largest share is in flight at once (shares beyond 8 rows take several trips)
template <typename Launch>
inline void with_row_share(uint32_t full_rows, uint32_t want, uint32_t cap, Launch launch) {
    const uint32_t grid = clamp_grid(want, cap);
    const uint32_t share = (full_rows + grid - 1) / grid;
    if (share <= 2) launch(grid, std::integral_constant<int, 2>());
    else if (share <= 4) launch(grid, std::integral_constant<int, 4>());
    else launch(grid, std::integral_constant<int, 8>());
}

// launch(std::bool_constant<..>, ..) for run-time flags (the histograms' asymmetric, clip_outliers and streaming loads), like
// with_tile_shape (fq_walk.hpp)
template <typename Launch>
inline void with_flags(Launch launch) { launch(); }
template <typename Launch, typename... Rest>
inline void with_flags(Launch launch, bool first, Rest... rest) {
    if (first) with_flags([&](auto... t) { launch(std::true_type(), t...); }, rest...);
    else with_flags([&](auto... t) { launch(std::false_type(), t...); }, rest...);
}

#if defined(__HIPCC__)

// ---- device ---------------------------------------------------------------------------------------------------------------------
// how a walk reads: the 16-B load of the full tiles / rows and the 4-B load of the masked paths
template <bool NT>
struct PlainLoads {
    static __device__ __forceinline__ float4 v4(const float4* p) { return load4<NT>(p); }
    static __device__ __forceinline__ float v1(const float* p) { return *p; }
};

// Indices k, k + STEP, .. below end (k < end); `a` holds index k already: whatever the caller does between that first fetch and
// this loop runs behind the loads.  fetch(buf, index) issues a tile's loads, consume(buf, index) uses them.
template <int STEP, int K, typename Fetch, typename Consume>
__device__ __forceinline__ void ping_pong(float4 (&a)[K], float4 (&b)[K], uint32_t k, uint32_t end, Fetch fetch, Consume consume) {
    for (;;) {
        fetch(b, min(k + STEP, end - 1));
        consume(a, k);
        k += STEP;
        if (k >= end) break;
        fetch(a, min(k + STEP, end - 1));
        consume(b, k);
        k += STEP;
        if (k >= end) break;
    }
}

// the job a tile walk is about to stream
struct StreamJob {
    const float* x;
    uint32_t n;
};

// first_tile read out of the kernel arguments (MinMaxJobs, HistJobs: the table travels by value)
template <typename Jobs>
struct ArgTiles {
    const Jobs& jobs;
    __device__ __forceinline__ uint32_t count() const { return jobs.count; }
    __device__ __forceinline__ uint32_t total() const { return jobs.total_tiles; }
    __device__ __forceinline__ void stage() const {}
    __device__ __forceinline__ uint32_t first(uint32_t j) const { return jobs.job[j].first_tile; }
};

// Tiles of BLOCK * U float4.  The workgroup takes its even share [t, t_end) of tiles.total() and walks the jobs it covers: the
// job of tile t is the last one whose first tile is not behind t (tiles.first(j), after tiles.stage()).  Per job, tiles [k, k1):
//     begin(j, k)            -> StreamJob (the tensor, by value)
//     ready()                once per job, behind the loads of its first full tile (at once where it has none here); false: leave
//                            this job (no end)
//     consume(buf, k)        a full tile, U float4 per lane
//     tail(value, in, r)     the ragged tail tile, or every tile of a tensor that is not 16-B aligned: 4 * U masked elements per lane
//     end(j)
// A workgroup beyond the last tile (blockIdx.x >= tiles.total()) has an empty share: nothing is called.
template <int BLOCK, int U, typename Loads, typename Tiles, typename Begin, typename Ready, typename Consume, typename Tail, typename End>
__device__ __forceinline__ void tile_walk(const Tiles& tiles, Begin begin, Ready ready, Consume consume, Tail tail, End end) {
    constexpr uint32_t kVec = (uint32_t)BLOCK * U, kElems = kVec * 4;
    uint32_t t, t_end;
    even_split(tiles.total(), gridDim.x, blockIdx.x, t, t_end);
    if (t >= t_end) return;
    tiles.stage();
    uint32_t lo = 0, hi = tiles.count();       // wave uniform
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tiles.first(mid) <= t) lo = mid; else hi = mid;
    }
    for (uint32_t j = lo; t < t_end; j++) {
        const uint32_t first = tiles.first(j);
        const uint32_t j_end = (j + 1 < tiles.count()) ? tiles.first(j + 1) : tiles.total();
        uint32_t k = t - first;
        const uint32_t k1 = min(t_end, j_end) - first;
        t = min(t_end, j_end);
        const StreamJob job = begin(j, k);
        const float* x = job.x;
        const uint32_t n = job.n;
        const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
        const uint32_t full = vec_ok ? (n >> 2) / kVec : 0u;
        const uint32_t kf = min(k1, full);                                 // full tiles [k, kf)
        const float4* xv = reinterpret_cast<const float4*>(x) + threadIdx.x;
        float4 bufa[U], bufb[U];
        auto fetch = [&](float4 (&buf)[U], uint32_t tile) {
            const float4* p = xv + (size_t)tile * kVec;
#pragma unroll
            for (int u = 0; u < U; u++) buf[u] = Loads::v4(p + u * BLOCK);
        };
        // (ready() stands in the block of the loads it hides behind: after a join the compiler waits for them first)
        if (k < kf) {
            fetch(bufa, k);
            if (!ready()) continue;
            ping_pong<1>(bufa, bufb, k, kf, fetch, consume);
            k = kf;
        } else if (!ready()) continue;
        for (; k < k1; k++) {
            const uint32_t e0 = k * kElems + threadIdx.x;
#pragma unroll 4
            for (int r = 0; r < 4 * U; r++) {
                const uint32_t i = e0 + r * BLOCK;
                const bool in = i < n;
                tail(in ? Loads::v1(x + i) : 0.f, in, r);
            }
        }
        end(j);
    }
}

// Rows of BLOCK float4 of one 16-B aligned tensor.  The workgroup takes its even share [r0, r1) of the full rows, K rows per trip
// (clamped at r1 - 1: duplicates are loaded, not consumed), with one register tile or, PING, two.  Workgroup G - 1 also takes the
// ragged rest: less than BLOCK float4 and n % 4 elements.
//     ready()                behind the loads of the first trip; false: leave (returns false)
//     consume(buf, cnt)      K float4 per lane, the first cnt rows of them real (workgroup uniform)
//     rest(value, in, t)     trip t of the rest, masked
template <int BLOCK, int K, bool PING, typename Loads, typename Ready, typename Consume, typename Rest>
__device__ __forceinline__ bool row_walk(const float* x, uint32_t n, Ready ready, Consume consume, Rest rest) {
    const uint32_t G = gridDim.x, g = blockIdx.x;
    const uint32_t full_rows = (n >> 2) / BLOCK;
    uint32_t r0, r1;
    even_split(full_rows, G, g, r0, r1);
    const float4* xv = reinterpret_cast<const float4*>(x) + threadIdx.x;
    float4 bufa[K], bufb[K];
    auto fetch = [&](float4 (&buf)[K], uint32_t r) {
#pragma unroll
        for (int k = 0; k < K; k++) buf[k] = Loads::v4(xv + (size_t)min(r + (uint32_t)k, r1 - 1) * BLOCK);
    };
    auto eat = [&](const float4 (&buf)[K], uint32_t r) { consume(buf, min((uint32_t)K, r1 - r)); };
    if (r0 < r1) fetch(bufa, r0);
    if (!ready()) return false;
    if (r0 < r1) {
        if (PING) ping_pong<K>(bufa, bufb, r0, r1, fetch, eat);
        else {
            for (uint32_t r = r0;;) {
                eat(bufa, r);
                r += K;
                if (r >= r1) break;
                fetch(bufa, r);
            }
        }
    }
    if (g == G - 1) {
        const uint32_t e0 = full_rows * BLOCK * 4;
        const uint32_t trips = (n - e0 + BLOCK - 1) / BLOCK;
        for (uint32_t t = 0; t < trips; t++) {
            const uint32_t i = e0 + t * BLOCK + threadIdx.x;
            const bool in = i < n;
            rest(in ? Loads::v1(x + i) : 0.f, in, t);
        }
    }
    return true;
}

#endif  // __HIPCC__

}  // namespace ppqhip
