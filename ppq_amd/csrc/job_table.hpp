// job_table.hpp -- what every "_multi" entry point that launches over a table of jobs shares (the convention is stated once in
// DESIGN.md, "Job tables"): the host-side preamble, the padding of a table's tail, the overlap rule for the tensors of one call,
// and the device-side search that maps a workgroup to its job.  Each entry point keeps its own job struct and its own packing.
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#include "common.hpp"

namespace ppqhip {

// the preamble of an entry point: a negative count, or jobs without a table
inline int check_job_table(const char* what, const void* jobs, int num_jobs) {
    if (num_jobs < 0 || (num_jobs > 0 && jobs == nullptr)) { set_error("%s: bad job table", what); return PPQHIP_ERR_INVALID_VALUE; }
    return PPQHIP_OK;
}

// The tail of a table that holds `count` jobs over `blocks` workgroups: jobs[0] again, starting behind the last workgroup, so
// that every byte of the kernel arguments is defined and job_of never lands there.  Args has jobs[], first_block[] and count.
template <typename Args>
inline void pad_job_table(Args& args, uint32_t count, uint32_t blocks) {
    constexpr uint32_t capacity = sizeof(args.jobs) / sizeof(args.jobs[0]);
    static_assert(sizeof(args.first_block) / sizeof(args.first_block[0]) == capacity, "one first_block per job");
    for (uint32_t k = count; k < capacity; k++) { args.jobs[k] = args.jobs[0]; args.first_block[k] = blocks; }
    args.count = count;
}

// No two tensors a call writes may share memory, and none of them may share memory with a tensor the call reads: the jobs of
// one launch run in any order.  A tensor changed in place is an output.  (`outs` is sorted here.)
typedef std::pair<const char*, const char*> Span;
template <typename T>
inline Span span_of(const T* p, int64_t count) { return Span((const char*)p, (const char*)(p + count)); }

inline int check_overlap(const char* what, const std::vector<Span>& ins, std::vector<Span>& outs) {
    std::sort(outs.begin(), outs.end());
    for (size_t k = 1; k < outs.size(); k++) {
        if (outs[k].first < outs[k - 1].second) { set_error("%s: two outputs overlap in memory", what); return PPQHIP_ERR_INVALID_VALUE; }
    }
    for (const Span& in : ins) {                   // the first output that ends behind the input's start must begin at or behind its end
        auto it = std::upper_bound(outs.begin(), outs.end(), in.first, [](const char* p, const Span& o) { return p < o.second; });
        if (it != outs.end() && it->first < in.second) { set_error("%s: an output overlaps an input", what); return PPQHIP_ERR_INVALID_VALUE; }
    }
    return PPQHIP_OK;
}

#if defined(__HIPCC__)

// the job of this workgroup (wave-uniform) and `local`, the workgroup's index inside it: the last job whose first_block is not
// behind blockIdx.x
template <typename Args>
__device__ __forceinline__ uint32_t job_of(const Args& args, uint32_t& local) {
    uint32_t lo = 0, hi = args.count;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (args.first_block[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    local = blockIdx.x - args.first_block[lo];
    return __builtin_amdgcn_readfirstlane(lo);
}

#endif  // __HIPCC__

}  // namespace ppqhip
