// minmax_fold.hpp -- the comparison and combine steps of the per-tensor running range, shared by every kernel that feeds an
// observer's float[slots][2] accumulator (reduce.hip's streaming kernels, epilogue.hip's statistics variant).  fminf / fmaxf
// drop a NaN operand and order -0.0 below +0.0 (v_min_f32 / v_max_f32), so the folded range has the same bits whatever the
// order in which the elements, lanes, waves and slots are combined -- and whichever kernel combined them.
#pragma once

#include "common.hpp"

namespace ppqhip {

__device__ __forceinline__ void minmax_fold1(float& mn, float& mx, float a) {
    mn = fminf(mn, a);
    mx = fmaxf(mx, a);
}

__device__ __forceinline__ void minmax_fold4(float& mn, float& mx, const float4& v) {
    mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
    mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
}

// (mn, mx) of the whole workgroup, valid in thread 0 afterwards: wave shuffles, then the waves meet in LDS (lds: 32 floats,
// mins at [0, 16), maxs at [16, 32)).  Every thread of the workgroup calls it; it ends WITHOUT a barrier, so a caller
// that reuses `lds` synchronises first.
__device__ __forceinline__ void minmax_block_fold(float& mn, float& mx, float* lds) {
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    if (lane == 0) { lds[wid] = mn; lds[16 + wid] = mx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nw; w++) { mn = fminf(mn, lds[w]); mx = fmaxf(mx, lds[16 + w]); }
}

// fold a workgroup's (mn, mx) into ITS OWN slot: a plain read-modify-write, race free because a launch has one owner per
// slot and launches are stream ordered
__device__ __forceinline__ void minmax_slot_fold(float* slot, float mn, float mx) {
    slot[0] = fminf(mn, slot[0]);
    slot[1] = fmaxf(mx, slot[1]);
}

}  // namespace ppqhip
