// pick.h — the trust-region pick over one segment of rows, stated once for metrics.hip (select_row_kernel: equal segments of B rows,
// the plans of a batch) and guide.hip (goal_pick_kernel: ragged segments, the IK-goal candidates of a scene group).
//
// The rule is the reference's IK-goal filter (infer_serial.py:119-129): everything within volume_trust_region of the minimum volume,
// then the smallest key.
#pragma once
#include "common.h"

namespace edmp {

constexpr int kPickThreads = 256;  // threads of a workgroup that calls block_pick / segment_select

// lexicographic (class, value, index) minimum: the order every selection step reduces under
struct Pick {
    int cls;
    double val;
    int idx;
};
__device__ __forceinline__ bool pick_before(const Pick& a, const Pick& b) {
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.val != b.val) return a.val < b.val;
    return a.idx < b.idx;
}
__device__ __forceinline__ Pick block_pick(Pick mine, Pick* s_pick) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Pick other = {__shfl_xor(mine.cls, o, 64), __shfl_xor(mine.val, o, 64), __shfl_xor(mine.idx, o, 64)};
        if (pick_before(other, mine)) mine = other;
    }
    __syncthreads();  // s_pick may still be read from the previous call
    if (threadIdx.x % kWave == 0) s_pick[threadIdx.x / kWave] = mine;
    __syncthreads();
    Pick best = s_pick[0];
    for (int w = 1; w < kPickThreads / kWave; ++w)
        if (pick_before(s_pick[w], best)) best = s_pick[w];
    return best;
}

// volumes (n,) f32, key (n,) f64 -> the picked index inside the segment, the same value in every thread of the workgroup (all
// kPickThreads threads call it): m = first minimum of the volumes with NaN as the smallest value (argmin_kernel's rule,
// lib/guide.py:650); a NaN minimum keeps m; else among the rows with (double)v_b < (double)v_m + trust the one with the smallest finite
// key; m when no such row has a finite key.  Equal keys: VOL_TIE = false takes the first index; VOL_TIE = true the smaller volume, then
// the first index - the reference's arg-min over the volume-sorted candidate list (infer_serial.py:121-129).
template <bool VOL_TIE>
__device__ __forceinline__ int segment_select(const float* __restrict__ vol, const double* __restrict__ key, int n, double trust, Pick* s_pick) {
    const int tid = threadIdx.x;
    const Pick none = {3, 0.0, 0x7fffffff};
    Pick mine = none;
    for (int b = tid; b < n; b += kPickThreads) {
        const float x = vol[b];
        const Pick c = (x != x) ? Pick{0, 0.0, b} : Pick{1, (double)x, b};
        if (pick_before(c, mine)) mine = c;
    }
    const Pick m = block_pick(mine, s_pick);
    if (m.cls == 0) return m.idx;  // block-uniform: a NaN volume wins as it does in the reference
    const double bound = m.val + trust;
    mine = none;
    for (int b = tid; b < n; b += kPickThreads) {
        const double kb = key[b];
        if ((double)vol[b] < bound && isfinite(kb)) {
            const Pick c = {1, kb, b};
            if (pick_before(c, mine)) mine = c;
        }
    }
    const Pick w = block_pick(mine, s_pick);
    if (w.cls != 1) return m.idx;
    if (!VOL_TIE) return w.idx;
    mine = none;
    for (int b = tid; b < n; b += kPickThreads) {
        const double vb = (double)vol[b];
        if (vb < bound && key[b] == w.val) {
            const Pick c = {1, vb, b};
            if (pick_before(c, mine)) mine = c;
        }
    }
    return block_pick(mine, s_pick).idx;
}

}  // namespace edmp
