// selfcol.hip — exact self-collision check of every row of a batch, on the GPU.
//
// Stands for (reference): the `self_collision` metric of the evaluation package (mpinets/metrics.py:278-292, 351-361; a plan with
// self-collision counts as a physical violation, :505), which asks robofin / pybullet - neither is part of this package.  The criterion
// here is geometric and exact on the primitives the success check uses for the robot: the 9 link boxes (lib/guide.py:243-342) in their
// float64 modified-DH poses, box against box by the 15-axis separating-axis test (linkbox.h: the statements of the success check,
// touching counts as overlap), at the success check's own configurations - every waypoint plus `substeps - 1` joint-space interpolants
// per segment, nc = (N - 1) * substeps + 1.  The link boxes are AABBs of meshes, so neighbouring links overlap by construction: WHICH
// pairs (a, b), a < b, count is the caller's (9, 9) mask (franka.self_collision_pairs(): joint-frame indices at least 3 apart).
//
// Per row: the smallest key c * 81 + a * 9 + b over all (configuration c, masked pair (a, b)) whose boxes overlap - an integer LDS
// minimum, so the answer is deterministic and depends on the row alone.  first = c / substeps (the waypoint index of the first colliding
// configuration, -1 none), pair = a * 9 + b (the first masked pair in row-major order that overlaps THERE, -1 none).
//
// Design (linkbox.h: PairPlan, configuration_self_hit hold the plan and the work item's body): one 256-thread workgroup per row, all f64 (the decision margin of the tests, 1e-9 m, is far below f32 resolution at arm's
// length).  A work item is (configuration c, lower link a with a non-empty mask row): it walks the chain to a's frame, keeps that ONE box
// pose (12 doubles), walks on and tests each masked b > a as its frame arrives (LINK_FRAME is monotone, so b's frame never precedes
// a's), stopping at its first hit - b ascends, so that hit is the item's smallest key - or after the last frame a masked b rides.
// Re-walking the chain per a costs a few sincos; holding nine f64 frames per thread would cost the registers.  The joint loop is not
// unrolled and holds no per-thread array indexed by the joint number: the joint values come from global memory as they are needed and
// every table index (joint, link) is uniform over the lanes still in the loop - its trip count (the last frame a masked b rides) and
// the early stop do differ from lane to lane -, so nothing lives in scratch.  Items are handed out in key order
// (w = c * na + item), so a thread leaves its loop as soon as the row's minimum so far lies below everything it could still find: a
// benign race that changes the work done, never the result.  Checker: tests/self_collision_inputs.py (oracle/success_oracle.py, NumPy).
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"

namespace edmp {

constexpr int kNoKey = 0x7fffffff;

// X (n, 7, N) f64.  first[n], pair[n] (either may be NULL)
__global__ __launch_bounds__(256) void self_collision_rows_kernel(const double* __restrict__ X, int N, int substeps, PairPlan plan, Robot64 rc,
                                                                  int32_t* __restrict__ first, int32_t* __restrict__ pair) {
    __shared__ int s_key;
    __shared__ int s_a[EDMP_N_LINKS - 1], s_bits[EDMP_N_LINKS - 1], s_jlast[EDMP_N_LINKS - 1];
    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) s_key = kNoKey;
    if (tid < plan.na) {  // (the item index differs from lane to lane: the plan goes to LDS, the kernel arguments stay uniformly indexed)
        s_a[tid] = plan.a[tid];
        s_bits[tid] = plan.bits[tid];
        s_jlast[tid] = plan.jlast[tid];
    }
    __syncthreads();
    const double* xr = X + (size_t)r * 7 * N;
    const int na = plan.na;
    const int items = ((N - 1) * substeps + 1) * na;
    for (int w = tid; w < items; w += 256) {
        const int c = w / na, it = w - c * na;
        const int a = s_a[it], bits = s_bits[it], jlast = s_jlast[it];
        // the smallest key this item - and every later item of this thread - could bring
        if (c * 81 + a * 9 >= __hip_atomic_load(&s_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        const int i = c / substeps, s = c - i * substeps;
        const double f = (double)s / (double)substeps;
        // the success check's interpolation expression                                         success.hip: success_rows_kernel
        const int hit = configuration_self_hit(
            [&](int j) { return (s == 0) ? xr[j * N + i] : (1.0 - f) * xr[j * N + i] + f * xr[j * N + i + 1]; }, rc, a, bits, jlast);
        if (hit >= 0) atomicMin(&s_key, c * 81 + a * 9 + hit);
    }
    __syncthreads();
    if (tid == 0) {
        const int key = s_key;
        if (first) first[r] = (key == kNoKey) ? -1 : (key / 81) / substeps;
        if (pair) pair[r] = (key == kNoKey) ? -1 : key % 81;
    }
}

}  // namespace edmp

using namespace edmp;

extern "C" int edmp_self_collision_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, int substeps, const double* dh_f64,
                                            const int32_t* pair_mask, int32_t* first_dev, int32_t* pair_dev) {
    EDMP_REQUIRE(ctx, "edmp_self_collision_rows_dev: null context");
    if (!ctx->guide || !ctx->guide->obb) {
        set_error("edmp_self_collision_rows_dev: no guide bound (edmp_scene_set or edmp_scene_batch_set first: the link boxes are the bound guide's)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(X_dev && pair_mask, "edmp_self_collision_rows_dev: X_dev and pair_mask must not be NULL");
    EDMP_REQUIRE(n >= 1 && N >= 2 && substeps >= 1 && substeps <= 64,
                 "edmp_self_collision_rows_dev: need n >= 1 (got %d), N >= 2 (got %d), 1 <= substeps <= 64 (got %d)", n, N, substeps);
    // the key c * 81 + a * 9 + b and the item index c * na + item are 32-bit
    EDMP_REQUIRE(((int64_t)(N - 1) * substeps + 1) * 81 < (int64_t)kNoKey, "edmp_self_collision_rows_dev: (N - 1) * substeps + 1 = %lld configurations per row, the key holds %d",
                 (long long)((int64_t)(N - 1) * substeps + 1), kNoKey / 81);
    PairPlan plan;
    int bad_a = 0, bad_b = 0;
    if (!pair_plan_of(pair_mask, &plan, &bad_a, &bad_b))
        EDMP_REQUIRE(false, "edmp_self_collision_rows_dev: pair_mask[%d][%d] = %d, mask entries are 0 or 1", bad_a, bad_b, (int)pair_mask[bad_a * EDMP_N_LINKS + bad_b]);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    if (plan.na == 0 || (!first_dev && !pair_dev)) {  // an all-zero mask: -1 everywhere, no chain to walk
        if (first_dev) EDMP_HIP_CHECK(hipMemsetAsync(first_dev, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
        if (pair_dev) EDMP_HIP_CHECK(hipMemsetAsync(pair_dev, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
        return EDMP_OK;
    }
    const Robot64 rc = robot64_of(ctx->guide, dh_f64);
    hipLaunchKernelGGL(self_collision_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, X_dev, N, substeps, plan, rc, first_dev, pair_dev);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}
