// success.hip — geometric success check of every row of the finished batch, on the GPU.
//
// Stands for (reference): RobotEnvironment.benchmark_trajectory (lib/environment.py:632-680) — the plan is executed under
// position control and check_collisions (:591-608) queries contacts between the manipulator and every spawned obstacle:
// cuboids (spawn_collision_cuboids :230-247) and TRUE cylinders (spawn_collision_cylinders :249-268, radius config[7],
// height config[8], axis local z); success = no contact (:672).  The driver tallies it per scene (infer_serial.py:94-99,
// 165-168).  pybullet is a third-party dependency absent offline ("parity unpinned"), so the criterion is geometric and
// exact on the primitives the guide uses for the robot: the 9 link boxes (lib/guide.py:243-342) in float64 modified-DH
// poses against every obstacle, at every waypoint and at `substeps` joint-space interpolated configurations per segment,
// plus the joint-limit test.  The reference only PRINTS "Joint Limits Exceeded" (:659-661); its success is num_collisions == 0
// alone (:672).  Per row the kernel therefore reports three things: first (first colliding waypoint, -1 = collision-free = the
// reference's success), within (all waypoints inside the limits) and ok = within && collision-free, the STRICTER flag; callers
// tally `first < 0` where the reference's number is meant (infer_serial.py, bench.py success_proxy.collision_free_rate) and
// report `ok` beside it.  Checker: oracle/success_oracle.py (same arithmetic, NumPy).
//
// Design: one workgroup per trajectory row, thread = configuration (waypoint i, sub-step s): 197 configurations at N = 50,
// S = 4.  Each thread walks the DH chain in f64 and tests the link boxes riding each frame against the obstacles staged in
// LDS: oriented boxes by the 15-axis separating-axis test, finite cylinders by the exact clipped-polytope test.  The first
// colliding configuration of the row is an LDS integer min — deterministic.  All f64: the decision margin of touching /
// just-separated pairs (1e-9 m in the tests) is far below f32 resolution at arm's length.
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"  // Robot64, robot64_of, SceneSlices, configuration_hits and the box tests: shared with shortcut.hip and selfcol.hip

namespace edmp {

// X (B, 7, N) f64.  flags: ok[B], first[B] (first colliding waypoint, -1 none), within[B] (all waypoints inside the limits).
// Workgroup r stages the boxes and kinds of ITS scene only; everything after the staging is the row's own arithmetic.
__global__ __launch_bounds__(256) void success_rows_kernel(const double* __restrict__ X, int B, int N, int substeps, const double* __restrict__ obb,
                                                           const int32_t* __restrict__ kind, SceneSlices sl, Robot64 rc, int32_t* __restrict__ ok,
                                                           int32_t* __restrict__ first, int32_t* __restrict__ within) {
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ int s_first, s_out;
    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    const int scene = r / sl.rps;
    const int no = min(sl.cnt[scene], EDMP_MAX_OBSTACLES);
    obb += (size_t)sl.off[scene] * 16;
    kind += sl.off[scene];
    for (int i = tid; i < no * 16; i += 256) s_ob[i] = obb[i];
    for (int i = tid; i < no; i += 256) s_kind[i] = kind[i];
    if (tid == 0) {
        s_first = 0x7fffffff;
        s_out = 0;
    }
    __syncthreads();
    const double* xr = X + (size_t)r * 7 * N;
    // joint limits over all waypoints (incl. the pinned start / goal columns)                 lib/environment.py:659-661
    {
        int bad = 0;
        for (int e = tid; e < 7 * N; e += 256) {
            const int j = e / N;
            const double v = xr[e];
            bad |= !(v >= rc.qlo[j] - 1e-9 && v <= rc.qhi[j] + 1e-9);
        }
        if (bad) atomicOr(&s_out, 1);
    }
    const int nc = (N - 1) * substeps + 1;
    for (int c = tid; c < nc; c += 256) {
        const int i = c / substeps, s = c - i * substeps;
        double q[7];
        if (s == 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) q[j] = xr[j * N + i];
        } else {
            const double f = (double)s / (double)substeps;
#pragma unroll
            for (int j = 0; j < 7; ++j) q[j] = interp_joint(xr[j * N + i], xr[j * N + i + 1], f);
        }
        const bool hit = configuration_hits<true>([&](int j) { return q[j]; }, rc, s_ob, s_kind, no);
        if (hit) atomicMin(&s_first, c);
    }
    __syncthreads();
    if (tid == 0) {
        const int fc = s_first;
        const int w = s_out ? 0 : 1;
        first[r] = (fc == 0x7fffffff) ? -1 : fc / substeps;
        within[r] = w;
        ok[r] = (w && fc == 0x7fffffff) ? 1 : 0;
    }
}

// counts[0] = rows ok, [1] = rows within the limits, [2] = rows without a collision, [3] = B; block s counts the rows [s*B, (s+1)*B) into
// quadruple s (grid 1: the whole batch; a scene batch: one block per scene, B = rows per scene)
__global__ void count_flags_kernel(const int32_t* __restrict__ ok, const int32_t* __restrict__ first, const int32_t* __restrict__ within, int B,
                                   int32_t* __restrict__ counts) {
    __shared__ int s[3];
    ok += (size_t)blockIdx.x * B;
    first += (size_t)blockIdx.x * B;
    within += (size_t)blockIdx.x * B;
    counts += 4 * blockIdx.x;
    if (threadIdx.x < 3) s[threadIdx.x] = 0;
    __syncthreads();
    int a = 0, w = 0, f = 0;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        a += ok[i] != 0;
        w += within[i] != 0;
        f += first[i] < 0;
    }
    atomicAdd(&s[0], a);
    atomicAdd(&s[1], w);
    atomicAdd(&s[2], f);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[0] = s[0];
        counts[1] = s[1];
        counts[2] = s[2];
        counts[3] = B;
    }
}

}  // namespace edmp

using namespace edmp;

// flags: room for `rows` rows and `quads` count quadruples; grow-only, from the context's pool
static int ensure_flags(edmp_ctx* ctx, Guide* g, int rows, int quads) {
    if (g->flags && g->flags_B >= rows && g->flags_Q >= quads) return EDMP_OK;
    const int nb = std::max(rows, g->flags_B), nq = std::max(quads, g->flags_Q);
    ctx_release(ctx, g->flags);
    g->flags = nullptr;
    g->flags_B = 0;
    g->flags_Q = 1;
    if (int rc = ctx_alloc(ctx, (void**)&g->flags, ((size_t)3 * nb + 4 * (size_t)nq) * sizeof(int32_t))) return rc;
    g->flags_B = nb;
    g->flags_Q = nq;
    return EDMP_OK;
}

// edmp_scene_set_shapes and edmp_scene_batch_set_shapes behind their own state and count checks: value check and upload of n kinds
static int shapes_set(edmp_ctx* ctx, const int32_t* kind, int n) {
    for (int i = 0; i < n; ++i) EDMP_REQUIRE(kind[i] == 0 || kind[i] == 1, "obstacle %d: kind must be 0 (cuboid) or 1 (cylinder)", i);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    EDMP_HIP_CHECK(hipMemcpyAsync(ctx->guide->kind, kind, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return EDMP_OK;
}

extern "C" int edmp_scene_set_shapes(edmp_ctx* ctx, const int32_t* kind, int n_obstacles) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_scene_set_shapes: call edmp_scene_set first");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_scene_set_shapes");
    EDMP_REQUIRE(kind && n_obstacles == ctx->guide->no, "edmp_scene_set_shapes: need %d kinds (one per obstacle of the scene)", ctx->guide->no);
    return shapes_set(ctx, kind, n_obstacles);
}

extern "C" int edmp_scene_batch_set_shapes(edmp_ctx* ctx, const int32_t* kind, int n_total) {
    EDMP_REQUIRE(ctx, "edmp_scene_batch_set_shapes: null context");
    Guide* g = ctx->guide;
    if (!g || !g->obb || !g->kind) {
        set_error("edmp_scene_batch_set_shapes: call edmp_scene_batch_set first");
        return EDMP_ERR_STATE;
    }
    if (!g->is_batch) {
        set_error("edmp_scene_batch_set_shapes: the bound guide is a single-scene guide (edmp_scene_set); use edmp_scene_set_shapes");
        return EDMP_ERR_STATE;
    }
    const int total = g->scene_off_h.back() + g->scene_no_h.back();
    EDMP_REQUIRE(kind && n_total == total, "edmp_scene_batch_set_shapes: need %d kinds (one per obstacle of the batch's %d scenes, scene after scene), got %d",
                 total, g->S, n_total);
    return shapes_set(ctx, kind, n_total);
}

// the caller's three flag arrays, each replaced by its block of the guide's flags scratch where it is NULL, and the count quadruples
struct FlagPtrs {
    int32_t *ok, *first, *within, *counts;
};
static FlagPtrs flags_or_scratch(const Guide* g, int32_t* ok_dev, int32_t* first_dev, int32_t* within_dev) {
    const size_t fb = (size_t)g->flags_B;
    return {ok_dev ? ok_dev : g->flags, first_dev ? first_dev : g->flags + fb, within_dev ? within_dev : g->flags + 2 * fb, g->flags + 3 * fb};
}

// edmp_success_rows_dev and edmp_scenes_success_rows_dev behind their own state and argument checks: S scenes x rps rows, one count
// quadruple per scene.  batch = false: the one scene of a single-scene guide.
static int success_rows(edmp_ctx* ctx, bool batch, const double* X_dev, int S, int rps, int N, int substeps, const double* dh_f64, int32_t* ok_dev,
                        int32_t* first_dev, int32_t* within_dev, int32_t* counts_host) {
    Guide* g = ctx->guide;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    const int n = S * rps;
    const int32_t* had = g->flags;
    if (int rc = ensure_flags(ctx, g, n, S)) return rc;
    if (batch && g->flags != had) ctx->epoch++;  // (the single-scene call never bumped the epoch for its flags)
    const FlagPtrs f = flags_or_scratch(g, ok_dev, first_dev, within_dev);
    const Robot64 rc = robot64_of(g, dh_f64);
    const SceneSlices sl = scene_slices_of(g, batch, S, rps);
    hipLaunchKernelGGL(success_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, X_dev, n, N, substeps, g->obb, g->kind, sl, rc, f.ok, f.first, f.within);
    EDMP_HIP_CHECK(hipGetLastError());
    if (counts_host) {
        hipLaunchKernelGGL(count_flags_kernel, dim3(S), dim3(256), 0, ctx->stream, f.ok, f.first, f.within, rps, f.counts);
        EDMP_HIP_CHECK(hipGetLastError());
        EDMP_HIP_CHECK(hipMemcpyAsync(counts_host, f.counts, (size_t)S * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return EDMP_OK;
}

extern "C" int edmp_success_rows_dev(edmp_ctx* ctx, const double* X_dev, int B, int N, int substeps, const double* dh_f64, int32_t* ok_dev,
                                     int32_t* first_dev, int32_t* within_dev, int32_t* counts_host) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_success_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_success_rows_dev");
    EDMP_REQUIRE(X_dev && B >= 1 && N >= 2 && substeps >= 1 && substeps <= 64, "edmp_success_rows_dev: need B >= 1, N >= 2, 1 <= substeps <= 64");
    return success_rows(ctx, false, X_dev, 1, B, N, substeps, dh_f64, ok_dev, first_dev, within_dev, counts_host);
}

extern "C" int edmp_scenes_success_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int substeps, const double* dh_f64, int32_t* ok_dev,
                                            int32_t* first_dev, int32_t* within_dev, int32_t* counts_host) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_success_rows_dev");
    EDMP_REQUIRE(X_dev && N >= 2 && substeps >= 1 && substeps <= 64, "edmp_scenes_success_rows_dev: need X, N >= 2 (got %d), 1 <= substeps <= 64 (got %d)", N,
                 substeps);
    return success_rows(ctx, true, X_dev, S, B, N, substeps, dh_f64, ok_dev, first_dev, within_dev, counts_host);
}
