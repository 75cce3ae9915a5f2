// blend.hip — parabolic corner blends of finished rows under the exact collision check: the choice of beta, for motions that may leave the
// polyline by a bounded amount.  The blended path is timed and sampled by timing.hip (the blended instantiations of its two kernels).
//
// On the polyline every real corner carries a velocity-jump cap and the arm all but stops there.  Here corner i is replaced by the
// quadratic Bezier curve with the control points x_i - beta d_{i-1}, x_i, x_i + beta d_i, traversed at constant acceleration:
//   q(u) = x_i + beta (u^2 d_i - (1 - u)^2 d_{i-1}),  u in [0, 1];  d_i = x_{i+1} - x_i,  Delta_i = d_i - d_{i-1}.
// It leaves the polyline by at most beta |Delta_ij| / 4 in joint j (at u = 1/2), meets both segments tangentially, and at the path speed
// sqrt y has the constant joint acceleration y Delta_i / (2 beta).  include/edmp_hip.h states the rule in full; tests/blend_inputs.py
// is its host statement.  All f64, every operation rounded on its own.
//
// blend_rows_kernel chooses beta.  ONE 256-thread workgroup per listed row; the row and its scene's obstacles live in LDS as in
// shortcut_rows_kernel.  Thread i < N owns waypoint i: it forms V, J, K and beta0 of its corner once and keeps the corner's state in
// LDS entries of its own (the test then has every register to itself: 230 VGPRs, no scratch).  Per halving h the owners publish which corners are tried and at which beta (three LDS values per corner), one
// __syncthreads_or both orders that and tells every thread whether any corner is still tried (no: the loop ends for all 256 alike),
// then thread = (corner, k), strided, tests the K_b + 1 configurations of every tried corner with the success check's own test
// (linkbox.h: configuration_hits) and raises the corner's hit flag; behind the next barrier the owners read their flag.  No atomics,
// rows are independent.  An accepted blend was tested at exactly the configurations q(k / K_b), k = 0..K_b, the two ends included.
//
// SELF (the *_self_dev entry points with a non-zero pair mask): a try must also leave the arm free of itself at those configurations
// (linkbox.h: configuration_self_hit, the work item of self_collision_rows_kernel).  The items of a halving become (configuration, test),
// test-major: the E = (N - 2)(K_b + 1) obstacle items, padded to a multiple of 64 so that a wave runs one kind of test, then the na E
// self items, lower link after lower link.  Two LDS flags per tried corner: an obstacle item is skipped only when the corner's obstacle
// flag is up, a self item when either is up; the try is rejected if either is up and counts in self_hits iff the obstacle flag is down
// and the self flag up - which depends on the inputs only.  SELF = false is the kernel as it was: self-collision is then NOT tested.
#include <cmath>

#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"  // Robot64, SceneSlices, configuration_hits: shared with success.hip and shortcut.hip
#include "rowlist.h"  // check_limits, check_rows, rows_upload, rows_call_end: shared with shortcut.hip and timing.hip

// every operation of the rule is rounded on its own (the host rule's): no fused multiply-add in this file's own code
#pragma clang fp contract(off)

namespace edmp {

constexpr int kBlendN = 64;             // waypoints per row at most: the LDS row stride
constexpr double kBlendMaxReach = 0.45; // two neighbouring blends leave l >= 0.1 of their segment
constexpr int kPending = -2;            // a corner that is still to be tried (never written out)

struct BlendArgs {
    const double* X;      // (n, 7, N)
    const int32_t* rows;  // the listed rows, or nullptr = row = workgroup
    int N, K, H;
    double reach;
    double vmax[7], amax[7], jump[7], dev[7];
    const double* obb;    // the guide's obstacle table and kinds
    const int32_t* kind;
    double* beta;         // (n, N)
    int32_t* code;        // (n, N)
    int32_t* halved;      // (n, N)
    int32_t* tested;      // (n,)
};

// what the SELF kernel takes beside today's arguments: the one element of its argument pack (the SELF = false kernel's pack is empty - it
// is launched with today's arguments, and nothing else)
struct BlendSelf {
    PairPlan plan;
    int32_t* self_hits;  // (n, N)
};

template <bool SELF, class... Self>
__global__ __launch_bounds__(256) void blend_rows_kernel(BlendArgs a, SceneSlices sl, Robot64 rc, Self... self_pack) {
    static_assert(sizeof...(Self) == (SELF ? 1 : 0), "the SELF kernel takes ONE more argument, the plain kernel none");
    const auto& sf = self_arguments(self_pack...);  // (BlendSelf, or nothing to read)
    __shared__ double s_x[7 * kBlendN];  // the row
    __shared__ double s_beta[kBlendN];   // the beta under test of each corner
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ double s_b0[kBlendN], s_K[kBlendN], s_J2[kBlendN], s_out[kBlendN];  // per corner: beta0, K, J^2 and the beta that was kept
    __shared__ int s_try[kBlendN], s_hit[kBlendN], s_cnt[kBlendN], s_code[kBlendN], s_halved[kBlendN];
    __shared__ int s_bad;
    __shared__ int s_self[kBlendN], s_scnt[kBlendN];  // (SELF only: unused ones take no LDS) the self flag, the tries the self test alone rejected
    __shared__ int s_pa[EDMP_N_LINKS - 1], s_pbits[EDMP_N_LINKS - 1], s_pjlast[EDMP_N_LINKS - 1];
    const int tid = threadIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[blockIdx.x] : (int)blockIdx.x);
    const int scene = __builtin_amdgcn_readfirstlane(r / sl.rps);  // (one row, one scene: workgroup-uniform)
    int N_ = __builtin_amdgcn_readfirstlane(a.N), K_ = __builtin_amdgcn_readfirstlane(a.K), H_ = __builtin_amdgcn_readfirstlane(a.H);
    // SELF: N, K and H arrive as ONE 128-bit scalar load that lives through the whole kernel; under the SELF kernel's scalar pressure the
    // allocator spills that tuple, rematerialises it instead and leaves the 16-byte slot behind - a private segment nobody touches.  Three
    // registers of their own end the tuple here (an empty statement, no instruction).  This steers one version of one allocator:
    // tests/test_code_objects.py::test_no_kernel_uses_scratch is the guard, and the statement can go once the kernel passes it without
    // (a compiler that no longer leaves the dead slot behind)
    if constexpr (SELF) asm volatile("" : "+s"(N_), "+s"(K_), "+s"(H_));
    const int N = N_, K = K_, H = H_;
    const int no = min(sl.cnt[scene], EDMP_MAX_OBSTACLES);
    const double* obb = a.obb + (size_t)sl.off[scene] * 16;
    const int32_t* kind = a.kind + sl.off[scene];
    const double* xr = a.X + (size_t)r * 7 * N;
    if (tid == 0) s_bad = 0;
    if (tid < kBlendN) s_try[tid] = s_hit[tid] = s_cnt[tid] = 0;
    int na = 0;
    if constexpr (SELF) {
        na = __builtin_amdgcn_readfirstlane(sf.plan.na);
        if (tid < kBlendN) s_self[tid] = s_scnt[tid] = 0;
        if (tid < na) {  // (the item's plan entry differs from lane to lane: the plan goes to LDS, the kernel arguments stay uniformly indexed)
            s_pa[tid] = sf.plan.a[tid];
            s_pbits[tid] = sf.plan.bits[tid];
            s_pjlast[tid] = sf.plan.jlast[tid];
        }
    }
    __syncthreads();
    for (int i = tid; i < no * 16; i += 256) s_ob[i] = obb[i];
    for (int i = tid; i < no; i += 256) s_kind[i] = kind[i];
    for (int e = tid; e < 7 * N; e += 256) {
        const int j = e / N, m = e - j * N;
        const double v = xr[e];
        s_x[j * kBlendN + m] = v;
        if (!isfinite(v)) s_bad = 1;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_bad)) {  // (one LDS value behind a barrier: the whole workgroup leaves) the row is left alone
        if (tid < N) {
            a.beta[(size_t)r * N + tid] = __builtin_nan("");
            a.code[(size_t)r * N + tid] = -1;
            a.halved[(size_t)r * N + tid] = 0;
            if constexpr (SELF) sf.self_hits[(size_t)r * N + tid] = 0;
        }
        if (tid == 0) a.tested[r] = 0;
        return;
    }
    // the owner of waypoint tid: what its corner is, once.  The corner's state lives in LDS, written and read by its owner alone: the
    // test between the barriers below has every register to itself
    const double kInf = __builtin_inf();
    const bool owner = tid < N;
    if (owner) {
        double Vp = kInf, V = kInf, J = kInf, Kc = kInf, b0 = a.reach;
        bool zp = true, z = true, flat = true;
        const bool corner = tid >= 1 && tid < N - 1;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double x0 = s_x[j * kBlendN + tid];
            const double dp = corner ? x0 - s_x[j * kBlendN + tid - 1] : 0.0, d = corner ? s_x[j * kBlendN + tid + 1] - x0 : 0.0;
            const double adp = fabs(dp), ad = fabs(d), adl = fabs(d - dp);
            zp = zp && adp == 0.0;
            z = z && ad == 0.0;
            flat = flat && adl == 0.0;
            // a limit over 0 is +inf and never the minimum, which leaves that joint out
            const double qvp = a.vmax[j] / adp, qv = a.vmax[j] / ad, qj = a.jump[j] / adl, qk = a.amax[j] / adl, qb = (4.0 * a.dev[j]) / adl;
            Vp = qvp < Vp ? qvp : Vp;
            V = qv < V ? qv : V;
            J = qj < J ? qj : J;
            Kc = qk < Kc ? qk : Kc;
            b0 = qb < b0 ? qb : b0;
        }
        const double V2p = Vp * Vp, V2 = V * V, J2 = J * J;
        const double vm = V2 < V2p ? V2 : V2p;
        // 0: nothing to blend (an end, a zero segment beside it, no corner); 1: the corner cap does not bind; kPending: to be tried
        s_code[tid] = (zp || z || flat) ? 0 : !(J2 < vm) ? 1 : kPending;
        s_b0[tid] = b0;
        s_K[tid] = Kc;
        s_J2[tid] = J2;
        s_out[tid] = 0.0;
        s_halved[tid] = 0;
    }
    double scale = 1.0;  // 2^-h
    for (int h = 0; h <= H; ++h, scale = scale * 0.5) {
        int mytry = 0;
        if (owner && s_code[tid] == kPending) {
            const double b = s_b0[tid] * scale;
            if (!((2.0 * b) * s_K[tid] > s_J2[tid])) {  // the blend's cap is no better than the jump cap: no gain
                s_code[tid] = 2;
            } else {
                s_beta[tid] = b;
                s_hit[tid] = 0;
                if constexpr (SELF) s_self[tid] = 0;
                mytry = 1;
            }
        }
        if (tid < kBlendN) s_try[tid] = mytry;
        if (!__syncthreads_or(mytry)) break;  // (one value for all 256 threads) no corner is tried any more
        for (int e = tid; e < (N - 2) * (K + 1); e += 256) {
            const int i = 1 + e / (K + 1), k = e - (i - 1) * (K + 1);
            if (!s_try[i] || *(volatile int*)&s_hit[i]) continue;  // somebody has hit already: less work, the same result
            const double u = (double)k / (double)K, b = s_beta[i];
            const double uu = u * u, w = 1.0 - u;
            const double ww = w * w;
            const double* xi = s_x + i;
            const bool hit = configuration_hits<false>(
                [&](int j) {
                    const double x0 = xi[j * kBlendN];
                    const double dp = x0 - xi[j * kBlendN - 1], d = xi[j * kBlendN + 1] - x0;
                    return x0 + b * (uu * d - ww * dp);
                },
                rc, s_ob, s_kind, no);
            if (hit) s_hit[i] = 1;
        }
        if constexpr (SELF) {
            // the self items behind the obstacle items: item = (lower link of the plan, corner, k), link-major
            // item w of the whole list runs on thread w % 256: self item s = w - Ep starts on the wave behind the obstacle items' last one
            const int E = (N - 2) * (K + 1), Ep = (E + 63) & ~63;
            for (int w = Ep + ((tid - Ep) & 255); w < Ep + na * E; w += 256) {
                const int it = (w - Ep) / E, e = (w - Ep) - it * E;
                const int i = 1 + e / (K + 1), k = e - (i - 1) * (K + 1);
                if (!s_try[i] || *(volatile int*)&s_hit[i] || *(volatile int*)&s_self[i]) continue;  // rejected already: less work, the same result
                const double u = (double)k / (double)K, b = s_beta[i];
                const double uu = u * u, w1 = 1.0 - u;
                const double ww = w1 * w1;
                const double* xi = s_x + i;
                const int lb = configuration_self_hit(
                    [&](int j) {
                        const double x0 = xi[j * kBlendN];
                        const double dp = x0 - xi[j * kBlendN - 1], d = xi[j * kBlendN + 1] - x0;
                        return x0 + b * (uu * d - ww * dp);
                    },
                    rc, s_pa[it], s_pbits[it], s_pjlast[it]);
                if (lb >= 0) s_self[i] = 1;
            }
        }
        __syncthreads();
        if (mytry) {  // (corner tid's entries are touched by its owner alone from here to the next barrier)
            s_cnt[tid] += K + 1;
            bool self_hit = false;
            if constexpr (SELF) {
                self_hit = s_self[tid] != 0;
                if (!s_hit[tid] && self_hit) s_scnt[tid] += 1;  // the obstacle test passed this try, the self test alone rejected it
            }
            if (!s_hit[tid] && !self_hit) {
                s_code[tid] = 3;
                s_out[tid] = s_beta[tid];
                s_halved[tid] = h;
            } else if (h == H) {
                s_code[tid] = 4;
            }
        }
    }
    if (owner) {
        a.beta[(size_t)r * N + tid] = s_out[tid];
        a.code[(size_t)r * N + tid] = s_code[tid];
        a.halved[(size_t)r * N + tid] = s_halved[tid];
        if constexpr (SELF) sf.self_hits[(size_t)r * N + tid] = s_scnt[tid];
    }
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int m = 1; m < N - 1; ++m) total += s_cnt[m];
        a.tested[r] = total;
    }
}

}  // namespace edmp

using namespace edmp;

// edmp_blend_rows_dev and edmp_scenes_blend_rows_dev behind their own state checks: n = S x rps rows of X (n, 7, N).  Every refusal
// comes before any device call.  self: the *_self_dev entry points - the SELF kernel with the mask's plan, or, for an all-zero mask,
// today's kernel and a zero-filled self_hits.
static int blend_rows(edmp_ctx* ctx, const char* what, bool batch, const double* X_dev, int S, int rps, int N, const int32_t* rows_host, int n_rows,
                      const double* vmax, const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                      const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev,
                      const int32_t* pair_mask = nullptr, int32_t* self_hits_dev = nullptr, bool self = false) {
    Guide* g = ctx->guide;
    const int n = S * rps;
    EDMP_REQUIRE(X_dev && beta_dev && code_dev && halved_dev && tested_dev, "%s: null pointer", what);
    EDMP_REQUIRE(N >= 2 && N <= kBlendN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kBlendN, N);
    EDMP_REQUIRE(substeps >= 1 && substeps <= 8, "%s: substeps %d outside 1..8", what, substeps);
    EDMP_REQUIRE(halvings >= 0 && halvings <= 8, "%s: halvings %d outside 0..8", what, halvings);
    EDMP_REQUIRE(std::isfinite(reach) && reach > 0.0 && reach <= kBlendMaxReach, "%s: reach %g outside (0, %g]", what, reach, kBlendMaxReach);
    if (int rc = check_limits(what, "vmax", vmax)) return rc;
    if (int rc = check_limits(what, "amax", amax)) return rc;
    if (int rc = check_limits(what, "jump", jump)) return rc;
    if (int rc = check_limits(what, "deviation", deviation)) return rc;
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;
    BlendSelf sf = {};
    if (self) {
        EDMP_REQUIRE(pair_mask && self_hits_dev, "%s: pair_mask and self_hits_dev must not be NULL", what);
        int bad_a = 0, bad_b = 0;
        if (!pair_plan_of(pair_mask, &sf.plan, &bad_a, &bad_b))
            EDMP_REQUIRE(false, "%s: pair_mask[%d][%d] = %d, mask entries are 0 or 1", what, bad_a, bad_b, (int)pair_mask[bad_a * EDMP_N_LINKS + bad_b]);
        sf.self_hits = self_hits_dev;
    }
    const int launch = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int rc = rows_upload(ctx, rows_host, n_rows, &rows_dev)) return rc;
    BlendArgs a;
    a.X = X_dev;
    a.rows = rows_dev;
    a.N = N;
    a.K = substeps;
    a.H = halvings;
    a.reach = reach;
    for (int j = 0; j < 7; ++j) a.vmax[j] = vmax[j], a.amax[j] = amax[j], a.jump[j] = jump[j], a.dev[j] = deviation[j];
    a.obb = g->obb;
    a.kind = g->kind;
    a.beta = beta_dev;
    a.code = code_dev;
    a.halved = halved_dev;
    a.tested = tested_dev;
    if (self && sf.plan.na > 0) {
        hipLaunchKernelGGL((blend_rows_kernel<true, BlendSelf>), dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64), sf);
    } else {  // no self test, or an all-zero mask: today's kernel, no try rejected by the self test
        if (self) EDMP_HIP_CHECK(hipMemsetAsync(self_hits_dev, 0, (size_t)n * N * sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(blend_rows_kernel<false>, dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64));
    }
    return rows_call_end(ctx, rows_dev);
}

extern "C" int edmp_blend_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, const double* vmax,
                                   const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                                   const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_blend_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_blend_rows_dev");
    EDMP_REQUIRE(n >= 1, "edmp_blend_rows_dev: need n >= 1 rows (got %d)", n);
    return blend_rows(ctx, "edmp_blend_rows_dev", false, X_dev, 1, n, N, rows_host, n_rows, vmax, amax, jump, deviation, reach, substeps, halvings, dh_f64,
                      beta_dev, code_dev, halved_dev, tested_dev);
}

// edmp_blend_rows_dev for a bound scene batch: every row against its own scene's obstacles and kinds
extern "C" int edmp_scenes_blend_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows,
                                          const double* vmax, const double* amax, const double* jump, const double* deviation, double reach,
                                          int substeps, int halvings, const double* dh_f64, double* beta_dev, int32_t* code_dev,
                                          int32_t* halved_dev, int32_t* tested_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_blend_rows_dev");
    return blend_rows(ctx, "edmp_scenes_blend_rows_dev", true, X_dev, S, B, N, rows_host, n_rows, vmax, amax, jump, deviation, reach, substeps, halvings,
                      dh_f64, beta_dev, code_dev, halved_dev, tested_dev);
}

// edmp_blend_rows_dev with the self test (pair_mask: 81 host ints, entries above the diagonal read): a try is taken only if it is free of
// the scene AND of itself
extern "C" int edmp_blend_rows_self_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, const double* vmax,
                                        const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                                        const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev,
                                        const int32_t* pair_mask, int32_t* self_hits_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_blend_rows_self_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_blend_rows_self_dev");
    EDMP_REQUIRE(n >= 1, "edmp_blend_rows_self_dev: need n >= 1 rows (got %d)", n);
    return blend_rows(ctx, "edmp_blend_rows_self_dev", false, X_dev, 1, n, N, rows_host, n_rows, vmax, amax, jump, deviation, reach, substeps, halvings, dh_f64,
                      beta_dev, code_dev, halved_dev, tested_dev, pair_mask, self_hits_dev, true);
}

// edmp_blend_rows_self_dev for a bound scene batch: one mask for all scenes
extern "C" int edmp_scenes_blend_rows_self_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows,
                                               const double* vmax, const double* amax, const double* jump, const double* deviation, double reach,
                                               int substeps, int halvings, const double* dh_f64, double* beta_dev, int32_t* code_dev,
                                               int32_t* halved_dev, int32_t* tested_dev, const int32_t* pair_mask, int32_t* self_hits_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_blend_rows_self_dev");
    return blend_rows(ctx, "edmp_scenes_blend_rows_self_dev", true, X_dev, S, B, N, rows_host, n_rows, vmax, amax, jump, deviation, reach, substeps, halvings,
                      dh_f64, beta_dev, code_dev, halved_dev, tested_dev, pair_mask, self_hits_dev, true);
}
