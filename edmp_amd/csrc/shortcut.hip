// shortcut.hip — path shortcutting of finished rows under the exact collision check: the stage between repair and selection.
//
// The reference ships no shortcutting (its evaluator, mpinets/metrics.py, scores the path length and smoothness that this stage improves).
// A shortcut replaces the waypoints strictly between i and j by points of the joint-space chord x_i -> x_j.  It is accepted only if the
// success check's own test (linkbox.h: configuration_hits, nine f64 link boxes against the scene's boxes and cylinders, touching counts)
// finds no hit at EVERY configuration the success check will later test on the new piece: the new waypoints and the K - 1 interpolants of
// every segment of the piece, formed by the same expression (interp_joint).  So a row that passes success_rows before passes it after.
//
// The rule (include/edmp_hip.h states it in full; tests/shortcut_inputs.py is its host statement):
//   spans s = N - 1, then (s + 1) / 2 while s > 2, ending with s = 2;  per pass, per span: i = 0; while i + s <= N - 1: j = i + s,
//   gain = sum_{m = i}^{j - 1} |x_{m+1} - x_m| - |x_j - x_i| (index order); not gain > min_gain: ++i, nothing tested; else the piece
//   y_m = x_i + (m - i) / (j - i) (x_j - x_i) is tested: no hit: x_m <- y_m, i = j; hit: ++i.  A pass that accepts nothing ends the row.
//
// Design: one 256-thread workgroup per listed row for the whole run of the row.  The row, its segment lengths, the piece and the scene's
// obstacles live in LDS (a fixed 15.8 KB: nothing depends on N, K or passes).  Thread 0 walks the candidates whose gain is too small - a
// few adds each - and publishes the next candidate to test, or the end of the row, as ONE LDS value; all 256 threads read it behind a
// barrier, write the piece, test its configurations (thread = configuration, strided: 503 at N = 64, K = 8) and read the one hit flag
// behind the next barrier.  No per-wave or per-lane condition leaves the candidate loop.  All f64, no atomics, rows are independent.
//
// SELF (the *_self_dev entry points with a non-zero pair mask): a candidate must also leave the arm free of itself at the same
// configurations - linkbox.h: configuration_self_hit, the work item of self_collision_rows_kernel, on the bits self_collision_rows will
// form on the output (interp_joint).  So a row that self_collision_rows (same substeps, same mask) calls free before is free after.  The
// test loop's items become (configuration, test), test-major: first the M = sp K - 1 obstacle items, padded to a multiple of 64 so that
// a wave runs one kind of test, then the na M self items, lower link after lower link - they fill the threads a small span leaves idle.
// Two LDS flags per candidate: an obstacle item is skipped only when the obstacle flag is up, a self item when either is up; the
// candidate is rejected if either is up and counts as rejected by the self test alone iff the obstacle flag is down and the self flag
// up - both of which depend on the inputs only, not on which thread came first.  SELF = false is the kernel as it was.
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"  // Robot64, SceneSlices, configuration_hits, interp_joint: shared with success.hip
#include "rowlist.h"  // check_rows, rows_upload, rows_call_end: shared with timing.hip and blend.hip

// the gain and the piece are stated as separately rounded f64 operations (the host rule's): no fused multiply-add in this file's own code
#pragma clang fp contract(off)

namespace edmp {

constexpr int kShortcutN = 64;  // waypoints per row at most: the LDS row stride

struct ShortcutArgs {
    double* X;             // (n, 7, N), in place
    const int32_t* rows;   // the listed rows, or nullptr = row = workgroup
    int N, K, passes, log_cap;
    double min_gain;
    const double* obb;     // the guide's obstacle table and kinds
    const int32_t* kind;
    int32_t* accepted;     // (n,)
    int32_t* tested;       // (n,)
    double* length;        // (n, 2) before | after
    int32_t* spans;        // (n, log_cap, 2)
};

// |x_b - x_a| over the seven joints of the LDS row x (stride kShortcutN), squares summed in joint order
__device__ __forceinline__ double shortcut_distance(const double* x, int a, int b) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double d = x[j * kShortcutN + b] - x[j * kShortcutN + a];
        s = s + d * d;
    }
    return sqrt(s);
}

// what the SELF kernel takes beside today's arguments: the one element of its argument pack (the SELF = false kernel's pack is empty - it
// is launched with today's arguments, and nothing else)
struct ShortcutSelf {
    PairPlan plan;
    int32_t* self_rejected;  // (n,)
};

template <bool SELF, class... Self>
__global__ __launch_bounds__(256) void shortcut_rows_kernel(ShortcutArgs a, SceneSlices sl, Robot64 rc, Self... self_pack) {
    static_assert(sizeof...(Self) == (SELF ? 1 : 0), "the SELF kernel takes ONE more argument, the plain kernel none");
    const auto& sf = self_arguments(self_pack...);  // (ShortcutSelf, or nothing to read)
    __shared__ double s_x[7 * kShortcutN];  // the row
    __shared__ double s_y[7 * kShortcutN];  // the piece of the candidate, at the columns it would take
    __shared__ double s_len[kShortcutN];    // s_len[m] = |x_{m+1} - x_m|
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ int s_ci, s_cj, s_hit, s_bad;
    __shared__ int s_self, s_pa[EDMP_N_LINKS - 1], s_pbits[EDMP_N_LINKS - 1], s_pjlast[EDMP_N_LINKS - 1];  // (SELF only: unused ones take no LDS)
    const int tid = threadIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[blockIdx.x] : (int)blockIdx.x);
    const int scene = __builtin_amdgcn_readfirstlane(r / sl.rps);  // (one row, one scene: workgroup-uniform)
    const int N = __builtin_amdgcn_readfirstlane(a.N), K = __builtin_amdgcn_readfirstlane(a.K), passes = __builtin_amdgcn_readfirstlane(a.passes);
    const int no = min(sl.cnt[scene], EDMP_MAX_OBSTACLES);
    const double* obb = a.obb + (size_t)sl.off[scene] * 16;
    const int32_t* kind = a.kind + sl.off[scene];
    double* xr = a.X + (size_t)r * 7 * N;
    int32_t* log = a.spans + (size_t)r * a.log_cap * 2;
    if (tid == 0) s_bad = 0;
    int na = 0;
    if constexpr (SELF) {
        na = __builtin_amdgcn_readfirstlane(sf.plan.na);
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
        s_x[j * kShortcutN + m] = v;
        if (!isfinite(v)) s_bad = 1;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_bad)) {  // (one LDS value behind a barrier: the whole workgroup leaves) the row is not touched
        for (int e = tid; e < 2 * a.log_cap; e += 256) log[e] = -1;
        if (tid == 0) {
            a.accepted[r] = -1;
            a.tested[r] = 0;
            a.length[2 * r] = a.length[2 * r + 1] = __builtin_nan("");
            if constexpr (SELF) sf.self_rejected[r] = 0;
        }
        return;
    }
    for (int m = tid; m < N - 1; m += 256) s_len[m] = shortcut_distance(s_x, m, m + 1);
    __syncthreads();
    // thread 0's own: where the walk stands and what it has counted
    int span = N - 1, i = 0, pass = 0, pass_accepted = 0, accepted = 0, tested = 0, self_rejected = 0;
    bool over = passes == 0;
    if (tid == 0) {
        double len = 0.0;
        for (int m = 0; m < N - 1; ++m) len = len + s_len[m];
        a.length[2 * r] = len;
    }
    for (;;) {
        if (tid == 0) {  // walk to the next candidate whose gain asks for a test
            int ci = -1, cj = -1;
            while (!over) {
                if (i + span > N - 1) {  // this span is through
                    if (span > 2) {
                        span = (span + 1) >> 1;
                        i = 0;
                        continue;
                    }
                    ++pass;  // the pass is through; one that accepted nothing ends the row: a further pass would repeat it
                    if (pass_accepted == 0 || pass >= passes) {
                        over = true;
                        break;
                    }
                    pass_accepted = 0;
                    span = N - 1;
                    i = 0;
                    continue;
                }
                const int j = i + span;
                double sum = 0.0;
                for (int m = i; m < j; ++m) sum = sum + s_len[m];
                const double gain = sum - shortcut_distance(s_x, i, j);
                if (gain > a.min_gain) {
                    ci = i;
                    cj = j;
                    break;
                }
                ++i;
            }
            s_ci = ci;
            s_cj = cj;
            s_hit = 0;
            if constexpr (SELF) s_self = 0;
        }
        __syncthreads();
        const int ci = __builtin_amdgcn_readfirstlane(s_ci), cj = __builtin_amdgcn_readfirstlane(s_cj);
        if (ci < 0) break;  // the same value for all 256 threads: the row has ended
        const int sp = cj - ci;
        for (int e = tid; e < 7 * (sp + 1); e += 256) {  // the piece, its ends being x_i and x_j themselves
            const int j = e / (sp + 1), m = e - j * (sp + 1);
            const double xi = s_x[j * kShortcutN + ci], xj = s_x[j * kShortcutN + cj];
            const double g = (double)m / (double)sp;
            s_y[j * kShortcutN + ci + m] = m == 0 ? xi : m == sp ? xj : xi + g * (xj - xi);
        }
        __syncthreads();
        // configuration c = m K + k of the piece, as the success check numbers them; 0 and sp K are the waypoints i and j themselves
        for (int c = 1 + tid; c < sp * K; c += 256) {
            if (*(volatile int*)&s_hit) continue;  // somebody has hit already: less work, the same result
            const int m = c / K, k = c - m * K;
            const double f = (double)k / (double)K;
            const double* ya = s_y + ci + m;
            const bool hit = configuration_hits<false>(
                [&](int j) {
                    const double y0 = ya[j * kShortcutN];
                    return k == 0 ? y0 : interp_joint(y0, ya[j * kShortcutN + 1], f);
                },
                rc, s_ob, s_kind, no);
            if (hit) s_hit = 1;
        }
        if constexpr (SELF) {
            // the self items behind the obstacle items: item = (lower link of the plan, configuration), link-major
            // item w of the whole list runs on thread w % 256: self item s = w - Mp starts on the wave behind the obstacle items' last one
            const int M = sp * K - 1, Mp = (M + 63) & ~63;
            for (int w = Mp + ((tid - Mp) & 255); w < Mp + na * M; w += 256) {
                if (*(volatile int*)&s_hit || *(volatile int*)&s_self) continue;  // rejected already: less work, the same result
                const int it = (w - Mp) / M, c = 1 + (w - Mp) - it * M;
                const int m = c / K, k = c - m * K;
                const double f = (double)k / (double)K;
                const double* ya = s_y + ci + m;
                const int b = configuration_self_hit(
                    [&](int j) {
                        const double y0 = ya[j * kShortcutN];
                        return k == 0 ? y0 : interp_joint(y0, ya[j * kShortcutN + 1], f);
                    },
                    rc, s_pa[it], s_pbits[it], s_pjlast[it]);
                if (b >= 0) s_self = 1;
            }
        }
        __syncthreads();
        const int obstacle_hit = __builtin_amdgcn_readfirstlane(s_hit);
        int hit = obstacle_hit;
        if constexpr (SELF) hit |= __builtin_amdgcn_readfirstlane(s_self);
        if (!hit) {  // accept (one LDS value behind a barrier: all 256 threads take the same side)
            for (int e = tid; e < 7 * (sp - 1); e += 256) {
                const int j = e / (sp - 1), m = ci + 1 + (e - j * (sp - 1));
                s_x[j * kShortcutN + m] = s_y[j * kShortcutN + m];
            }
            __syncthreads();
            for (int m = tid; m < sp; m += 256) s_len[ci + m] = shortcut_distance(s_x, ci + m, ci + m + 1);
        }
        if (tid == 0) {
            ++tested;
            if (SELF && hit && !obstacle_hit) ++self_rejected;  // the obstacle test passed it, the self test alone rejected it
            if (!hit) {
                if (accepted < a.log_cap) {
                    log[2 * accepted] = ci;
                    log[2 * accepted + 1] = cj;
                }
                ++accepted;
                ++pass_accepted;
                i = cj;
            } else {
                ++i;
            }
        }
        __syncthreads();  // the new row and lengths before thread 0 walks on; s_ci / s_hit read by all before they are written again
    }
    if (tid == 0) s_hit = accepted;  // (nobody reads s_hit between the walk's last barrier and the next one)
    __syncthreads();
    const int n_acc = __builtin_amdgcn_readfirstlane(s_hit);
    for (int e = 2 * min(n_acc, a.log_cap) + tid; e < 2 * a.log_cap; e += 256) log[e] = -1;
    if (n_acc > 0)  // columns 0 and N - 1 are never written
        for (int e = tid; e < 7 * (N - 2); e += 256) {
            const int j = e / (N - 2), m = 1 + (e - j * (N - 2));
            xr[j * N + m] = s_x[j * kShortcutN + m];
        }
    if (tid == 0) {
        double len = 0.0;
        for (int m = 0; m < N - 1; ++m) len = len + s_len[m];
        a.length[2 * r + 1] = len;
        a.accepted[r] = accepted;
        a.tested[r] = tested;
        if constexpr (SELF) sf.self_rejected[r] = self_rejected;
    }
}

}  // namespace edmp

using namespace edmp;

// edmp_shortcut_rows_dev and edmp_scenes_shortcut_rows_dev behind their own state checks: n = S x rps rows of the state X (n, 7, N).
// Every refusal comes before any device call.  The row list goes into a block of the call's own (rowlist.h).  pair_mask non-NULL: the
// *_self_dev entry points - the SELF kernel with the mask's plan, or, for an all-zero mask, today's kernel and a zero-filled self_rejected.
static int shortcut_rows(edmp_ctx* ctx, const char* what, bool batch, double* X_dev, int S, int rps, int N, const int32_t* rows_host, int n_rows,
                         int substeps, int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                         int32_t* spans_dev, int log_cap, const int32_t* pair_mask = nullptr, int32_t* self_rejected_dev = nullptr,
                         bool self = false) {
    Guide* g = ctx->guide;
    const int n = S * rps;
    EDMP_REQUIRE(X_dev && accepted_dev && tested_dev && length_dev, "%s: null pointer", what);
    EDMP_REQUIRE(N >= 3 && N <= kShortcutN, "%s: need 3 <= N <= %d waypoints per row (got %d)", what, kShortcutN, N);
    EDMP_REQUIRE(substeps >= 1 && substeps <= 64, "%s: substeps %d outside 1..64", what, substeps);
    EDMP_REQUIRE(passes >= 0 && passes <= EDMP_MAX_SHORTCUT_PASSES, "%s: passes %d outside 0..%d", what, passes, EDMP_MAX_SHORTCUT_PASSES);
    EDMP_REQUIRE(std::isfinite(min_gain) && min_gain >= 0.0, "%s: min_gain %g must be finite and >= 0", what, min_gain);
    EDMP_REQUIRE(log_cap >= 0 && (log_cap == 0 || spans_dev), "%s: log_cap %d needs log_cap >= 0 and a span log of that many entries per row", what, log_cap);
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;
    ShortcutSelf sf = {};
    if (self) {
        EDMP_REQUIRE(pair_mask && self_rejected_dev, "%s: pair_mask and self_rejected_dev must not be NULL", what);
        int bad_a = 0, bad_b = 0;
        if (!pair_plan_of(pair_mask, &sf.plan, &bad_a, &bad_b))
            EDMP_REQUIRE(false, "%s: pair_mask[%d][%d] = %d, mask entries are 0 or 1", what, bad_a, bad_b, (int)pair_mask[bad_a * EDMP_N_LINKS + bad_b]);
        sf.self_rejected = self_rejected_dev;
    }
    const int launch = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int rc = rows_upload(ctx, rows_host, n_rows, &rows_dev)) return rc;
    ShortcutArgs a;
    a.X = X_dev;
    a.rows = rows_dev;
    a.N = N;
    a.K = substeps;
    a.passes = passes;
    a.log_cap = log_cap;
    a.min_gain = min_gain;
    a.obb = g->obb;
    a.kind = g->kind;
    a.accepted = accepted_dev;
    a.tested = tested_dev;
    a.length = length_dev;
    a.spans = spans_dev;
    if (self && sf.plan.na > 0) {
        hipLaunchKernelGGL((shortcut_rows_kernel<true, ShortcutSelf>), dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64), sf);
    } else {  // no self test, or an all-zero mask: today's kernel, nothing rejected by the self test
        if (self) EDMP_HIP_CHECK(hipMemsetAsync(self_rejected_dev, 0, (size_t)n * sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(shortcut_rows_kernel<false>, dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64));
    }
    return rows_call_end(ctx, rows_dev);
}

extern "C" int edmp_shortcut_rows_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int substeps, int passes,
                                      double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                                      int32_t* spans_dev, int log_cap) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_shortcut_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_shortcut_rows_dev");
    EDMP_REQUIRE(n >= 1, "edmp_shortcut_rows_dev: need n >= 1 rows (got %d)", n);
    return shortcut_rows(ctx, "edmp_shortcut_rows_dev", false, X_dev, 1, n, N, rows_host, n_rows, substeps, passes, min_gain, dh_f64, accepted_dev, tested_dev,
                         length_dev, spans_dev, log_cap);
}

// edmp_shortcut_rows_dev for a bound scene batch: every row against its own scene's obstacles and kinds
extern "C" int edmp_scenes_shortcut_rows_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int substeps,
                                             int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev,
                                             double* length_dev, int32_t* spans_dev, int log_cap) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_shortcut_rows_dev");
    return shortcut_rows(ctx, "edmp_scenes_shortcut_rows_dev", true, X_dev, S, B, N, rows_host, n_rows, substeps, passes, min_gain, dh_f64, accepted_dev,
                         tested_dev, length_dev, spans_dev, log_cap);
}

// edmp_shortcut_rows_dev with the self test (pair_mask: 81 host ints, entries above the diagonal read): a candidate is taken only if it is
// free of the scene AND of itself
extern "C" int edmp_shortcut_rows_self_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int substeps, int passes,
                                           double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                                           int32_t* spans_dev, int log_cap, const int32_t* pair_mask, int32_t* self_rejected_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_shortcut_rows_self_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_shortcut_rows_self_dev");
    EDMP_REQUIRE(n >= 1, "edmp_shortcut_rows_self_dev: need n >= 1 rows (got %d)", n);
    return shortcut_rows(ctx, "edmp_shortcut_rows_self_dev", false, X_dev, 1, n, N, rows_host, n_rows, substeps, passes, min_gain, dh_f64, accepted_dev,
                         tested_dev, length_dev, spans_dev, log_cap, pair_mask, self_rejected_dev, true);
}

// edmp_shortcut_rows_self_dev for a bound scene batch: one mask for all scenes
extern "C" int edmp_scenes_shortcut_rows_self_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int substeps,
                                                  int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev,
                                                  double* length_dev, int32_t* spans_dev, int log_cap, const int32_t* pair_mask,
                                                  int32_t* self_rejected_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_shortcut_rows_self_dev");
    return shortcut_rows(ctx, "edmp_scenes_shortcut_rows_self_dev", true, X_dev, S, B, N, rows_host, n_rows, substeps, passes, min_gain, dh_f64, accepted_dev,
                         tested_dev, length_dev, spans_dev, log_cap, pair_mask, self_rejected_dev, true);
}
