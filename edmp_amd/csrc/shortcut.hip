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

__global__ __launch_bounds__(256) void shortcut_rows_kernel(ShortcutArgs a, SceneSlices sl, Robot64 rc) {
    __shared__ double s_x[7 * kShortcutN];  // the row
    __shared__ double s_y[7 * kShortcutN];  // the piece of the candidate, at the columns it would take
    __shared__ double s_len[kShortcutN];    // s_len[m] = |x_{m+1} - x_m|
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ int s_ci, s_cj, s_hit, s_bad;
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
        }
        return;
    }
    for (int m = tid; m < N - 1; m += 256) s_len[m] = shortcut_distance(s_x, m, m + 1);
    __syncthreads();
    // thread 0's own: where the walk stands and what it has counted
    int span = N - 1, i = 0, pass = 0, pass_accepted = 0, accepted = 0, tested = 0;
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
        __syncthreads();
        const int hit = __builtin_amdgcn_readfirstlane(s_hit);
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
    }
}

}  // namespace edmp

using namespace edmp;

// edmp_shortcut_rows_dev and edmp_scenes_shortcut_rows_dev behind their own state checks: n = S x rps rows of the state X (n, 7, N).
// Every refusal comes before any device call.  The row list goes into a block of the call's own (rowlist.h).
static int shortcut_rows(edmp_ctx* ctx, const char* what, bool batch, double* X_dev, int S, int rps, int N, const int32_t* rows_host, int n_rows,
                         int substeps, int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                         int32_t* spans_dev, int log_cap) {
    Guide* g = ctx->guide;
    const int n = S * rps;
    EDMP_REQUIRE(X_dev && accepted_dev && tested_dev && length_dev, "%s: null pointer", what);
    EDMP_REQUIRE(N >= 3 && N <= kShortcutN, "%s: need 3 <= N <= %d waypoints per row (got %d)", what, kShortcutN, N);
    EDMP_REQUIRE(substeps >= 1 && substeps <= 64, "%s: substeps %d outside 1..64", what, substeps);
    EDMP_REQUIRE(passes >= 0 && passes <= EDMP_MAX_SHORTCUT_PASSES, "%s: passes %d outside 0..%d", what, passes, EDMP_MAX_SHORTCUT_PASSES);
    EDMP_REQUIRE(std::isfinite(min_gain) && min_gain >= 0.0, "%s: min_gain %g must be finite and >= 0", what, min_gain);
    EDMP_REQUIRE(log_cap >= 0 && (log_cap == 0 || spans_dev), "%s: log_cap %d needs log_cap >= 0 and a span log of that many entries per row", what, log_cap);
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;
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
    hipLaunchKernelGGL(shortcut_rows_kernel, dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64));
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
