// timing.hip — time parameterisation of finished rows: the stage that turns a geometric polyline into something a controller can follow,
// along the polyline itself (edmp_time_rows_dev, edmp_sample_rows_dev) or along the path with the corner blends that blend.hip chose
// (edmp_time_blended_rows_dev, edmp_sample_blended_rows_dev).
//
// The reference replays its plans at constant velocity in pybullet and ships no timing.  Here every finished row x (7, N) gets the fastest
// rest-to-rest motion ALONG ITS OWN POLYLINE under joint velocity, joint acceleration and corner velocity-jump limits, and that motion is
// sampled at a controller period.  The path is not changed: every sample is x_i + s (x_{i+1} - x_i) with 0 <= s <= 1, so the verdicts of
// the success, self-collision and shortcut stages still describe what is executed.
//
// The rule (include/edmp_hip.h states it in full; tests/timing_inputs.py is its host statement).  Path parameter s in [0, N-1], y = sdot^2:
//   segment i:  d_i = x_{i+1} - x_i;  V_i = min_j vmax_j / |d_ij|,  A_i = min_j amax_j / |d_ij| over the joints with d_ij != 0;
//               d_i = 0: a zero segment - no time, no V / A, y handed across unchanged
//   waypoint i: c_0 = c_{N-1} = 0;  c_i = min(V_{i-1}^2, V_i^2, J_i^2),  J_i = min_j jump_j / |d_ij - d_{i-1,j}|  (absent terms left out)
//   forward:    y_0 = 0,  y_{i+1} = min(c_{i+1}, y_i + 2 A_i)           backward:  y_i = min(y_i, y_{i+1} + 2 A_i)
//   inside a segment: accelerate at A_i, cruise at V_i, decelerate at A_i;  p_i = min(V_i^2, (y_i + y_{i+1}) / 2 + A_i)
// y is the component-wise maximum of {0 <= y_i <= c_i, |y_{i+1} - y_i| <= 2 A_i} (a linear programme reproduces it), so the profile is the
// time optimum on this path, the zero-segment hand-over excepted, which is conservative.
//
// The blended rule (tests/blend_inputs.py is its host statement) is this one with beta (n, N) as blend_rows_kernel (blend.hip) wrote it and
// two changes: the cap of a blended corner is the blend's acceleration cap (2 beta_i) K_i, K_i = min_j amax_j / |d_ij - d_{i-1,j}|, and
// segment i's straight part has the length l_i = (1 - beta_i) - beta_{i+1}.  With beta = 0 everywhere l = 1.0 and (2 A) 1.0 are exact: the
// plain rule's bits.  Each kernel is ONE template over `Blended`, instantiated twice: the plain one reads no beta and forms no l and no K.
//
// time_rows_kernel: ONE wave per row, four rows to a 256-thread workgroup (row = blockIdx.x * 4 + wave, as sdf_goal_kernel deals them);
// lane = waypoint = segment.  Each lane forms d, V, A, c of its own index (d_{i-1} by one shuffle).  The two passes and the time sums are
// serial recurrences of at most 63 steps: a wave-uniform loop reads lane i's operands (v_readlane: i is a loop counter) and every lane
// keeps the value at its own index.  One order of every sum - the host rule's - no LDS, no barrier, no atomics, no divergence inside
// a wave; a wave past the last row leaves by a scalar branch.
//
// sample_rows_kernel: the throughput kernel.  Workgroup = (listed row, chunk of 256 samples), thread = sample.  The row's waypoints and
// profile are staged once in LDS (7 KB, blended 8 KB, whatever M); a thread searches the piece starts - the <= 63 segments, blended the
// 2 N - 3 pieces line 0, blend 1, line 1, ..., line N - 2 - then the <= 3 phases, and evaluates the closed-form quadratic.  Outputs are
// (R, 7, M) with the sample index innermost: each joint's store is coalesced.
#include <cmath>

#include "common.h"
#include "rowlist.h"  // check_limits, check_rows, rows_upload, rows_call_end: shared with shortcut.hip and blend.hip

// every operation of the rule is rounded on its own (the host rule's): no fused multiply-add in this file
#pragma clang fp contract(off)

namespace edmp {

constexpr int kTimedN = 64;         // waypoints per row at most: one wave, lane = waypoint
constexpr int kSampleChunk = 256;   // samples per workgroup

// the kernel arguments, each instantiation's own so that neither carries what it does not read
template <bool Blended> struct TimeArgs;
template <> struct TimeArgs<false> {
    const double* X;  // (n, 7, N)
    int n, N;
    double vmax[7], amax[7], jump[7];
    double* y;         // (n, N)
    double* phase;     // (n, N-1, 3) t_acc | t_cru | t_dec (blended: of the straight part)
    double* times;     // (n, N) waypoint times (blended: (n, N, 2) the time entering | leaving waypoint i's blend)
    double* duration;  // (n,)
    int32_t* limit;    // (n, N)
    double* seg;       // (n, N-1, 2) A_i | p_i: what the sampler needs beside y, phase and times
};
template <> struct TimeArgs<true> {  // the same, with beta (n, N) in and blend (n, N) = the blend times out
    const double *X, *beta;
    int n, N;
    double vmax[7], amax[7], jump[7];
    double *y, *phase, *times, *duration;
    int32_t* limit;
    double *seg, *blend;
};

// lane l's value for the whole wave; l is wave-uniform
__device__ __forceinline__ double lane_value(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

template <bool Blended>
__global__ __launch_bounds__(256) void time_rows_kernel(TimeArgs<Blended> a) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int N = __builtin_amdgcn_readfirstlane(a.N);
    if (r >= a.n) return;  // (r is wave-uniform: the whole wave leaves)
    const double kInf = __builtin_inf();
    const bool wp = lane < N, sg = lane < N - 1;
    const double* xr = a.X + (size_t)r * 7 * N;
    double* yo = a.y + (size_t)r * N;
    double* to = a.times + (size_t)r * N * (Blended ? 2 : 1);
    double* bo = nullptr;
    if constexpr (Blended) bo = a.blend + (size_t)r * N;
    int32_t* lo = a.limit + (size_t)r * N;
    double* po = a.phase + ((size_t)r * (N - 1) + lane) * 3;
    double* so = a.seg + ((size_t)r * (N - 1) + lane) * 2;

    double d[7], dp[7];  // d_i and d_{i-1} of this lane's index
    double b = 0.0;      // beta of this lane's waypoint
    if constexpr (Blended) b = wp ? a.beta[(size_t)r * N + lane] : 0.0;
    bool finite = isfinite(b);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double x0 = wp ? xr[j * N + lane] : 0.0;
        finite = finite && isfinite(x0);
        const double x1 = __shfl_down(x0, 1, 64);
        d[j] = sg ? x1 - x0 : 0.0;
        dp[j] = __shfl_up(d[j], 1, 64);
    }
    if (__ballot(!finite) != 0) {  // (one value for the wave) a row with a non-finite element, of beta too, is not timed
        const double nan = __builtin_nan("");
        if (wp) {
            yo[lane] = nan;
            if constexpr (Blended) {
                to[2 * lane] = to[2 * lane + 1] = nan;
                bo[lane] = nan;
            } else {
                to[lane] = nan;
            }
            lo[lane] = -1;
        }
        if (sg) {
            po[0] = po[1] = po[2] = nan;
            so[0] = so[1] = nan;
        }
        if (lane == 0) a.duration[r] = nan;
        return;
    }
    const double b1 = Blended ? __shfl_down(b, 1, 64) : 0.0;  // (every lane takes part)
    const double ell = Blended && sg ? (1.0 - b) - b1 : 1.0;  // the straight part of segment `lane`

    // segment bounds: a limit over |d_ij| = 0 is +inf and never the minimum, which leaves that joint out; all seven out = a zero segment
    double V = kInf, A = kInf, J = kInf, Kc = kInf;
    bool zero = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double ad = fabs(d[j]), adl = fabs(d[j] - dp[j]);
        const double qv = a.vmax[j] / ad, qa = a.amax[j] / ad, qj = a.jump[j] / adl, qk = Blended ? a.amax[j] / adl : kInf;
        zero = zero && ad == 0.0;
        V = qv < V ? qv : V;
        A = qa < A ? qa : A;
        J = qj < J ? qj : J;
        if constexpr (Blended) Kc = qk < Kc ? qk : Kc;  // the blend's acceleration cap over 2 beta
    }
    const double V2 = V * V;
    const double C2 = Blended && b > 0.0 ? (2.0 * b) * Kc : J * J;  // the corner: the acceleration cap of its blend, or the jump cap
    const double V2p = __shfl_up(V2, 1, 64);
    const bool end = lane == 0 || lane == N - 1;
    double c = V2p;
    c = V2 < c ? V2 : c;
    c = C2 < c ? C2 : c;
    c = end ? 0.0 : c;
    const int zi = zero ? 1 : 0;
    // what a segment can add to y: 2 A_i, doubled where lane i's A_i is read; over a straight part g_i = (2 A_i) l_i, formed by lane i
    const double g = Blended ? (2.0 * A) * ell : A;

    // forward pass: y_{i+1} = min(c_{i+1}, y_i + 2 A_i); lane i + 1 keeps y_{i+1} and the forward candidate
    double y = 0.0, fw = kInf, bw = kInf, run = 0.0;
    for (int i = 0; i < N - 1; ++i) {
        const double gi = lane_value(g, i), c1 = lane_value(c, i + 1);
        const double f = __builtin_amdgcn_readlane(zi, i) ? run : run + (Blended ? gi : 2.0 * gi);
        run = f < c1 ? f : c1;
        if (lane == i + 1) {
            y = run;
            fw = f;
        }
    }
    // backward pass: y_i = min(y_i, y_{i+1} + 2 A_i); lane i keeps y_i and the backward candidate
    run = lane_value(y, N - 1);
    for (int i = N - 2; i >= 0; --i) {
        const double gi = lane_value(g, i), yi = lane_value(y, i);
        const double bb = __builtin_amdgcn_readlane(zi, i) ? run : run + (Blended ? gi : 2.0 * gi);
        run = bb < yi ? bb : yi;
        if (lane == i) {
            y = run;
            bw = bb;
        }
    }
    // the binding constraint: first index of the minimum among rest end | V_{i-1}^2 | V_i^2 | corner | forward | backward
    int code = 0;
    if (!end) {
        double best = V2p;
        code = 1;
        if (V2 < best) best = V2, code = 2;
        if (C2 < best) best = C2, code = 3;
        if (fw < best) best = fw, code = 4;
        if (bw < best) best = bw, code = 5;
    }
    // inside the segment's straight part: accelerate, cruise, decelerate
    const double y1 = __shfl_down(y, 1, 64);
    double p = (y + y1) / 2.0 + (Blended ? A * ell : A);
    p = V2 < p ? V2 : p;
    const double sp = sqrt(p);
    double ta = (sp - sqrt(y)) / A, td = (sp - sqrt(y1)) / A;
    double tc = (ell - (p - y) / (2.0 * A) - (p - y1) / (2.0 * A));
    ta = ta > 0.0 ? ta : 0.0;
    td = td > 0.0 ? td : 0.0;
    tc = (tc > 0.0 ? tc : 0.0) / sp;
    if (zero) ta = tc = td = 0.0, p = y, A = 0.0;
    const double tb = Blended && b > 0.0 ? (2.0 * b) / sqrt(y) : 0.0;  // blend `lane`, crossed at the constant path speed sqrt y
    // times: the phases summed in index order; blended line 0, blend 1, line 1, ... in that order, T = entering and Tout = leaving a blend
    double T = 0.0, Tout = 0.0;
    run = 0.0;
    for (int i = 0; i < N - 1; ++i) {
        run = run + lane_value(ta, i);
        run = run + lane_value(tc, i);
        run = run + lane_value(td, i);
        if (lane == i + 1) T = run;
        if constexpr (Blended) {
            run = run + lane_value(tb, i + 1);
            if (lane == i + 1) Tout = run;
        }
    }
    if (wp) {
        yo[lane] = y;
        if constexpr (Blended) {
            to[2 * lane] = T;
            to[2 * lane + 1] = Tout;
            bo[lane] = tb;
        } else {
            to[lane] = T;
        }
        lo[lane] = code;
    }
    if (sg) {
        po[0] = ta;
        po[1] = tc;
        po[2] = td;
        so[0] = A;
        so[1] = p;
    }
    if (lane == 0) a.duration[r] = run;
}

template <bool Blended> struct SampleArgs;
template <> struct SampleArgs<false> {
    const double *X, *y, *phase, *times, *duration, *seg;
    const int32_t* rows;  // the listed rows, or nullptr = row = slot
    int N, M;
    double period;
    double* q;       // (R, 7, M)
    double* qd;      // (R, 7, M)
    int32_t* count;  // (R,)
};
template <> struct SampleArgs<true> {  // the same, with beta
    const double *X, *beta, *y, *phase, *times, *duration, *seg;
    const int32_t* rows;
    int N, M;
    double period;
    double *q, *qd;
    int32_t* count;
};

// 1 + the smallest k with (double)k * period >= duration, saturated at INT32_MAX; 0 for a row that was not timed
__device__ __forceinline__ int32_t sample_count(double duration, double period) {
    if (!isfinite(duration)) return 0;
    const double g = ceil(duration / period);
    if (!(g < 2147483646.0)) return 2147483647;
    long long k = (long long)g;
    for (int it = 0; it < 4 && k > 0 && (double)(k - 1) * period >= duration; ++it) --k;
    for (int it = 0; it < 4 && (double)k * period < duration; ++it) ++k;
    return (int32_t)(1 + k);
}

template <bool Blended>
__global__ __launch_bounds__(kSampleChunk) void sample_rows_kernel(SampleArgs<Blended> a) {
    constexpr int kT = Blended ? 2 : 1;  // times per waypoint: T_i, blended the time entering | leaving blend i
    __shared__ double s_x[7 * kTimedN], s_T[kT * kTimedN], s_y[kTimedN], s_ph[3 * kTimedN], s_sg[2 * kTimedN];
    double* s_b = nullptr;  // the row's beta: the blended instantiation's own array
    if constexpr (Blended) {
        __shared__ double s_beta[kTimedN];
        s_b = s_beta;
    }
    const int tid = threadIdx.x;
    const int slot = blockIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[slot] : slot);
    const int N = __builtin_amdgcn_readfirstlane(a.N), M = __builtin_amdgcn_readfirstlane(a.M);
    const double* xr = a.X + (size_t)r * 7 * N;
    for (int e = tid; e < 7 * N; e += kSampleChunk) {
        const int j = e / N, m = e - j * N;
        s_x[j * kTimedN + m] = xr[e];
    }
    for (int m = tid; m < N; m += kSampleChunk) {
        s_y[m] = a.y[(size_t)r * N + m];
        if constexpr (Blended) s_b[m] = a.beta[(size_t)r * N + m];
    }
    for (int e = tid; e < kT * N; e += kSampleChunk) s_T[e] = a.times[(size_t)r * N * kT + e];
    for (int e = tid; e < 3 * (N - 1); e += kSampleChunk) s_ph[e] = a.phase[(size_t)r * (N - 1) * 3 + e];
    for (int e = tid; e < 2 * (N - 1); e += kSampleChunk) s_sg[e] = a.seg[(size_t)r * (N - 1) * 2 + e];
    const double dur = a.duration[r];
    __syncthreads();
    if (blockIdx.y == 0 && tid == 0) a.count[slot] = sample_count(dur, a.period);
    const int k = blockIdx.y * kSampleChunk + tid;
    if (k >= M) return;
    const double t = (double)k * a.period;
    const bool timed = isfinite(dur), moving = timed && t < dur;
    // plain: piece p = 0..N-2 is segment p and starts at T_p.  Blended: piece p = 0..2N-4 starts at s_T[p + 1]: p even is the straight part
    // of segment p / 2 (it starts where blend p / 2 is left), p odd is blend (p + 1) / 2 (it starts where that blend is entered)
    const double* start = s_T + (Blended ? 1 : 0);
    int i = N - 2;
    bool on_blend = false;
    double s = 0.0, sd = 0.0, u = 0.0, sy = 0.0, bi = 0.0;
    if (moving) {
        // the largest p with start <= t (the starts are non-decreasing, the first is 0; t < duration makes the next start > t)
        int lo = 0, hi = Blended ? 2 * N - 4 : N - 2;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (start[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const double tau = t - start[lo];
        i = lo;
        if constexpr (Blended) {
            on_blend = (lo & 1) != 0;
            i = (lo + 1) >> 1;  // (lo even: lo / 2)
            bi = s_b[i];
        }
        if (on_blend) {
            sy = sqrt(s_y[i]);
            u = (tau * sy) / (2.0 * bi);
            u = u > 0.0 ? u : 0.0;
            u = u < 1.0 ? u : 1.0;
        } else {
            const double ell = Blended ? (1.0 - bi) - s_b[i + 1] : 1.0;  // the straight part of segment i
            const double ta = s_ph[3 * i], tc = s_ph[3 * i + 1], A = s_sg[2 * i], p = s_sg[2 * i + 1];
            const double yi = s_y[i], y1 = s_y[i + 1], sp = sqrt(p);
            if (tau < ta) {
                const double sq = sqrt(yi);
                sd = sq + A * tau;
                s = sq * tau + (0.5 * A) * (tau * tau);
            } else {
                const double t2 = tau - ta;
                if (t2 < tc) {
                    sd = sp;
                    s = (p - yi) / (2.0 * A) + sp * t2;
                } else {
                    const double t3 = t2 - tc;
                    sd = sp - A * t3;
                    s = (ell - (p - y1) / (2.0 * A)) + (sp * t3 - (0.5 * A) * (t3 * t3));
                }
            }
            sd = sd > 0.0 ? sd : 0.0;
            sd = sd < sp ? sd : sp;
            s = s > 0.0 ? s : 0.0;
            s = s < ell ? s : ell;
            if constexpr (Blended) s = bi + s;  // from waypoint i
        }
    }
    const double nan = __builtin_nan("");
    const size_t o = (size_t)slot * 7 * M + k;
    const double uu = u * u, w = 1.0 - u;
    const double ww = w * w;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double qv, qdv;
        if (!moving) {  // at rest at the goal, its bits; a row that was not timed has no samples
            qv = timed ? s_x[j * kTimedN + N - 1] : nan;
            qdv = timed ? 0.0 : nan;
        } else if (on_blend) {
            const double x0 = s_x[j * kTimedN + i];
            const double dpj = x0 - s_x[j * kTimedN + i - 1], dj = s_x[j * kTimedN + i + 1] - x0;
            qv = x0 + bi * (uu * dj - ww * dpj);
            qdv = sy * (w * dpj + u * dj);
        } else {
            const double xa = s_x[j * kTimedN + i], xb = s_x[j * kTimedN + i + 1];
            const double dj = xb - xa;
            qv = xa + s * dj;
            qdv = dj * sd;
        }
        a.q[o + (size_t)j * M] = qv;
        a.qd[o + (size_t)j * M] = qdv;
    }
}

}  // namespace edmp

using namespace edmp;

// edmp_time_rows_dev and edmp_time_blended_rows_dev (beta_dev and blend_dev: the blended entry's own)
template <bool Blended>
static int time_rows(edmp_ctx* ctx, const char* what, const double* X_dev, int n, int N, const double* beta_dev, const double* vmax, const double* amax,
                     const double* jump, double* y_dev, double* phase_dev, double* times_dev, double* duration_dev, int32_t* limit_dev, double* seg_dev,
                     double* blend_dev) {
    EDMP_REQUIRE(ctx, "%s: null context", what);
    EDMP_REQUIRE(X_dev && (!Blended || (beta_dev && blend_dev)) && y_dev && phase_dev && times_dev && duration_dev && limit_dev && seg_dev,
                 "%s: null pointer", what);
    EDMP_REQUIRE(n >= 1, "%s: need n >= 1 rows (got %d)", what, n);
    EDMP_REQUIRE(N >= 2 && N <= kTimedN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kTimedN, N);
    if (int rc = check_limits(what, "vmax", vmax)) return rc;
    if (int rc = check_limits(what, "amax", amax)) return rc;
    if (int rc = check_limits(what, "jump", jump)) return rc;
    TimeArgs<Blended> a;
    a.X = X_dev;
    a.n = n;
    a.N = N;
    for (int j = 0; j < 7; ++j) a.vmax[j] = vmax[j], a.amax[j] = amax[j], a.jump[j] = jump[j];
    a.y = y_dev;
    a.phase = phase_dev;
    a.times = times_dev;
    a.duration = duration_dev;
    a.limit = limit_dev;
    a.seg = seg_dev;
    if constexpr (Blended) a.beta = beta_dev, a.blend = blend_dev;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(time_rows_kernel<Blended>, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, a);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

extern "C" int edmp_time_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* vmax, const double* amax, const double* jump,
                                  double* y_dev, double* phase_dev, double* times_dev, double* duration_dev, int32_t* limit_dev, double* seg_dev) {
    return time_rows<false>(ctx, "edmp_time_rows_dev", X_dev, n, N, nullptr, vmax, amax, jump, y_dev, phase_dev, times_dev, duration_dev, limit_dev, seg_dev,
                            nullptr);
}

extern "C" int edmp_time_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* vmax,
                                          const double* amax, const double* jump, double* y_dev, double* phase_dev, double* times_dev,
                                          double* duration_dev, int32_t* limit_dev, double* seg_dev, double* blend_dev) {
    return time_rows<true>(ctx, "edmp_time_blended_rows_dev", X_dev, n, N, beta_dev, vmax, amax, jump, y_dev, phase_dev, times_dev, duration_dev, limit_dev,
                           seg_dev, blend_dev);
}

// edmp_sample_rows_dev and edmp_sample_blended_rows_dev (beta_dev: the blended entry's own).  Every refusal comes before any device call
template <bool Blended>
static int sample_rows(edmp_ctx* ctx, const char* what, const double* X_dev, int n, int N, const double* beta_dev, const double* y_dev,
                       const double* phase_dev, const double* times_dev, const double* duration_dev, const double* seg_dev, const int32_t* rows_host,
                       int n_rows, double period, int M, double* q_dev, double* qd_dev, int32_t* count_dev) {
    EDMP_REQUIRE(ctx, "%s: null context", what);
    EDMP_REQUIRE(X_dev && (!Blended || beta_dev) && y_dev && phase_dev && times_dev && duration_dev && seg_dev && q_dev && qd_dev && count_dev,
                 "%s: null pointer", what);
    EDMP_REQUIRE(n >= 1, "%s: need n >= 1 rows (got %d)", what, n);
    EDMP_REQUIRE(N >= 2 && N <= kTimedN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kTimedN, N);
    EDMP_REQUIRE(std::isfinite(period) && period > 0.0, "%s: period %g must be finite and > 0", what, period);
    EDMP_REQUIRE(M >= 1 && M <= EDMP_MAX_TIMED_SAMPLES, "%s: M = %d samples outside 1..%d", what, M, EDMP_MAX_TIMED_SAMPLES);
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;
    const int R = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int rc = rows_upload(ctx, rows_host, n_rows, &rows_dev)) return rc;
    SampleArgs<Blended> a;
    a.X = X_dev;
    if constexpr (Blended) a.beta = beta_dev;
    a.y = y_dev;
    a.phase = phase_dev;
    a.times = times_dev;
    a.duration = duration_dev;
    a.seg = seg_dev;
    a.rows = rows_dev;
    a.N = N;
    a.M = M;
    a.period = period;
    a.q = q_dev;
    a.qd = qd_dev;
    a.count = count_dev;
    hipLaunchKernelGGL(sample_rows_kernel<Blended>, dim3(R, (M + kSampleChunk - 1) / kSampleChunk), dim3(kSampleChunk), 0, ctx->stream, a);
    return rows_call_end(ctx, rows_dev);
}

extern "C" int edmp_sample_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* y_dev, const double* phase_dev,
                                    const double* times_dev, const double* duration_dev, const double* seg_dev, const int32_t* rows_host, int n_rows,
                                    double period, int M, double* q_dev, double* qd_dev, int32_t* count_dev) {
    return sample_rows<false>(ctx, "edmp_sample_rows_dev", X_dev, n, N, nullptr, y_dev, phase_dev, times_dev, duration_dev, seg_dev, rows_host, n_rows, period,
                              M, q_dev, qd_dev, count_dev);
}

extern "C" int edmp_sample_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* y_dev,
                                            const double* phase_dev, const double* times_dev, const double* duration_dev, const double* seg_dev,
                                            const int32_t* rows_host, int n_rows, double period, int M, double* q_dev, double* qd_dev,
                                            int32_t* count_dev) {
    return sample_rows<true>(ctx, "edmp_sample_blended_rows_dev", X_dev, n, N, beta_dev, y_dev, phase_dev, times_dev, duration_dev, seg_dev, rows_host, n_rows,
                             period, M, q_dev, qd_dev, count_dev);
}
