// blend.hip — parabolic corner blends of finished rows under the exact collision check, and the timing and sampling of the blended path:
// the stage after time_rows / sample_rows (timing.hip), for motions that may leave the polyline by a bounded amount.
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
// rows are independent.  An accepted blend was tested at exactly the configurations q(k / K_b), k = 0..K_b, the two ends included;
// self-collision is NOT tested.
//
// time_blended_rows_kernel is time_rows_kernel's layout - one wave per row, lane = waypoint, the passes and sums as wave-uniform loops -
// with the rule's two changes: the corner cap of a blended corner is the blend's acceleration cap (2 beta_i) K_i, and segment i's straight
// part has the length l_i = (1 - beta_i) - beta_{i+1}.  With beta = 0 everywhere l = 1.0 and (2 A) 1.0 are exact: time_rows' bits.
//
// sample_blended_rows_kernel is sample_rows_kernel's layout - workgroup = (listed row, 256 samples), the profile staged in LDS,
// coalesced stores - over the 2 N - 3 pieces line 0, blend 1, line 1, ..., line N - 2.
#include <cmath>

#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"  // Robot64, SceneSlices, configuration_hits: shared with success.hip and shortcut.hip

// every operation of the rule is rounded on its own (the host rule's): no fused multiply-add in this file's own code
#pragma clang fp contract(off)

namespace edmp {

constexpr int kBlendN = 64;             // waypoints per row at most: one wave in the timing kernel, the LDS row stride elsewhere
constexpr int kBlendChunk = 256;        // samples per workgroup
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

__global__ __launch_bounds__(256) void blend_rows_kernel(BlendArgs a, SceneSlices sl, Robot64 rc) {
    __shared__ double s_x[7 * kBlendN];  // the row
    __shared__ double s_beta[kBlendN];   // the beta under test of each corner
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ double s_b0[kBlendN], s_K[kBlendN], s_J2[kBlendN], s_out[kBlendN];  // per corner: beta0, K, J^2 and the beta that was kept
    __shared__ int s_try[kBlendN], s_hit[kBlendN], s_cnt[kBlendN], s_code[kBlendN], s_halved[kBlendN];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[blockIdx.x] : (int)blockIdx.x);
    const int scene = __builtin_amdgcn_readfirstlane(r / sl.rps);  // (one row, one scene: workgroup-uniform)
    const int N = __builtin_amdgcn_readfirstlane(a.N), K = __builtin_amdgcn_readfirstlane(a.K), H = __builtin_amdgcn_readfirstlane(a.H);
    const int no = min(sl.cnt[scene], EDMP_MAX_OBSTACLES);
    const double* obb = a.obb + (size_t)sl.off[scene] * 16;
    const int32_t* kind = a.kind + sl.off[scene];
    const double* xr = a.X + (size_t)r * 7 * N;
    if (tid == 0) s_bad = 0;
    if (tid < kBlendN) s_try[tid] = s_hit[tid] = s_cnt[tid] = 0;
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
        __syncthreads();
        if (mytry) {  // (corner tid's entries are touched by its owner alone from here to the next barrier)
            s_cnt[tid] += K + 1;
            if (!s_hit[tid]) {
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
    }
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int m = 1; m < N - 1; ++m) total += s_cnt[m];
        a.tested[r] = total;
    }
}

struct TimeBlendedArgs {
    const double* X;     // (n, 7, N)
    const double* beta;  // (n, N)
    int n, N;
    double vmax[7], amax[7], jump[7];
    double* y;         // (n, N)
    double* phase;     // (n, N-1, 3) t_acc | t_cru | t_dec of the straight part
    double* times;     // (n, N, 2) the time entering | leaving waypoint i's blend
    double* duration;  // (n,)
    int32_t* limit;    // (n, N)
    double* seg;       // (n, N-1, 2) A_i | p_i
    double* blend;     // (n, N) blend times
};

// lane l's value for the whole wave; l is wave-uniform
__device__ __forceinline__ double blend_lane_value(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void time_blended_rows_kernel(TimeBlendedArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int N = __builtin_amdgcn_readfirstlane(a.N);
    if (r >= a.n) return;  // (r is wave-uniform: the whole wave leaves)
    const double kInf = __builtin_inf();
    const bool wp = lane < N, sg = lane < N - 1;
    const double* xr = a.X + (size_t)r * 7 * N;
    double* yo = a.y + (size_t)r * N;
    double* to = a.times + (size_t)r * N * 2;
    double* bo = a.blend + (size_t)r * N;
    int32_t* lo = a.limit + (size_t)r * N;
    double* po = a.phase + ((size_t)r * (N - 1) + lane) * 3;
    double* so = a.seg + ((size_t)r * (N - 1) + lane) * 2;

    double d[7], dp[7];  // d_i and d_{i-1} of this lane's index
    const double b = wp ? a.beta[(size_t)r * N + lane] : 0.0;
    bool finite = isfinite(b);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double x0 = wp ? xr[j * N + lane] : 0.0;
        finite = finite && isfinite(x0);
        const double x1 = __shfl_down(x0, 1, 64);
        d[j] = sg ? x1 - x0 : 0.0;
        dp[j] = __shfl_up(d[j], 1, 64);
    }
    if (__ballot(!finite) != 0) {  // (one value for the wave) a row with a non-finite element, or a non-finite beta, is not timed
        const double nan = __builtin_nan("");
        if (wp) {
            yo[lane] = nan;
            to[2 * lane] = to[2 * lane + 1] = nan;
            bo[lane] = nan;
            lo[lane] = -1;
        }
        if (sg) {
            po[0] = po[1] = po[2] = nan;
            so[0] = so[1] = nan;
        }
        if (lane == 0) a.duration[r] = nan;
        return;
    }
    const double b1 = __shfl_down(b, 1, 64);
    const double ell = sg ? (1.0 - b) - b1 : 1.0;  // the straight part of segment `lane`

    double V = kInf, A = kInf, J = kInf, Kc = kInf;
    bool zero = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double ad = fabs(d[j]), adl = fabs(d[j] - dp[j]);
        const double qv = a.vmax[j] / ad, qa = a.amax[j] / ad, qj = a.jump[j] / adl, qk = a.amax[j] / adl;
        zero = zero && ad == 0.0;
        V = qv < V ? qv : V;
        A = qa < A ? qa : A;
        J = qj < J ? qj : J;
        Kc = qk < Kc ? qk : Kc;
    }
    const double V2 = V * V;
    const double C2 = b > 0.0 ? (2.0 * b) * Kc : J * J;  // the corner: blend acceleration cap, or jump cap
    const double V2p = __shfl_up(V2, 1, 64);
    const bool end = lane == 0 || lane == N - 1;
    double c = V2p;
    c = V2 < c ? V2 : c;
    c = C2 < c ? C2 : c;
    c = end ? 0.0 : c;
    const int zi = zero ? 1 : 0;
    const double g = (2.0 * A) * ell;  // what the straight part can add to y

    // forward pass: y_{i+1} = min(c_{i+1}, y_i + (2 A_i) l_i); lane i + 1 keeps y_{i+1} and the forward candidate
    double y = 0.0, fw = kInf, bw = kInf, run = 0.0;
    for (int i = 0; i < N - 1; ++i) {
        const double gi = blend_lane_value(g, i), c1 = blend_lane_value(c, i + 1);
        const double f = __builtin_amdgcn_readlane(zi, i) ? run : run + gi;
        run = f < c1 ? f : c1;
        if (lane == i + 1) {
            y = run;
            fw = f;
        }
    }
    // backward pass: y_i = min(y_i, y_{i+1} + (2 A_i) l_i); lane i keeps y_i and the backward candidate
    run = blend_lane_value(y, N - 1);
    for (int i = N - 2; i >= 0; --i) {
        const double gi = blend_lane_value(g, i), yi = blend_lane_value(y, i);
        const double bb = __builtin_amdgcn_readlane(zi, i) ? run : run + gi;
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
    // inside the straight part: accelerate, cruise, decelerate
    const double y1 = __shfl_down(y, 1, 64);
    double p = (y + y1) / 2.0 + A * ell;
    p = V2 < p ? V2 : p;
    const double sp = sqrt(p);
    double ta = (sp - sqrt(y)) / A, td = (sp - sqrt(y1)) / A;
    double tc = (ell - (p - y) / (2.0 * A) - (p - y1) / (2.0 * A));
    ta = ta > 0.0 ? ta : 0.0;
    td = td > 0.0 ? td : 0.0;
    tc = (tc > 0.0 ? tc : 0.0) / sp;
    if (zero) ta = tc = td = 0.0, p = y, A = 0.0;
    const double tb = b > 0.0 ? (2.0 * b) / sqrt(y) : 0.0;  // blend `lane`, crossed at the constant path speed sqrt y
    // times: line 0, blend 1, line 1, ... summed in that order
    double Tin = 0.0, Tout = 0.0;
    run = 0.0;
    for (int i = 0; i < N - 1; ++i) {
        run = run + blend_lane_value(ta, i);
        run = run + blend_lane_value(tc, i);
        run = run + blend_lane_value(td, i);
        if (lane == i + 1) Tin = run;
        run = run + blend_lane_value(tb, i + 1);
        if (lane == i + 1) Tout = run;
    }
    if (wp) {
        yo[lane] = y;
        to[2 * lane] = Tin;
        to[2 * lane + 1] = Tout;
        bo[lane] = tb;
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

struct SampleBlendedArgs {
    const double *X, *beta, *y, *phase, *times, *duration, *seg;
    const int32_t* rows;  // the listed rows, or nullptr = row = slot
    int N, M;
    double period;
    double* q;       // (R, 7, M)
    double* qd;      // (R, 7, M)
    int32_t* count;  // (R,)
};

// 1 + the smallest k with (double)k * period >= duration, saturated at INT32_MAX; 0 for a row that was not timed (sample_rows' count)
__device__ __forceinline__ int32_t blended_sample_count(double duration, double period) {
    if (!isfinite(duration)) return 0;
    const double g = ceil(duration / period);
    if (!(g < 2147483646.0)) return 2147483647;
    long long k = (long long)g;
    for (int it = 0; it < 4 && k > 0 && (double)(k - 1) * period >= duration; ++it) --k;
    for (int it = 0; it < 4 && (double)k * period < duration; ++it) ++k;
    return (int32_t)(1 + k);
}

__global__ __launch_bounds__(kBlendChunk) void sample_blended_rows_kernel(SampleBlendedArgs a) {
    __shared__ double s_x[7 * kBlendN], s_T[2 * kBlendN], s_y[kBlendN], s_b[kBlendN], s_ph[3 * kBlendN], s_sg[2 * kBlendN];
    const int tid = threadIdx.x;
    const int slot = blockIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[slot] : slot);
    const int N = __builtin_amdgcn_readfirstlane(a.N), M = __builtin_amdgcn_readfirstlane(a.M);
    const double* xr = a.X + (size_t)r * 7 * N;
    for (int e = tid; e < 7 * N; e += kBlendChunk) {
        const int j = e / N, m = e - j * N;
        s_x[j * kBlendN + m] = xr[e];
    }
    for (int m = tid; m < N; m += kBlendChunk) {
        s_y[m] = a.y[(size_t)r * N + m];
        s_b[m] = a.beta[(size_t)r * N + m];
    }
    for (int e = tid; e < 2 * N; e += kBlendChunk) s_T[e] = a.times[(size_t)r * N * 2 + e];
    for (int e = tid; e < 3 * (N - 1); e += kBlendChunk) s_ph[e] = a.phase[(size_t)r * (N - 1) * 3 + e];
    for (int e = tid; e < 2 * (N - 1); e += kBlendChunk) s_sg[e] = a.seg[(size_t)r * (N - 1) * 2 + e];
    const double dur = a.duration[r];
    __syncthreads();
    if (blockIdx.y == 0 && tid == 0) a.count[slot] = blended_sample_count(dur, a.period);
    const int k = blockIdx.y * kBlendChunk + tid;
    if (k >= M) return;
    const double t = (double)k * a.period;
    const bool timed = isfinite(dur), moving = timed && t < dur;
    // piece p = 0..2N-4 starts at s_T[p + 1]: p even is the straight part of segment p / 2 (it starts where blend p / 2 is left), p odd is
    // blend (p + 1) / 2 (it starts where that blend is entered)
    int i = N - 2;
    bool on_blend = false;
    double s = 0.0, sd = 0.0, u = 0.0, sy = 0.0, bi = 0.0;
    if (moving) {
        // the largest p with start <= t (the starts are non-decreasing, the first is 0; t < duration makes the next start > t)
        int lo = 0, hi = 2 * N - 4;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_T[mid + 1] <= t) lo = mid; else hi = mid - 1;
        }
        const double tau = t - s_T[lo + 1];
        on_blend = (lo & 1) != 0;
        if (on_blend) {
            i = (lo + 1) >> 1;
            bi = s_b[i];
            sy = sqrt(s_y[i]);
            u = (tau * sy) / (2.0 * bi);
            u = u > 0.0 ? u : 0.0;
            u = u < 1.0 ? u : 1.0;
        } else {
            i = lo >> 1;
            bi = s_b[i];
            const double ell = (1.0 - bi) - s_b[i + 1];
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
            s = bi + s;  // from waypoint i
        }
    }
    const double nan = __builtin_nan("");
    const size_t o = (size_t)slot * 7 * M + k;
    const double uu = u * u, w = 1.0 - u;
    const double ww = w * w;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double qv, qdv;
        if (!moving) {
            qv = timed ? s_x[j * kBlendN + N - 1] : nan;
            qdv = timed ? 0.0 : nan;
        } else if (on_blend) {
            const double x0 = s_x[j * kBlendN + i];
            const double dpj = x0 - s_x[j * kBlendN + i - 1], dj = s_x[j * kBlendN + i + 1] - x0;
            qv = x0 + bi * (uu * dj - ww * dpj);
            qdv = sy * (w * dpj + u * dj);
        } else {
            const double xa = s_x[j * kBlendN + i], xb = s_x[j * kBlendN + i + 1];
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

static int blend_check_limits(const char* what, const char* name, const double* v) {
    EDMP_REQUIRE(v, "%s: %s is a null pointer", what, name);
    for (int j = 0; j < 7; ++j) EDMP_REQUIRE(std::isfinite(v[j]) && v[j] > 0.0, "%s: %s[%d] = %g must be finite and > 0", what, name, j, v[j]);
    return EDMP_OK;
}

// the row list of a call, checked on the host: two workgroups on one row would write the same outputs
static int blend_check_rows(const char* what, const int32_t* rows_host, int n_rows, int n) {
    if (!rows_host) return EDMP_OK;
    EDMP_REQUIRE(n_rows >= 1 && n_rows <= n, "%s: %d listed rows outside 1..%d", what, n_rows, n);
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n_rows; ++i) {
        EDMP_REQUIRE(rows_host[i] >= 0 && rows_host[i] < n, "%s: rows[%d] = %d outside 0..%d", what, i, (int)rows_host[i], n - 1);
        EDMP_REQUIRE(!seen[rows_host[i]], "%s: rows[%d] = %d is listed twice", what, i, (int)rows_host[i]);
        seen[rows_host[i]] = 1;
    }
    return EDMP_OK;
}

// the checked list in a block of the call's own from the context's pool, given back by the caller after the call's synchronise
static int blend_upload_rows(edmp_ctx* ctx, const int32_t* rows_host, int n_rows, int32_t** rows_dev) {
    *rows_dev = nullptr;
    if (!rows_host) return EDMP_OK;
    if (int rc = ctx_alloc(ctx, (void**)rows_dev, (size_t)n_rows * sizeof(int32_t))) return rc;
    const hipError_t e = hipMemcpyAsync(*rows_dev, rows_host, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        ctx_release(ctx, *rows_dev);
        *rows_dev = nullptr;
        EDMP_HIP_CHECK(e);
    }
    return EDMP_OK;
}

// edmp_blend_rows_dev and edmp_scenes_blend_rows_dev behind their own state checks: n = S x rps rows of X (n, 7, N).  Every refusal
// comes before any device call.
static int blend_rows(edmp_ctx* ctx, const char* what, bool batch, const double* X_dev, int S, int rps, int N, const int32_t* rows_host, int n_rows,
                      const double* vmax, const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                      const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev) {
    Guide* g = ctx->guide;
    const int n = S * rps;
    EDMP_REQUIRE(X_dev && beta_dev && code_dev && halved_dev && tested_dev, "%s: null pointer", what);
    EDMP_REQUIRE(N >= 2 && N <= kBlendN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kBlendN, N);
    EDMP_REQUIRE(substeps >= 1 && substeps <= 8, "%s: substeps %d outside 1..8", what, substeps);
    EDMP_REQUIRE(halvings >= 0 && halvings <= 8, "%s: halvings %d outside 0..8", what, halvings);
    EDMP_REQUIRE(std::isfinite(reach) && reach > 0.0 && reach <= kBlendMaxReach, "%s: reach %g outside (0, %g]", what, reach, kBlendMaxReach);
    if (int rc = blend_check_limits(what, "vmax", vmax)) return rc;
    if (int rc = blend_check_limits(what, "amax", amax)) return rc;
    if (int rc = blend_check_limits(what, "jump", jump)) return rc;
    if (int rc = blend_check_limits(what, "deviation", deviation)) return rc;
    if (int rc = blend_check_rows(what, rows_host, n_rows, n)) return rc;
    const int launch = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int rc = blend_upload_rows(ctx, rows_host, n_rows, &rows_dev)) return rc;
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
    hipLaunchKernelGGL(blend_rows_kernel, dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), robot64_of(g, dh_f64));
    const hipError_t e = hipGetLastError();
    const hipError_t w = hipStreamSynchronize(ctx->stream);  // the list lives in the caller's array, its device block goes back to the pool
    if (rows_dev) ctx_release(ctx, rows_dev);
    EDMP_HIP_CHECK(w);
    EDMP_HIP_CHECK(e);
    return EDMP_OK;
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

extern "C" int edmp_time_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* vmax,
                                          const double* amax, const double* jump, double* y_dev, double* phase_dev, double* times_dev,
                                          double* duration_dev, int32_t* limit_dev, double* seg_dev, double* blend_dev) {
    const char* what = "edmp_time_blended_rows_dev";
    EDMP_REQUIRE(ctx, "%s: null context", what);
    EDMP_REQUIRE(X_dev && beta_dev && y_dev && phase_dev && times_dev && duration_dev && limit_dev && seg_dev && blend_dev, "%s: null pointer", what);
    EDMP_REQUIRE(n >= 1, "%s: need n >= 1 rows (got %d)", what, n);
    EDMP_REQUIRE(N >= 2 && N <= kBlendN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kBlendN, N);
    if (int rc = blend_check_limits(what, "vmax", vmax)) return rc;
    if (int rc = blend_check_limits(what, "amax", amax)) return rc;
    if (int rc = blend_check_limits(what, "jump", jump)) return rc;
    TimeBlendedArgs a;
    a.X = X_dev;
    a.beta = beta_dev;
    a.n = n;
    a.N = N;
    for (int j = 0; j < 7; ++j) a.vmax[j] = vmax[j], a.amax[j] = amax[j], a.jump[j] = jump[j];
    a.y = y_dev;
    a.phase = phase_dev;
    a.times = times_dev;
    a.duration = duration_dev;
    a.limit = limit_dev;
    a.seg = seg_dev;
    a.blend = blend_dev;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(time_blended_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, a);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

extern "C" int edmp_sample_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* y_dev,
                                            const double* phase_dev, const double* times_dev, const double* duration_dev, const double* seg_dev,
                                            const int32_t* rows_host, int n_rows, double period, int M, double* q_dev, double* qd_dev,
                                            int32_t* count_dev) {
    const char* what = "edmp_sample_blended_rows_dev";
    EDMP_REQUIRE(ctx, "%s: null context", what);
    EDMP_REQUIRE(X_dev && beta_dev && y_dev && phase_dev && times_dev && duration_dev && seg_dev && q_dev && qd_dev && count_dev, "%s: null pointer", what);
    EDMP_REQUIRE(n >= 1, "%s: need n >= 1 rows (got %d)", what, n);
    EDMP_REQUIRE(N >= 2 && N <= kBlendN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kBlendN, N);
    EDMP_REQUIRE(std::isfinite(period) && period > 0.0, "%s: period %g must be finite and > 0", what, period);
    EDMP_REQUIRE(M >= 1 && M <= EDMP_MAX_TIMED_SAMPLES, "%s: M = %d samples outside 1..%d", what, M, EDMP_MAX_TIMED_SAMPLES);
    if (int rc = blend_check_rows(what, rows_host, n_rows, n)) return rc;
    const int R = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int rc = blend_upload_rows(ctx, rows_host, n_rows, &rows_dev)) return rc;
    SampleBlendedArgs a;
    a.X = X_dev;
    a.beta = beta_dev;
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
    hipLaunchKernelGGL(sample_blended_rows_kernel, dim3(R, (M + kBlendChunk - 1) / kBlendChunk), dim3(kBlendChunk), 0, ctx->stream, a);
    const hipError_t e = hipGetLastError();
    const hipError_t w = hipStreamSynchronize(ctx->stream);
    if (rows_dev) ctx_release(ctx, rows_dev);
    EDMP_HIP_CHECK(w);
    EDMP_HIP_CHECK(e);
    return EDMP_OK;
}
