// ik.hip — batched numerical inverse kinematics of the 7-DoF Franka: the IK goal candidates of a whole scene group in one launch.
//
// Stands for (reference): FrankaRobot.ik of the problem's target pose (datasets/load_test_dataset.py:170-187), robofin's ikfast, which
// yields the 100 goal candidates the IK-goal filter then ranks (infer_serial.py:117-129).  ikfast is analytic and not part of this
// package; this is damped least squares from many seeds, so the candidates are OTHER points of the same solution continuum (the arm is
// redundant): every one reproduces the target pose to the stated tolerances, none is the reference's number.
//
// Design: one lane per seed, everything f64, the iteration count fixed inside the kernel.  Per iteration: the chain in modified DH
// (dh_step of chain.h) followed by the fixed tool frame; the error e = [p_t - p ; 1/2 sum_k R[:,k] x R_t[:,k]];
// the geometric 6 x 7 Jacobian from the joint frames' z axes and origins; A = J J^T + lambda^2 I by an unrolled Cholesky factorisation
// (SPD for lambda > 0), dq = J^T A^-1 e; the step scaled to max|dq| <= max_step and q clamped to the joint limits.  A workgroup is one
// wave (64 lanes) of ONE target, so the target pose is wave-uniform and a group of a few hundred seeds spreads over many CUs; every
// array is indexed by unrolled constants only, so the lane's state lives in registers (no private segment).  Lanes never talk to each
// other: a seed's result depends on (target, seed, parameters) alone, not on its neighbours, its block or the size of the call.
// Compaction: one workgroup walks the targets in order and writes the valid rows densely, in seed order (a ballot prefix per wave, the
// running base carried along) - stable and deterministic, the layout edmp_scenes_goal_filter_dev takes as goals_dev + n_goals.
#include <cmath>

#include "common.h"
#include "chain.h"

namespace edmp {

constexpr int kIkThreads = 64;
constexpr int kIkCompactThreads = 256;

struct IkRobot {
    double dh[7][4];  // a, d, cos(alpha), sin(alpha)
    double tool[12];  // row-major 3 x 4 [R | p] behind the joint-7 frame
    double qlo[7], qhi[7];
};

struct IkParams {
    int iters;
    double lambda2, max_step, tol_pos, tol_ang;
};

// blocks: (n_blocks, 3) int32 {target, first seed (row of the flat arrays), seeds in this block (1..64)}
__global__ __launch_bounds__(kIkThreads) void ik_solve_kernel(const double* __restrict__ targets, const int32_t* __restrict__ blocks,
                                                              const double* __restrict__ seeds, IkRobot rb, IkParams pr, double* __restrict__ q_out,
                                                              double* __restrict__ res_out, int32_t* __restrict__ valid_out) {
    const int32_t* bl = blocks + 3 * (size_t)blockIdx.x;
    if ((int)threadIdx.x >= bl[2]) return;
    const double* tg = targets + 12 * (size_t)bl[0];
    const size_t row = (size_t)bl[1] + threadIdx.x;
    double Rt[3][3], pt[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) Rt[a][b] = tg[a * 4 + b];
        pt[a] = tg[a * 4 + 3];
    }
    double q[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = seeds[row * 7 + j];
    double pos = 0.0, ang = 0.0;
#pragma unroll 1
    for (int it = 0;; ++it) {
        // FK: joint frame j = (R | o) after row j; its z axis and origin are joint j's axis
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        double o[3] = {0, 0, 0};
        double z[7][3], p[7][3];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double sq, cq;
            sincos(q[j], &sq, &cq);
            dh_step(R, o, sq, cq, rb.dh[j]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                z[j][a] = R[a][2];
                p[j][a] = o[a];
            }
        }
        // the tool frame
        double Re[3][3], pe[3];
        frame_apply(R, o, rb.tool, Re, pe);
        // error: position, and 1/2 sum_k Re[:,k] x Rt[:,k] (= sin(angle) * axis, world frame)
        double e[6];
        e[0] = pt[0] - pe[0];
        e[1] = pt[1] - pe[1];
        e[2] = pt[2] - pe[2];
        e[3] = e[4] = e[5] = 0.0;
        double tr = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e[3] += Re[1][k] * Rt[2][k] - Re[2][k] * Rt[1][k];
            e[4] += Re[2][k] * Rt[0][k] - Re[0][k] * Rt[2][k];
            e[5] += Re[0][k] * Rt[1][k] - Re[1][k] * Rt[0][k];
            tr += Re[0][k] * Rt[0][k] + Re[1][k] * Rt[1][k] + Re[2][k] * Rt[2][k];
        }
        e[3] *= 0.5;
        e[4] *= 0.5;
        e[5] *= 0.5;
        if (it >= pr.iters) {  // after the last step: the residuals of the q that is written
            pos = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            // the TRUE angle of Re^T Rt: the cross-product error alone is also zero at pi
            ang = atan2(sqrt(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]), 0.5 * (tr - 1.0));
            break;
        }
        // geometric Jacobian: column j = [z_j x (pe - p_j) ; z_j]
        double J[6][7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double d0 = pe[0] - p[j][0], d1 = pe[1] - p[j][1], d2 = pe[2] - p[j][2];
            J[0][j] = z[j][1] * d2 - z[j][2] * d1;
            J[1][j] = z[j][2] * d0 - z[j][0] * d2;
            J[2][j] = z[j][0] * d1 - z[j][1] * d0;
            J[3][j] = z[j][0];
            J[4][j] = z[j][1];
            J[5][j] = z[j][2];
        }
        // A = J J^T + lambda^2 I = L L^T (lower triangle in place), y = A^-1 e
        double L[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                double s = (a == b) ? pr.lambda2 : 0.0;
#pragma unroll
                for (int j = 0; j < 7; ++j) s += J[a][j] * J[b][j];
                L[a][b] = s;
            }
        }
        double inv[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b < a; ++b) {
                double s = L[a][b];
#pragma unroll
                for (int k = 0; k < b; ++k) s -= L[a][k] * L[b][k];
                L[a][b] = s * inv[b];
            }
            double d = L[a][a];
#pragma unroll
            for (int k = 0; k < a; ++k) d -= L[a][k] * L[a][k];
            inv[a] = 1.0 / sqrt(d);
        }
        double y[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double s = e[a];
#pragma unroll
            for (int k = 0; k < a; ++k) s -= L[a][k] * y[k];
            y[a] = s * inv[a];
        }
#pragma unroll
        for (int a = 5; a >= 0; --a) {
            double s = y[a];
#pragma unroll
            for (int k = a + 1; k < 6; ++k) s -= L[k][a] * y[k];
            y[a] = s * inv[a];
        }
        // dq = J^T y, scaled to max|dq| <= max_step; q clamped to the limits (a NaN stays a NaN)
        double dq[7], big = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) s += J[a][j] * y[a];
            dq[j] = s;
            big = fmax(big, fabs(s));
        }
        const double scale = big > pr.max_step ? pr.max_step / big : 1.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double v = q[j] + scale * dq[j];
            q[j] = v < rb.qlo[j] ? rb.qlo[j] : (v > rb.qhi[j] ? rb.qhi[j] : v);
        }
    }
    bool fin = isfinite(pos) && isfinite(ang);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        q_out[row * 7 + j] = q[j];
        fin = fin && isfinite(q[j]);
    }
    res_out[row * 2] = pos;
    res_out[row * 2 + 1] = ang;
    valid_out[row] = (fin && pos <= pr.tol_pos && ang <= pr.tol_ang) ? 1 : 0;
}

// off (T + 1,) int32: target t owns rows [off[t], off[t + 1]) of q / valid.  ONE workgroup: targets in order, each in chunks of 256
// rows; a valid row goes to goals[base + (valid rows before it)].  counts (T,) int32.
__global__ __launch_bounds__(kIkCompactThreads) void ik_compact_kernel(const double* __restrict__ q, const int32_t* __restrict__ valid,
                                                                       const int32_t* __restrict__ off, int T, double* __restrict__ goals,
                                                                       int32_t* __restrict__ counts) {
    __shared__ int s_wave[kIkCompactThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    int base = 0;
    for (int t = 0; t < T; ++t) {
        const int r0 = off[t], r1 = off[t + 1], start = base;
        for (int c = r0; c < r1; c += kIkCompactThreads) {
            const int r = c + tid;
            const bool v = r < r1 && valid[r] != 0;
            const unsigned long long m = __ballot(v);
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int w = 0; w < kIkCompactThreads / kWave; ++w) {
                const int n = s_wave[w];
                before += w < wave ? n : 0;
                total += n;
            }
            if (v) {
                const size_t dst = (size_t)(base + before) * 7, src = (size_t)r * 7;
#pragma unroll
                for (int j = 0; j < 7; ++j) goals[dst + j] = q[src + j];
            }
            base += total;
            __syncthreads();
        }
        if (tid == 0) counts[t] = base - start;
    }
}

}  // namespace edmp

using namespace edmp;

static bool ik_rows_total(const int32_t* n_seeds, int T, int64_t* total, int* bad) {
    *total = 0;
    for (int t = 0; t < T; ++t) {
        if (n_seeds[t] < 1) {
            *bad = t;
            return false;
        }
        *total += n_seeds[t];
    }
    return true;
}

extern "C" int edmp_ik_solve_dev(edmp_ctx* ctx, const double* targets, int T, const int32_t* n_seeds, const double* seeds_dev, const double* tool,
                                 int iters, double lambda, double max_step, double tol_pos, double tol_ang, double* q_dev, double* res_dev,
                                 int32_t* valid_dev) {
    EDMP_REQUIRE(ctx && targets && n_seeds && seeds_dev && tool && q_dev && res_dev && valid_dev,
                 "edmp_ik_solve_dev: context, targets, n_seeds, seeds, tool, q, residuals and valid are required (got%s%s%s%s%s%s%s%s NULL)", ctx ? "" : " ctx",
                 targets ? "" : " targets", n_seeds ? "" : " n_seeds", seeds_dev ? "" : " seeds", tool ? "" : " tool", q_dev ? "" : " q", res_dev ? "" : " residuals",
                 valid_dev ? "" : " valid");
    EDMP_REQUIRE(T >= 1, "edmp_ik_solve_dev: need T >= 1 targets (got %d)", T);
    int64_t total = 0;
    int bad = -1;
    EDMP_REQUIRE(ik_rows_total(n_seeds, T, &total, &bad), "edmp_ik_solve_dev: target %d brings %d seeds (need >= 1)", bad, n_seeds[bad]);
    EDMP_REQUIRE(total <= (int64_t)1 << 24, "edmp_ik_solve_dev: more than %d seeds in one call", 1 << 24);
    EDMP_REQUIRE(iters >= 1, "edmp_ik_solve_dev: need iters >= 1 (got %d)", iters);
    EDMP_REQUIRE(std::isfinite(lambda) && lambda > 0.0, "edmp_ik_solve_dev: lambda must be finite and > 0 (got %g): A = J J^T + lambda^2 I must be SPD", lambda);
    EDMP_REQUIRE(std::isfinite(max_step) && max_step > 0.0, "edmp_ik_solve_dev: max_step must be finite and > 0 (got %g)", max_step);
    EDMP_REQUIRE(std::isfinite(tol_pos) && tol_pos >= 0.0 && std::isfinite(tol_ang) && tol_ang >= 0.0,
                 "edmp_ik_solve_dev: tol_pos and tol_ang must be finite and >= 0 (got %g, %g)", tol_pos, tol_ang);
    auto orthonormal = [](const double* m, double* worst) {  // m: row-major 3 x 4; R^T R = I to 1e-9 and det > 0
        *worst = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double d = m[a] * m[b] + m[4 + a] * m[4 + b] + m[8 + a] * m[8 + b] - (a == b ? 1.0 : 0.0);
                *worst = std::fmax(*worst, std::fabs(d));
            }
        const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
        return *worst <= 1e-9 && det > 0.0;
    };
    double worst = 0.0;
    for (int i = 0; i < 12; ++i) EDMP_REQUIRE(std::isfinite(tool[i]), "edmp_ik_solve_dev: tool[%d] is not finite", i);
    EDMP_REQUIRE(orthonormal(tool, &worst), "edmp_ik_solve_dev: the tool frame's rotation is not orthonormal to 1e-9 (|R^T R - I| = %g) or is a reflection", worst);
    for (int t = 0; t < T; ++t) {
        for (int i = 0; i < 12; ++i) EDMP_REQUIRE(std::isfinite(targets[12 * (size_t)t + i]), "edmp_ik_solve_dev: target %d holds a non-finite value", t);
        EDMP_REQUIRE(orthonormal(targets + 12 * (size_t)t, &worst),
                     "edmp_ik_solve_dev: target %d: the rotation is not orthonormal to 1e-9 (|R^T R - I| = %g) or is a reflection", t, worst);
    }
    IkRobot rb;
    joint_dh64(nullptr, rb.dh);
    joint_limits_rad(rb.qlo, rb.qhi);
    for (int i = 0; i < 12; ++i) rb.tool[i] = tool[i];
    const IkParams pr = {iters, lambda * lambda, max_step, tol_pos, tol_ang};
    // the block table: every block is one wave of one target
    std::vector<int32_t> blocks;
    int32_t first = 0;
    for (int t = 0; t < T; ++t) {
        for (int32_t c = 0; c < n_seeds[t]; c += kIkThreads) {
            blocks.push_back(t);
            blocks.push_back(first + c);
            blocks.push_back(std::min<int32_t>(kIkThreads, n_seeds[t] - c));
        }
        first += n_seeds[t];
    }
    const int nb = (int)(blocks.size() / 3);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t tg_bytes = (size_t)T * 12 * sizeof(double), bl_bytes = blocks.size() * sizeof(int32_t);
    void* tmp = nullptr;
    if (int rc = ctx_alloc(ctx, &tmp, tg_bytes + bl_bytes)) return rc;
    double* tg_dev = (double*)tmp;
    int32_t* bl_dev = (int32_t*)((char*)tmp + tg_bytes);
    hipError_t err = hipMemcpyAsync(tg_dev, targets, tg_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(bl_dev, blocks.data(), bl_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(ik_solve_kernel, dim3(nb), dim3(kIkThreads), 0, ctx->stream, tg_dev, bl_dev, seeds_dev, rb, pr, q_dev, res_dev, valid_dev);
        err = hipGetLastError();
    }
    // the table is a temporary of this call: wait before it goes back to the pool (and before `blocks` leaves scope)
    const hipError_t serr = hipStreamSynchronize(ctx->stream);
    ctx_release(ctx, tmp);
    EDMP_HIP_CHECK(err);
    EDMP_HIP_CHECK(serr);
    return EDMP_OK;
}

extern "C" int edmp_ik_compact_dev(edmp_ctx* ctx, const double* q_dev, const int32_t* valid_dev, int T, const int32_t* n_seeds, double* goals_dev,
                                   int32_t* counts_host) {
    EDMP_REQUIRE(ctx && q_dev && valid_dev && n_seeds && goals_dev && counts_host,
                 "edmp_ik_compact_dev: context, q, valid, n_seeds, goals and counts are required (got%s%s%s%s%s%s NULL)", ctx ? "" : " ctx", q_dev ? "" : " q",
                 valid_dev ? "" : " valid", n_seeds ? "" : " n_seeds", goals_dev ? "" : " goals", counts_host ? "" : " counts");
    EDMP_REQUIRE(T >= 1, "edmp_ik_compact_dev: need T >= 1 targets (got %d)", T);
    int64_t total = 0;
    int bad = -1;
    EDMP_REQUIRE(ik_rows_total(n_seeds, T, &total, &bad), "edmp_ik_compact_dev: target %d brings %d seeds (need >= 1)", bad, n_seeds[bad]);
    EDMP_REQUIRE(total <= (int64_t)1 << 24, "edmp_ik_compact_dev: more than %d seeds in one call", 1 << 24);
    std::vector<int32_t> off(T + 1, 0);
    for (int t = 0; t < T; ++t) off[t + 1] = off[t] + n_seeds[t];
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    void* tmp = nullptr;
    if (int rc = ctx_alloc(ctx, &tmp, (size_t)(2 * T + 1) * sizeof(int32_t))) return rc;
    int32_t* off_dev = (int32_t*)tmp;
    int32_t* cnt_dev = off_dev + T + 1;
    hipError_t err = hipMemcpyAsync(off_dev, off.data(), (size_t)(T + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(ik_compact_kernel, dim3(1), dim3(kIkCompactThreads), 0, ctx->stream, q_dev, valid_dev, off_dev, T, goals_dev, cnt_dev);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(counts_host, cnt_dev, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t serr = hipStreamSynchronize(ctx->stream);
    ctx_release(ctx, tmp);
    EDMP_HIP_CHECK(err);
    EDMP_HIP_CHECK(serr);
    return EDMP_OK;
}
