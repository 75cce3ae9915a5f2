// chain.h — the Franka's modified-DH chain, stated once per number type, and the robot constants the host sides fill in.  f64:
// success_rows_kernel, metrics_rows_kernel, ik_solve_kernel.  f32: sdf_row; guide_kernel holds the same text inline (guide.hip says why).
// Two overloads, not one template: the f32 form nests its fmaf calls the way guide.hip matches torch's f32 matmul, the f64 form is the
// plain a*b + c*d + e*f of the f64 checkers; each compiles to what its kernels held inline.  Nothing from HIP is included and the
// three-trip loops carry no unroll pragma, so a C++ compiler reads this file too: tests/chain_host walks both chains on the CPU.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define EDMP_CHAIN_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define EDMP_CHAIN_FN inline
#endif

namespace edmp {

// (R | o) <- (R | o) * DH(a, d, cos(alpha), sin(alpha), q): modified DH, dh = {a, d, ca, sa}, sq / cq = sin / cos of the joint value
// (the caller's own sinf / cosf / sincos)                                                             lib/guide.py:45-72, 92
EDMP_CHAIN_FN void dh_step(float R[3][3], float o[3], float sq, float cq, const float dh[4]) {
    const float aa = dh[0], dd = dh[1], ca = dh[2], sa = dh[3];
    const float D[3][4] = {{cq, -sq, 0.f, aa}, {sq * ca, cq * ca, -sa, -sa * dd}, {sq * sa, cq * sa, ca, ca * dd}};
    float Rn[3][3], on[3];
    for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) Rn[i][c] = fmaf(R[i][2], D[2][c], fmaf(R[i][1], D[1][c], R[i][0] * D[0][c]));
        on[i] = fmaf(R[i][2], D[2][3], fmaf(R[i][1], D[1][3], R[i][0] * D[0][3])) + o[i];
    }
    for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) R[i][c] = Rn[i][c];
        o[i] = on[i];
    }
}
EDMP_CHAIN_FN void dh_step(double R[3][3], double o[3], double sq, double cq, const double dh[4]) {
    const double aa = dh[0], dd = dh[1], ca = dh[2], sa = dh[3];
    const double D[3][4] = {{cq, -sq, 0.0, aa}, {sq * ca, cq * ca, -sa, -sa * dd}, {sq * sa, cq * sa, ca, ca * dd}};
    double Rn[3][3], on[3];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) Rn[a][b] = R[a][0] * D[0][b] + R[a][1] * D[1][b] + R[a][2] * D[2][b];
        on[a] = R[a][0] * D[0][3] + R[a][1] * D[1][3] + R[a][2] * D[2][3] + o[a];
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) R[a][b] = Rn[a][b];
        o[a] = on[a];
    }
}

// (LR | Lo) = (R | o) * frame, frame a row-major 3 x 4 [R | p]: a link box's static frame, the IK tool frame       lib/guide.py:350
EDMP_CHAIN_FN void frame_apply(const float R[3][3], const float o[3], const float f[12], float LR[3][3], float Lo[3]) {
    for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) LR[i][c] = fmaf(R[i][2], f[8 + c], fmaf(R[i][1], f[4 + c], R[i][0] * f[c]));
        Lo[i] = fmaf(R[i][2], f[11], fmaf(R[i][1], f[7], R[i][0] * f[3])) + o[i];
    }
}
EDMP_CHAIN_FN void frame_apply(const double R[3][3], const double o[3], const double f[12], double LR[3][3], double Lo[3]) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) LR[a][b] = R[a][0] * f[b] + R[a][1] * f[4 + b] + R[a][2] * f[8 + b];
        Lo[a] = R[a][0] * f[3] + R[a][1] * f[7] + R[a][2] * f[11] + o[a];
    }
}

// the four-wave link grouping of guide_kernel<.., 4> and sdf_row: {0,1,2}, {3,4}, {5,6}, {hand, finger} (balanced on obstacle loop +
// corner search + chain rule + the DH prefix a group has to walk), and the last joint frame a wave's links ride
EDMP_CHAIN_FN int link_wave(int l) { return l < 3 ? 0 : l < 5 ? 1 : l < 7 ? 2 : 3; }
EDMP_CHAIN_FN int wave_last_joint(int wv) { return wv == 0 ? 2 : wv == 1 ? 4 : 6; }

// ---- host side: the robot constants ------------------------------------------------------------------------------------------
constexpr double kPi = 3.141592653589793;  // == numpy.pi
// the seven joint rows [a, d, alpha] of the reference's modified-DH table (lib/guide.py:29-35) = franka.DH_A_D_ALPHA
constexpr double kJointDh[7][3] = {{0, 0.333, 0},           {0, 0, -kPi / 2},   {0, 0.316, kPi / 2}, {0.0825, 0, kPi / 2},
                                   {-0.0825, 0.384, -kPi / 2}, {0, 0, kPi / 2}, {0.088, 0, kPi / 2}};
// rows 8-10 [a, d, alpha, theta] of the same table (lib/guide.py:36-38) = evaluation.EE_STATIC_DH: the end effector behind joint 7
constexpr double kEeStaticDh[3][4] = {{0.0, 0.107, 0.0, 0.0}, {0.0, 0.0, 0.0, -kPi / 4}, {0.0, 0.1034, 0.0, 0.0}};
// franka.JOINT_LOWER_DEG / JOINT_UPPER_DEG (diffusion/diffusion.py:282-296)
constexpr double kJointLowerDeg[7] = {-166.0, -101.0, -166.0, -176.0, -166.0, -1.0, -166.0};
constexpr double kJointUpperDeg[7] = {166.0, 101.0, 166.0, -4.0, 166.0, 215.0, 166.0};

// out = the caller's (7, 4) f64 rows [a, d, cos(alpha), sin(alpha)], or the table above when it passes none (franka.dh_table_f64())
inline void joint_dh64(const double* dh_f64_or_null, double out[7][4]) {
    for (int j = 0; j < 7; ++j) {
        const double row[4] = {kJointDh[j][0], kJointDh[j][1], std::cos(kJointDh[j][2]), std::sin(kJointDh[j][2])};
        for (int k = 0; k < 4; ++k) out[j][k] = dh_f64_or_null ? dh_f64_or_null[j * 4 + k] : row[k];
    }
}
// the limits in rad as deg * (pi / 180), the way diffusion.py:282-296 and franka.joint_limits() evaluate them
inline void joint_limits_rad(double qlo[7], double qhi[7]) {
    for (int j = 0; j < 7; ++j) {
        qlo[j] = kJointLowerDeg[j] * (kPi / 180);
        qhi[j] = kJointUpperDeg[j] * (kPi / 180);
    }
}

}  // namespace edmp
