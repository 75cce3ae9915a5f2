// linkbox.h — what the two exact f64 link-box checks share: the robot tables in f64 and the box / box separating-axis test.
// success.hip (link boxes against the scene's obstacles) and selfcol.hip (link boxes against each other) include it.
#pragma once
#include "common.h"
#include "guide.h"

namespace edmp {

struct Robot64 {
    double dh[7][4];   // a, d, cos(alpha), sin(alpha)
    double sf[9][12];  // static frames, row-major 3x4
    double he[9][3];   // link half extents
    double qlo[7], qhi[7];
};

constexpr double kSatEps = 1e-12;  // added to |R|: near-parallel edge pairs must not produce a null axis

// box (Ra columns = axes, ca, ha) against box: 15 candidate separating axes; touching counts as overlap
__device__ __forceinline__ bool obb_overlap(const double Ra[3][3], const double ca[3], const double ha[3], const double* __restrict__ ob) {
    // ob: R (9, row-major), c (3), h (3)
    double R[3][3], A[3][3], t[3];
    const double d0 = ob[9] - ca[0], d1 = ob[10] - ca[1], d2 = ob[11] - ca[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[i][j] = Ra[0][i] * ob[j] + Ra[1][i] * ob[3 + j] + Ra[2][i] * ob[6 + j];
            A[i][j] = fabs(R[i][j]) + kSatEps;
        }
        t[i] = Ra[0][i] * d0 + Ra[1][i] * d1 + Ra[2][i] * d2;
    }
    const double hb0 = ob[12], hb1 = ob[13], hb2 = ob[14];
    const double hb[3] = {hb0, hb1, hb2};
    bool sep = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) sep |= fabs(t[i]) > ha[i] + (hb0 * A[i][0] + hb1 * A[i][1] + hb2 * A[i][2]);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        sep |= fabs(t[0] * R[0][j] + t[1] * R[1][j] + t[2] * R[2][j]) > (ha[0] * A[0][j] + ha[1] * A[1][j] + ha[2] * A[2][j]) + hb[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const double ra = ha[i1] * A[i2][j] + ha[i2] * A[i1][j];
            const double rb = hb[j1] * A[i][j2] + hb[j2] * A[i][j1];
            sep |= fabs(t[i2] * R[i1][j] - t[i1] * R[i2][j]) > ra + rb;
        }
    }
    return !sep;
}

// (no dh_f64: the scene's own f32 table widened, as include/edmp_hip.h promises - not the Franka table of chain.h's joint_dh64)
inline Robot64 robot64_of(const Guide* g, const double* dh_f64) {
    Robot64 rc;
    for (int j = 0; j < 7; ++j)
        for (int k = 0; k < 4; ++k) rc.dh[j][k] = dh_f64 ? dh_f64[j * 4 + k] : (double)g->rc.dh[j][k];
    for (int l = 0; l < 9; ++l) {
        for (int k = 0; k < 12; ++k) rc.sf[l][k] = (double)g->rc.sf[l][k];
        for (int k = 0; k < 3; ++k) rc.he[l][k] = (double)g->rc.he[l][k];
    }
    for (int j = 0; j < 7; ++j) {
        rc.qlo[j] = g->rc.qlo[j];
        rc.qhi[j] = g->rc.qhi[j];
    }
    return rc;
}

}  // namespace edmp
