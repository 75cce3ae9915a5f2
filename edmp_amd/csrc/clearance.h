// clearance.h — what the continuous certificate (certify.hip) needs beside the exact yes / no tests of linkbox.h: a LOWER BOUND on the
// distance between a link box and an obstacle, and a bound on how far a link box can move between two configurations.  Written the way
// chain.h is written: host and device, nothing from HIP included, no unroll pragmas, so a plain C++ compiler reads it too
// (tests/clearance_host prints gaps and radii on the CPU; tests/certify_inputs.py states the same rule as plain Python).
//
// gap: the maximum, over a list of UNIT axes, of the separation of the two shapes' projections.  Every such separation is a lower bound
// on the Euclidean distance, so the maximum is one; it is positive only if the shapes are disjoint.  It is not the distance: where the
// closest features are a vertex and a vertex (or a rim point), no listed axis is the connecting direction and the gap stays below it.
#pragma once
#include <cmath>

#include "chain.h"  // EDMP_CHAIN_FN

namespace edmp {

constexpr double kGapSatEps = 1e-12;       // == linkbox.h's kSatEps: the |R| + eps of obb_overlap, so that the radii are the exact test's
constexpr double kGapEdgeNorm2Min = 1e-6;  // an edge axis a_i x b_j with |a_i x b_j|^2 = 1 - R[i][j]^2 below this is skipped (near-parallel edges)
constexpr double kGapRadialMin = 1e-9;     // the radial cylinder axis is skipped where the box centre is this close to the cylinder's axis line

// box (Ra columns = axes, ca, ha) against the box ob (R 9 row-major, c 3, h 3), in obb_overlap's own quantities R, A = |R| + eps, t: the
// six face axes, then the nine edge axes a_i x b_j, each divided by its norm sqrt(1 - R[i][j]^2)
EDMP_CHAIN_FN double box_box_gap(const double Ra[3][3], const double ca[3], const double ha[3], const double* ob) {
    double R[3][3], A[3][3], t[3];
    const double d0 = ob[9] - ca[0], d1 = ob[10] - ca[1], d2 = ob[11] - ca[2];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            R[i][j] = Ra[0][i] * ob[j] + Ra[1][i] * ob[3 + j] + Ra[2][i] * ob[6 + j];
            A[i][j] = fabs(R[i][j]) + kGapSatEps;
        }
        t[i] = Ra[0][i] * d0 + Ra[1][i] * d1 + Ra[2][i] * d2;
    }
    const double hb[3] = {ob[12], ob[13], ob[14]};
    double g = fabs(t[0]) - (ha[0] + (hb[0] * A[0][0] + hb[1] * A[0][1] + hb[2] * A[0][2]));
    for (int i = 1; i < 3; ++i) g = fmax(g, fabs(t[i]) - (ha[i] + (hb[0] * A[i][0] + hb[1] * A[i][1] + hb[2] * A[i][2])));
    for (int j = 0; j < 3; ++j)
        g = fmax(g, fabs(t[0] * R[0][j] + t[1] * R[1][j] + t[2] * R[2][j]) - ((ha[0] * A[0][j] + ha[1] * A[1][j] + ha[2] * A[2][j]) + hb[j]));
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const double n2 = 1.0 - R[i][j] * R[i][j];
            if (n2 < kGapEdgeNorm2Min) continue;
            const double ra = ha[i1] * A[i2][j] + ha[i2] * A[i1][j];
            const double rb = hb[j1] * A[i][j2] + hb[j2] * A[i][j1];
            g = fmax(g, (fabs(t[i2] * R[i1][j] - t[i1] * R[i2][j]) - (ra + rb)) / sqrt(n2));
        }
    }
    return g;
}

// box (Rb, cb, hb) against the finite cylinder ob, the (r, r, h) row read as obb_cylinder_overlap_body reads it (radius 2 ob[12], half
// height ob[14], axis = third column of the rotation): in the cylinder's frame (R columns = box axes, t = box centre) the cylinder axis,
// the three box normals n against the cylinder's extent H |n.z| + r sqrt(1 - (n.z)^2), and the radial direction from the axis line to
// the box centre
EDMP_CHAIN_FN double box_cylinder_gap(const double Rb[3][3], const double cb[3], const double hb[3], const double* ob) {
    double R[3][3], t[3];
    const double d0 = cb[0] - ob[9], d1 = cb[1] - ob[10], d2 = cb[2] - ob[11];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i][j] = ob[i] * Rb[0][j] + ob[3 + i] * Rb[1][j] + ob[6 + i] * Rb[2][j];
        t[i] = ob[i] * d0 + ob[3 + i] * d1 + ob[6 + i] * d2;
    }
    const double H = ob[14], rad = 2.0 * ob[12];
    double g = (fabs(t[2]) - H) - (hb[0] * fabs(R[2][0]) + hb[1] * fabs(R[2][1]) + hb[2] * fabs(R[2][2]));
    for (int i = 0; i < 3; ++i) {
        const double nz = R[2][i];
        const double ext = H * fabs(nz) + rad * sqrt(fmax(0.0, 1.0 - nz * nz));
        g = fmax(g, (fabs(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) - hb[i]) - ext);
    }
    const double d = sqrt(t[0] * t[0] + t[1] * t[1]);
    if (!(d < kGapRadialMin)) {
        const double ux = t[0] / d, uy = t[1] / d;
        const double ext = hb[0] * fabs(ux * R[0][0] + uy * R[1][0]) + hb[1] * fabs(ux * R[0][1] + uy * R[1][1]) + hb[2] * fabs(ux * R[0][2] + uy * R[1][2]);
        g = fmax(g, (d - rad) - ext);
    }
    return g;
}

// the joint frame link l rides (franka.LINK_FRAME): link7, hand and finger ride the last one
EDMP_CHAIN_FN int link_frame(int l) { return l < 7 ? l : 6; }

// rho[l * 7 + j]: turning joint j alone by dq carries every point of link box l along an arc of radius <= rho, so it moves <= |dq| rho.
// The joint's axis passes through the origin o_j of its frame; a point c of the box (in its static frame (S | p), corner c = +-he) lies
// at most sum_{i = j+1..k} |o_i - o_{i-1}| + |p + S c| from o_j, k the frame the link rides, and the distance between successive
// modified-DH origins, |(a_i, -sin(alpha_i) d_i, cos(alpha_i) d_i)| = sqrt(a_i^2 + d_i^2), depends on no joint value.  0 for j > k.
inline void motion_radii(const double dh[7][4], const double sf[9][12], const double he[9][3], double rho[63]) {
    for (int l = 0; l < 9; ++l) {
        const int k = link_frame(l);
        double far = 0.0;
        for (int c = 0; c < 8; ++c) {
            const double x = (c & 1) ? he[l][0] : -he[l][0], y = (c & 2) ? he[l][1] : -he[l][1], z = (c & 4) ? he[l][2] : -he[l][2];
            double v[3];
            for (int a = 0; a < 3; ++a) v[a] = sf[l][4 * a + 3] + (sf[l][4 * a] * x + sf[l][4 * a + 1] * y + sf[l][4 * a + 2] * z);
            far = fmax(far, sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
        }
        for (int j = 0; j < 7; ++j) {
            double s = 0.0;
            for (int i = j + 1; i <= k; ++i) s = s + sqrt(dh[i][0] * dh[i][0] + dh[i][1] * dh[i][1]);
            rho[l * 7 + j] = j <= k ? s + far : 0.0;
        }
    }
}

}  // namespace edmp
