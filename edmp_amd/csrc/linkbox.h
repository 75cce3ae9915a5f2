// linkbox.h — what the exact f64 link-box checks share: the robot tables in f64, the box / box separating-axis test, the box / cylinder
// test, the test of ONE configuration against a scene's obstacles and the test of ONE configuration's link boxes against each other (the
// pair plan of a (9, 9) mask, one lower link with its masked partners).  success.hip (link boxes against the scene's obstacles),
// shortcut.hip and blend.hip (both tests on the configurations of a candidate) and selfcol.hip (link boxes against each other) include it.
#pragma once
#include "common.h"
#include "chain.h"
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

// intersect [lo, hi] with { s : |p + s d| <= h }
__device__ __forceinline__ void clip_iv(double& lo, double& hi, double p, double d, double h) {
    if (d == 0.0) {
        if (!(fabs(p) <= h)) {
            lo = 1.0;
            hi = 0.0;
        }
        return;
    }
    double s0 = (-h - p) / d, s1 = (h - p) / d;
    if (s0 > s1) {
        const double tmp = s0;
        s0 = s1;
        s1 = tmp;
    }
    lo = fmax(lo, s0);
    hi = fmin(hi, s1);
}

__device__ __forceinline__ double seg_dist2_origin(double ax, double ay, double bx, double by) {
    const double dx = bx - ax, dy = by - ay;
    const double dd = dx * dx + dy * dy;
    const double s = dd == 0.0 ? 0.0 : fmin(1.0, fmax(0.0, -(ax * dx + ay * dy) / dd));
    const double px = ax + s * dx, py = ay + s * dy;
    return px * px + py * py;
}

// box against the finite cylinder of axis = third column of the obstacle rotation, radius ob[12] * 2 (the (r, r, h) row
// carries full extents, stored halved), half height ob[14].  In the cylinder frame the box clipped to the slab |z| <= H is
// a convex polytope P; the shapes meet iff min over P of x^2 + y^2 <= r^2: 0 if the axis line pierces P, else attained on a
// projected edge of P (12 clipped box edges + the face x cap-plane segments).  oracle/success_oracle.py, same steps.
// INDEXED chooses how the cap-plane part fetches the two in-plane axes of a face (below): the values are the same.
template <bool INDEXED>
__device__ __forceinline__ bool obb_cylinder_overlap_body(const double Rb[3][3], const double cb[3], const double hb[3], const double* __restrict__ ob) {
    double R[3][3], t[3];
    const double d0 = cb[0] - ob[9], d1 = cb[1] - ob[10], d2 = cb[2] - ob[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = ob[i] * Rb[0][j] + ob[3 + i] * Rb[1][j] + ob[6 + i] * Rb[2][j];
        t[i] = ob[i] * d0 + ob[3 + i] * d1 + ob[6 + i] * d2;
    }
    const double H = ob[14], rad = 2.0 * ob[12], r2 = rad * rad;
    if (fabs(t[2]) > H + hb[0] * fabs(R[2][0]) + hb[1] * fabs(R[2][1]) + hb[2] * fabs(R[2][2])) return false;
    {
        double lo = -H, hi = H;
#pragma unroll
        for (int i = 0; i < 3; ++i) clip_iv(lo, hi, -(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]), R[2][i], hb[i]);
        if (lo <= hi) return true;
    }
    bool hit = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double sj = (c & 2) ? hb[j] : -hb[j], sk = (c & 1) ? hb[k] : -hb[k];
            double p0[3], d[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                p0[m] = t[m] + sj * R[m][j] + sk * R[m][k] - hb[i] * R[m][i];
                d[m] = 2.0 * hb[i] * R[m][i];
            }
            double s0 = 0.0, s1 = 1.0;
            clip_iv(s0, s1, p0[2], d[2], H);
            if (s0 <= s1) hit |= seg_dist2_origin(p0[0] + s0 * d[0], p0[1] + s0 * d[1], p0[0] + s1 * d[0], p0[1] + s1 * d[1]) <= r2;
        }
    }
    if (hit) return true;
    // the face x cap-plane segments: in face coordinates (a, b) the cut is the line nj a + nk b = e, parametrised by the
    // coordinate with the smaller normal component and solved for the other (division by the dominant component only)
#pragma unroll
    for (int cap = 0; cap < 2; ++cap) {
        const double cz = cap ? -H : H;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int j = (i + 1) % 3, k = (i + 2) % 3;
            double nj = R[2][j], nk = R[2][k];
            double Rj0, Rj1, Rk0, Rk1, hj, hk;
            if (INDEXED) {  // j and k become run-time indices: the arrays they index live in the callee's frame
                if (fabs(nk) > fabs(nj)) {
                    const int tj = j;
                    j = k;
                    k = tj;
                    const double tn = nj;
                    nj = nk;
                    nk = tn;
                }
                if (nj == 0.0) continue;  // face parallel to the cap: its edges are box edges
                Rj0 = R[0][j], Rj1 = R[1][j], Rk0 = R[0][k], Rk1 = R[1][k], hj = hb[j], hk = hb[k];
            } else {  // the same values chosen from registers: no private memory
                const bool swap = fabs(nk) > fabs(nj);
                Rj0 = swap ? R[0][k] : R[0][j], Rj1 = swap ? R[1][k] : R[1][j], Rk0 = swap ? R[0][j] : R[0][k], Rk1 = swap ? R[1][j] : R[1][k];
                hj = swap ? hb[k] : hb[j], hk = swap ? hb[j] : hb[k];
                const double tn = nj;
                nj = swap ? nk : nj;
                nk = swap ? tn : nk;
                if (nj == 0.0) continue;
            }
            const double d = -nk / nj;
#pragma unroll
            for (int sgn = 0; sgn < 2; ++sgn) {
                const double si = sgn ? hb[i] : -hb[i];
                const double f0 = t[0] + si * R[0][i], f1 = t[1] + si * R[1][i], f2 = t[2] + si * R[2][i];
                const double p = (cz - f2) / nj;
                double lo = -hk, hi = hk;
                clip_iv(lo, hi, p, d, hj);
                if (lo <= hi) {
                    const double aa = p + d * lo, ba = p + d * hi;
                    hit |= seg_dist2_origin(f0 + aa * Rj0 + lo * Rk0, f1 + aa * Rj1 + lo * Rk1, f0 + ba * Rj0 + hi * Rk0, f1 + ba * Rj1 + hi * Rk1) <= r2;
                }
            }
        }
    }
    return hit;
}

// the same test as a real call: the box goes by address and the callee has a frame of its own (success_rows_kernel's stack)
__device__ __noinline__ inline bool obb_cylinder_overlap(const double Rb[3][3], const double cb[3], const double hb[3], const double* __restrict__ ob) {
    return obb_cylinder_overlap_body<true>(Rb, cb, hb, ob);
}

// joint value of the interpolant at fraction f of the segment a -> b, (1 - f) a + f b, as both kernels that test interpolants form it.
// The shortcut stage's guarantee - every configuration the success check tests on an accepted piece was tested - needs the same BITS in
// two translation units, so the one fused multiply-add is written out and does not hang on each unit's contraction setting: the rounded
// product f b, then fma(1 - f, a, .).  (What the compiler made of the plain expression in success_rows_kernel before: its results stay.)
// self_collision_rows_kernel writes the plain expression (1.0 - f) * a + f * b; its code object holds ONE v_mul_f64 (f b) and ONE
// v_fmac_f64 (that product plus (1 - f) a, one rounding) for it - this form, read off the disassembly -, so the self items of shortcut.hip take their configurations
// through interp_joint too and see the bits self_collision_rows will form on the output.  NOTHING pins that contraction: another compiler,
// other flags or a contraction pragma in selfcol.hip can give the plain expression there another rounding, and the bit-level form of the
// guarantee (a row self_collision_rows calls free before a shortcut is free after it) then holds only up to one rounding of a joint value -
// whoever changes how selfcol.hip is built reads its disassembly again, or writes interp_joint there (which would change its results).
__device__ __forceinline__ double interp_joint(double a, double b, double f) { return fma(1.0 - f, a, f * b); }

// ONE configuration against the `no` obstacles ob / kind (16 doubles and one int each): the chain walk in f64, every link box
// riding a joint frame against every obstacle - boxes by obb_overlap, cylinders by the clipped-polytope test.  joint(j) gives the
// value of joint j; it is asked once per joint, in order.  CYL_CALL: the cylinder test is a call (a stack), else it is inlined.
// Returns at the first hit: touching counts.
template <bool CYL_CALL, class Joint>
__device__ __forceinline__ bool configuration_hits(Joint joint, const Robot64& rc, const double* ob_all, const int* kind, int no) {
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double o[3] = {0, 0, 0};
    bool hit = false;
#pragma unroll 1
    for (int j = 0; j < 7 && !hit; ++j) {
        double sq, cq;
        sincos(joint(j), &sq, &cq);
        dh_step(R, o, sq, cq, rc.dh[j]);
        const int nl = (j == 6) ? 3 : 1;  // link7, hand and finger ride the last frame               lib/guide.py:93-94
        for (int ll = 0; ll < nl && !hit; ++ll) {
            const int l = (ll == 0) ? j : 6 + ll;
            double LR[3][3], Lc[3], he[3];
            frame_apply(R, o, rc.sf[l], LR, Lc);
#pragma unroll
            for (int a = 0; a < 3; ++a) he[a] = rc.he[l][a];
            for (int ob = 0; ob < no && !hit; ++ob) {
                const double* od = ob_all + ob * 16;
                if (kind[ob] == 1)
                    hit = CYL_CALL ? obb_cylinder_overlap(LR, Lc, he, od) : obb_cylinder_overlap_body<false>(LR, Lc, he, od);
                else
                    hit = obb_overlap(LR, Lc, he, od);
            }
        }
    }
    return hit;
}

// ---- link boxes against each other -------------------------------------------------------------------------------------------------------
// the lower links with a non-empty mask row, ascending: link a, the mask bits of its partners b > a, the last joint frame one of them rides
struct PairPlan {
    int na;
    int a[EDMP_N_LINKS - 1], bits[EDMP_N_LINKS - 1], jlast[EDMP_N_LINKS - 1];
};

// ONE configuration, ONE lower link a, its masked partners `bits` (b > a): walk the chain to a's frame and keep that one box pose (12
// doubles), walk on and test each masked b by obb_overlap as its frame arrives (the frame of link l is monotone in l, so b's never
// precedes a's), stop at the first hit - b ascends, so it is the smallest - or after frame jlast.  -> that b, or -1.  joint(j) gives the
// value of joint j; it is asked once per joint, in order, up to jlast at most.  The rules of selfcol.hip hold here: nine f64 frames are
// not held per thread (re-walking the chain per a costs a few sincos, the frames would cost the registers), the joint loop is not
// unrolled and no per-thread array is indexed by the joint number - every table index (joint, link) is uniform over the lanes still in
// the loop -, so nothing goes to scratch.
template <class Joint>
__device__ __forceinline__ int configuration_self_hit(Joint joint, const Robot64& rc, int a, int bits, int jlast) {
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double o[3] = {0, 0, 0};
    double Ra[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, ca[3] = {0, 0, 0}, ha[3] = {0, 0, 0};
    int hit = -1;
#pragma unroll 1
    for (int j = 0; j <= jlast && hit < 0; ++j) {
        const double q = joint(j);
        double sq, cq;
        sincos(q, &sq, &cq);
        dh_step(R, o, sq, cq, rc.dh[j]);
        const int nl = (j == 6) ? 3 : 1;  // link7, hand and finger ride the last frame               lib/guide.py:93-94
#pragma unroll 1
        for (int ll = 0; ll < nl && hit < 0; ++ll) {
            const int l = (ll == 0) ? j : 6 + ll;
            if (l < a || (l > a && !((bits >> l) & 1))) continue;
            double ob[15];
            {
                double LR[3][3], Lc[3];
                frame_apply(R, o, rc.sf[l], LR, Lc);
#pragma unroll
                for (int m = 0; m < 3; ++m) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) ob[m * 3 + k] = LR[m][k];
                    ob[9 + m] = Lc[m];
                    ob[12 + m] = rc.he[l][m];
                }
            }
            if (l == a) {  // the one pose this item keeps
#pragma unroll
                for (int m = 0; m < 3; ++m) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) Ra[m][k] = ob[m * 3 + k];
                    ca[m] = ob[9 + m];
                    ha[m] = ob[12 + m];
                }
            } else if (obb_overlap(Ra, ca, ha, ob)) {
                hit = l;
            }
        }
    }
    return hit;
}

// what a kernel templated on SELF reads its further arguments through: the ONE element of the SELF instantiation's argument pack, nothing
// for the plain instantiation (whose kernel arguments are then exactly what they were before the template)
struct NoSelfArguments {};
__device__ __forceinline__ NoSelfArguments self_arguments() { return {}; }
template <class T>
__device__ __forceinline__ const T& self_arguments(const T& t) {
    return t;
}

// the plan of an 81-entry 0/1 mask of which the entries above the diagonal are read.  -> false with (*bad_a, *bad_b) the first entry that
// is neither 0 nor 1 (the plan is then not to be used)
inline bool pair_plan_of(const int32_t* pair_mask, PairPlan* plan, int* bad_a, int* bad_b) {
    *plan = PairPlan{};
    for (int a = 0; a < EDMP_N_LINKS; ++a) {
        int bits = 0, jlast = 0;
        for (int b = a + 1; b < EDMP_N_LINKS; ++b) {  // (entries on or below the diagonal are not read)
            const int32_t m = pair_mask[a * EDMP_N_LINKS + b];
            if (m != 0 && m != 1) {
                *bad_a = a;
                *bad_b = b;
                return false;
            }
            if (m) {
                bits |= 1 << b;
                jlast = b < 7 ? b : 6;  // the joint frame link b rides (franka.LINK_FRAME)
            }
        }
        if (bits) {
            plan->a[plan->na] = a;
            plan->bits[plan->na] = bits;
            plan->jlast[plan->na] = jlast;
            plan->na++;
        }
    }
    return true;
}

// the obstacle rows of every scene of the guide object inside obb / kind: scene s owns rows [off[s], off[s] + cnt[s]); row r of the
// state belongs to scene r / rps.  One scene: rps = B, off[0] = 0, cnt[0] = no.
struct SceneSlices {
    int rps;
    int off[EDMP_MAX_SCENES], cnt[EDMP_MAX_SCENES];
};

// the slices of a guide: a scene batch's own offsets and counts, or the whole table of a single-scene guide for all rps rows
inline SceneSlices scene_slices_of(const Guide* g, bool batch, int S, int rps) {
    SceneSlices sl = {};
    sl.rps = rps;
    for (int s = 0; s < S; ++s) {
        sl.off[s] = batch ? g->scene_off_h[s] : 0;  // (the single-scene call: the whole table, g->no obstacles)
        sl.cnt[s] = batch ? g->scene_no_h[s] : g->no;
    }
    return sl;
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
