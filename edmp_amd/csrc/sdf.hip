// sdf.hip — the sphere signed-distance guide for gfx950: a third guidance method beside the AABB-overlap volumes of guide.hip.
//
// No live counterpart in the reference: its sphere / SDF collision loss exists only in the vendored mpinets (mpinets/loss.py:47-94,
// mpinets/geometry.py:238-288, 456-507) and its smoothness_cost (lib/guide.py:670-677) is never called.  The cost of a row at step t,
// over the padded waypoints w = 0..L+1 (start, the L interior waypoints, goal), all arithmetic in f32:
//   c(w, s)   = T_frame(link_s)(q_w) * static_frame[link_s] * centre_s       the chain, frames and link -> frame map of guide_kernel
//   sdf_o(p)  = ||max(e, 0)|| + min(max_k e_k, 0)                            cuboid: e = |R_o^T (p - c_o)| - h_o
//                                                                            cylinder: the same in 2-D on (rho - r, |z| - height / 2)
//   d(w, s)   = min_o sdf_o(c(w, s)) - radius_s
//   collision = sum_{w=1..L} sum_s max(0, m - d(w, s))                       m = sdf_margin[r][t - 1] for t >= 1, 0 at t = 0
//   smooth    = smoothness[r] * sum_{w=0..L} ||q_{w+1} - q_w||^2             the FULL padded chain (lib/guide.py:670-677 drops both ends)
//   cost      = collision + smooth;  the gradient is taken with respect to the L interior waypoints.
// The obstacles are the TRUE primitives of the success check (Guide::obb / Guide::kind): oriented boxes, and cylinders of radius
// dims[0] and half height dims[2] / 2 about their local z axis (success.hip, lib/environment.py:249-268).
//
// Sub-gradient conventions (the kernel holds to them; a checker has to keep its inputs away from these boundaries):
//   * the first obstacle index wins a min_o tie (strict < in obstacle order);
//   * the hinge is active iff m - d > 0;
//   * inside a box the first axis of the maximal e_k carries the gradient;
//   * ||.|| at exactly 0 (and rho = 0 on a cylinder axis, |p_k| at p_k = 0) contributes a zero gradient - torch gives NaN at the norm.
//
// Layout (that of guide_kernel<GM_GRAD, ., 4>): one 256-thread workgroup per row, lane = padded waypoint, the four waves take the
// link groups {0,1,2}, {3,4}, {5,6}, {hand, finger} and meet in wave 0 (meet_in_wave0): no atomics, every sum has one order.  The row's
// obstacles are staged once per workgroup as f32 [16] = rotation (row-major, columns = axes) | centre | half extents | kind, the sphere
// table (sorted by link on the host, table order kept inside a link) as f32 [4] = centre | radius.
//
// Scene batch (edmp_scene_batch_set_sdf): a row is one workgroup, hence one scene = row / rps.  The workgroup stages the obstacles and
// kinds of ITS scene only (Guide::obb / Guide::kind hold every scene's primitives, scene after scene) and loops over that scene's own
// count - no padding, so the first-index rule of a min_o tie is the scene's own - and reads its scene's start / goal pair; margin,
// smoothness, graw and rowsq are indexed by the global row.  Everything behind the staging is the row's own arithmetic, so a row of
// scene s computes what it computes on scene s's own guide.  One scene: rps = 0, slice 0 = the whole table.
//
// Self-clearance term (sdf_self_kernel, edmp_sdf_set_self): on the same sphere model and link-sorted table; the lane's joints, sphere
// centres, wave combine and rowsq are sdf_row's by the helpers below.  For an SDF row r at step t, over the sphere pairs (s, u) with
// mask[link_s][link_u], link_s < link_u:
//   d(w; s, u) = ||c_s(q_w) - c_u(q_w)|| - r_s - r_u
//   self(r)    = weight_r * sum_{w=1..L} sum_{(s,u)} max(0, m_r(t) - d(w; s, u))       m_r(t) = self_margin[r][t - 1] for t >= 1, 0 at t = 0
// Interior waypoints only: no start / goal pair and nothing of the scene, so the term is the same inside a scene batch.  The hinge is
// active iff m - d > 0 and a zero norm contributes a zero gradient, as above.  Gradient: with n = (c_s - c_u) / ||c_s - c_u||, a joint at
// or below link_s's frame moves both centres rigidly and n . (z_i x (c_s - c_u)) is identically zero; only the joints i with
// frame(link_s) < i <= frame(link_u) contribute, d d / d q_i = -n . (z_i x (c_u - o_i)), so d self / d q_i = weight * n . (z_i x (c_u - o_i))
// on an active pair.  sdf_self_kernel runs after sdf_guide_kernel over the rows whose weight is > 0, adds this to the row's graw and
// rewrites rowsq[r].  Every wave walks the whole chain (it needs every z_i, o_i of its lane), the link frames meet in LDS, pair p of
// the list (s ascending, then u) belongs to wave p % 4 and a wave adds its pairs in list order.
//
// Tool-pose goal term (sdf_goal_kernel, edmp_sdf_set_goal): the only term that looks at where the tool is.  For an SDF row r with
// goal_weight[r] > 0, over the interior waypoints w = 1..L, all arithmetic in f32:
//   (R_w | p_w) = T_7(q_w) * tool                   joint-7 frame of the chain times a 3 x 4 tool frame
//   e_pos(w)    = ||p_w - p*||^2
//   e_ori(w)    = 3 - tr(R*^T R_w)                  = 4 sin^2(theta_w / 2): smooth everywhere, no kink at 0 or pi
//   rho_r(w)    = max(0, w - L + K_r) / K_r         K_r = goal_window[r] >= 1: a linear ramp that is 1 at w = L
//   goal(r)     = goal_weight[r] * sum_w rho_r(w) * (e_pos(w) + goal_rotation[r] * e_ori(w))
// (R* | p*) is the target pose of the row's scene.  No dependence on t, none on the obstacles, no kink: nothing to keep inputs away from.
// Gradient: with c_k, c*_k the columns of R_w, R* and a_w = sum_k c*_k x c_k (d c_k / d q_i = z_i x c_k, so d e_ori / d q_i = z_i . a_w),
//   d goal / d q_{w,i} = weight * rho(w) * (2 (p_w - p*) . (z_i x (p_w - o_i)) + rotation * z_i . a_w)        all seven joints.
// sdf_goal_kernel runs after sdf_guide_kernel and sdf_self_kernel over the rows whose weight is > 0, adds this to the row's graw and
// rewrites rowsq[r].  One chain walk and seven dot products per waypoint: ONE wave per row, lane = padded waypoint as above, four rows to
// a 256-thread workgroup (row = rows[blockIdx.x * 4 + wave]); a wave past the list leaves as a whole.  No LDS, no barrier, no atomics.
//
// Swept-clearance term (sdf_sweep_kernel, edmp_sdf_set_sweep): the obstacle hinge at the configurations BETWEEN the waypoints that the
// success check tests (success.hip: substeps - 1 joint-space interpolants per segment), so that guide and check look at the same set.
// For an SDF row r with sweep_weight[r] > 0 and K = sweep_substeps[r], over the padded chain w = 0..L+1, all arithmetic in f32:
//   q(w, k)  = (1 - f) q_w + f q_{w+1}      f = k / K, w = 0..L, k = 1..K-1; q_w the clipped, f32-cast joints above, q_0 / q_{L+1} the
//                                           pinned start / goal
//   sweep(r) = sweep_weight[r] * sum_{w=0..L} sum_{k=1..K-1} sum_s max(0, m_r(t) - d(q(w, k), s))
// d, m_r(t) = the obstacle part's clearance and margin (sdf_margin), the same sphere table, staging and sub-gradient conventions.
// Gradient with respect to the interior waypoints only: an active hinge at q(w, k) sends (1 - f) J^T n to waypoint w and f J^T n to
// waypoint w + 1; what would land on start or goal is dropped.  sdf_sweep_kernel runs after the three kernels above over the rows whose
// weight is > 0, adds weight x this to the row's graw and rewrites rowsq[r].  Layout: the obstacle part's (one workgroup per row, the
// scene's own staging, four waves by link group) with lane = SEGMENT w holding q_w and q_{w+1} (one shuffle inside each wave).  Per k, in
// a loop that is not unrolled (K is workgroup-uniform and nothing of the kernel's resources depends on it): one chain walk up to the
// wave's last joint, the sphere loop of its links, and two sets of seven accumulators, (1 - f) x and f x.  Both sets meet in wave 0 as
// ((w0 + w1) + w2) + w3; lane w then takes its own first set plus lane w-1's second set by one __shfl_up.  No atomics, one order of every sum.
//
// Repair of finished rows (sdf_repair_kernel, edmp_sdf_repair_rows_dev / edmp_scenes_sdf_repair_rows_dev): projected descent on the swept
// cost of a row of the finished state X (., 7, N) f64, between the end of the loop and the selection.  No guide rows, no step t: the call
// brings the scalars margin m >= 0, smoothness lambda >= 0, substeps K in 1..EDMP_MAX_SWEEP_SUBSTEPS, iters n in 0..EDMP_MAX_REPAIR_ITERS,
// step eta > 0 and max_step delta > 0.  The interior columns 1..N-2 are the L = N - 2 waypoints, the scene's start / goal pair the ends.
// Evaluation E(x), all arithmetic in f32 in the statements above:
//   q_w      = (float) clip(x_w), w = 1..L (lane_joints with do_clip = 1); q_0, q_{L+1} = the f32 casts of start and goal
//   q(w, k)  = fmaf(f, q_{w+1}, (1 - f) q_w)      f = (float)k / (float)K, w = 0..L, k = 0..K-1, so q(w, 0) = q_w; the goal q_{L+1} joins the set
//   H        = sum max(0, m - d(c, s))            over every configuration c of the set except start and goal, and every sphere s:
//                                                 the obstacle part's hinge at margin m plus the sweep term at weight 1 and the same margin
//   S        = lambda * sum_{w=0..L} ||q_{w+1} - q_w||^2
//   g        = grad (H + S) with respect to the interior waypoints: an active hinge at q(w, k) sends (1 - f) J^T n to waypoint w and
//              f J^T n to waypoint w + 1; what would land on start or goal is dropped
//   cost     = H + S, the hinge terms summed in f64 per lane and wave in (k, link, sphere) order, waves as ((w0 + w1) + w2) + w3, plus the
//              lane's smoothness term, then wave_sum over the lanes;  clearance = min d over ALL configurations of the set, start and goal included
// Iteration: for i = 0, 1, ...: evaluate E(x_i); stop with iterations = i if no hinge term is active (H = 0) or i = n; otherwise every
// interior element moves in f64: delta = min(max(-eta * (double)g, -delta_max), delta_max), x <- min(max(x + delta, qlo_j), qhi_j).  Columns
// 0 and N-1 are never written; a row that is clear by m at every tested configuration keeps its bits (iterations = 0); iters = 0 is a pure
// report; at most n + 1 evaluations.  Per row: cost and clearance of evaluation 0 and of the last evaluation, and iterations.  A row with
// a non-finite element in its interior columns is not touched: iterations = -1, NaN reports.  Rows are independent: no whole-batch norm, no
// atomics, one order of every sum.  The self-clearance and goal terms are NOT part of the repaired cost: start and goal are pinned, and
// self_collision_rows stays the check for self-collision.  Layout: the sweep term's (one workgroup per listed row for the WHOLE run of the
// row, the scene staged once, lane = segment w, k loop from 0, two sets of seven accumulators); wave 0 keeps the row's f64 state, seven
// values per lane, applies the update and hands the new f32 joints and the stop decision to all four waves through LDS.
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "rowlist.h"  // check_rows: the row list of the repair calls

#include <algorithm>
#include <cmath>

namespace edmp {

// what every kernel here takes of a row: its L interior waypoints, its margin schedule and where its results go
struct RowView {
    const double* joints;  // element (r, j, wi) at joints[(r*7 + j)*ldw + off + wi], wi in 0..L-1
    int ldw, off;
    int L, t;
    int do_clip;           // clip to the joint limits in f64 before the f32 cast (diffusion.py:328), as guide_kernel
    const int32_t* rows;   // gradient: the rows of the batch that the kernel works on, one workgroup each
    const double* margin;  // [B][T]; read at t >= 1 only
    int T;
    float* graw;           // gradient: [B][7][L]
    double* rowsq;         // gradient: per-row sum g^2
    double* cost;          // rows: [n]
    double* clearance;     // rows: [n]
};

struct SdfArgs {
    RowView v;             // rows: the SDF rows; margin: sdf_margin
    const double* smooth;  // [B], or nullptr = 0 (edmp_sdf_rows_dev on rows that are not the bound ones)
    const double* obb;     // [sum of the scenes' obstacles][16] f64, scene after scene
    const int32_t* kind;   // [the same]
    int rps;               // scene batch: rows per scene (row r belongs to scene r / rps), else 0 = one scene
    int sc_off[EDMP_MAX_SCENES], sc_cnt[EDMP_MAX_SCENES];  // scene s owns the obstacle rows [sc_off[s], sc_off[s] + sc_cnt[s]) (SceneSlices, success.hip)
    const float* spheres;  // [ns][4] sorted by link
    int ns;
    int link_off[EDMP_N_LINKS + 1];  // spheres of link l: [link_off[l], link_off[l+1])
    const float* startgoal;          // [14] f32 (scene batch: [S][14])
};

// signed distance of the world point (cx, cy, cz) to the staged obstacle ob[16]; e[3] and the local point come back for the gradient
__device__ __forceinline__ float sdf_one(const float* ob, float cx, float cy, float cz, float p[3], float e[3]) {
    const float dx = cx - ob[9], dy = cy - ob[10], dz = cz - ob[11];
    p[0] = fmaf(ob[6], dz, fmaf(ob[3], dy, ob[0] * dx));
    p[1] = fmaf(ob[7], dz, fmaf(ob[4], dy, ob[1] * dx));
    p[2] = fmaf(ob[8], dz, fmaf(ob[5], dy, ob[2] * dx));
    if (ob[15] != 0.f) {  // cylinder (obstacle-uniform, so wave-uniform)
        const float rho = sqrtf(fmaf(p[1], p[1], p[0] * p[0]));
        e[0] = rho - ob[12];
        e[1] = fabsf(p[2]) - ob[14];
        e[2] = -3.0e38f;  // no third axis: never positive, never the maximum
    } else {
        e[0] = fabsf(p[0]) - ob[12];
        e[1] = fabsf(p[1]) - ob[13];
        e[2] = fabsf(p[2]) - ob[14];
    }
    const float m0 = fmaxf(e[0], 0.f), m1 = fmaxf(e[1], 0.f), m2 = fmaxf(e[2], 0.f);
    const float outside = sqrtf(fmaf(m2, m2, fmaf(m1, m1, m0 * m0)));
    const float inside = fminf(fmaxf(e[0], fmaxf(e[1], e[2])), 0.f);
    return outside + inside;
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// world gradient of sdf_one at the same point (the conventions of the header)
__device__ __forceinline__ void sdf_grad(const float* ob, float cx, float cy, float cz, float n[3]) {
    float p[3], e[3];
    (void)sdf_one(ob, cx, cy, cz, p, e);
    const float m0 = fmaxf(e[0], 0.f), m1 = fmaxf(e[1], 0.f), m2 = fmaxf(e[2], 0.f);
    const float outside = sqrtf(fmaf(m2, m2, fmaf(m1, m1, m0 * m0)));
    float a0, a1, a2;  // d sdf / d e_k
    if (outside > 0.f) {
        a0 = m0 / outside;
        a1 = m1 / outside;
        a2 = m2 / outside;
    } else {
        const bool k0 = e[0] >= e[1] && e[0] >= e[2];
        const bool k1 = !k0 && e[1] >= e[2];
        a0 = k0 ? 1.f : 0.f;
        a1 = k1 ? 1.f : 0.f;
        a2 = (!k0 && !k1) ? 1.f : 0.f;
    }
    float gl[3];
    if (ob[15] != 0.f) {
        const float rho = sqrtf(fmaf(p[1], p[1], p[0] * p[0]));
        const float ux = rho > 0.f ? p[0] / rho : 0.f, uy = rho > 0.f ? p[1] / rho : 0.f;
        gl[0] = a0 * ux;
        gl[1] = a0 * uy;
        gl[2] = a1 * sgn(p[2]);
    } else {
        gl[0] = a0 * sgn(p[0]);
        gl[1] = a1 * sgn(p[1]);
        gl[2] = a2 * sgn(p[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = fmaf(ob[i * 3 + 2], gl[2], fmaf(ob[i * 3 + 1], gl[1], ob[i * 3] * gl[0]));
}

// ---- what the obstacle part (sdf_row) and the self term (sdf_self_row) share: the lane's waypoint, its chain, the wave combine ------
// q = the joints of row r at padded waypoint w (0 and >= L+1 repeat the first / last interior waypoint), loaded as guide_kernel loads
// them: f64, clipped under do_clip, then f32
__device__ __forceinline__ void lane_joints(const RowView& v, const RobotConst& rc, int r, int w, float q[7]) {
    const int wi = min(max(w - 1, 0), v.L - 1);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double xd = v.joints[((size_t)r * 7 + j) * v.ldw + v.off + wi];
        if (v.do_clip) {
            xd = xd < rc.qlo[j] ? rc.qlo[j] : xd;
            xd = xd > rc.qhi[j] ? rc.qhi[j] : xd;
        }
        q[j] = (float)xd;
    }
}

__device__ __forceinline__ float row_margin(const RowView& v, int r) { return (v.t >= 1) ? (float)v.margin[(size_t)r * v.T + (v.t - 1)] : 0.f; }

// joint j of the lane's chain: (R | o) steps over it, zax[j] / org[j] take its axis and origin
__device__ __forceinline__ void joint_step(const RobotConst& rc, const float q[7], int j, float R[3][3], float o[3], float zax[7][3], float org[7][3]) {
    dh_step(R, o, sinf(q[j]), cosf(q[j]), rc.dh[j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        zax[j][i] = R[i][2];
        org[j][i] = o[i];
    }
}

// world centre of the sphere sp = centre | radius of the link whose frame is LR | Lo
__device__ __forceinline__ void sphere_world(const float LR[3][3], const float Lo[3], const float* sp, float c[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = fmaf(LR[i][2], sp[2], fmaf(LR[i][1], sp[1], LR[i][0] * sp[0])) + Lo[i];
}

// n . (z x (c - o)): what a unit turn of the joint with axis z through o moves the point c along n
__device__ __forceinline__ float screw_dot(const float n[3], const float z[3], const float o[3], const float c[3]) {
    const float rx = c[0] - o[0], ry = c[1] - o[1], rz = c[2] - o[2];
    const float kx = z[1] * rz - z[2] * ry;
    const float ky = z[2] * rx - z[0] * rz;
    const float kz = z[0] * ry - z[1] * rx;
    return fmaf(n[2], kz, fmaf(n[1], ky, n[0] * kx));
}

// The four waves' partials of a lane meet in wave 0 as ((w0 + w1) + w2) + w3: the seven gradient elements g, or (ROWS) the f32 minimum
// dmin and the f64 sum cacc.  Waves 1..3 leave theirs in s_g / s_c (ROWS: s_g[.][0] holds dmin); false: the wave is done.  NG = 14: the
// sweep term's two sets of seven
template <bool ROWS, int NG = 7>
__device__ __forceinline__ bool meet_in_wave0(float (*s_g)[NG][64], double (*s_c)[64], int wv, int lane, float g[NG], float& dmin, double& cacc) {
    if (wv > 0) {
        if (ROWS) {
            s_g[wv - 1][0][lane] = dmin;
            s_c[wv - 1][lane] = cacc;
        } else {
#pragma unroll
            for (int i = 0; i < NG; ++i) s_g[wv - 1][i][lane] = g[i];
        }
    }
    __syncthreads();
    if (wv > 0) return false;
    if (ROWS) {
        cacc = ((cacc + s_c[0][lane]) + s_c[1][lane]) + s_c[2][lane];
        dmin = fminf(fminf(fminf(dmin, s_g[0][0][lane]), s_g[1][0][lane]), s_g[2][0][lane]);
    } else {
#pragma unroll
        for (int i = 0; i < NG; ++i) g[i] = ((g[i] + s_g[0][i][lane]) + s_g[1][i][lane]) + s_g[2][i][lane];
    }
    return true;
}

// rowsq = the sum over the wave's lanes of the lane's seven final gradient elements squared
__device__ __forceinline__ void store_rowsq(const float g[7], int lane, double* rowsq) {
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) sq = fmaf(g[i], g[i], sq);
    const double tot = wave_sum((double)sq);
    if (lane == 0) *rowsq = tot;
}

// the report of a row: scale x the sum of the lanes' costs, and the smallest of their clearances
__device__ __forceinline__ void store_report(double cacc, float dmin, double scale, int lane, double* cost, double* clearance) {
    const double tot = wave_sum(cacc);
    dmin = wave_min(dmin);
    if (lane == 0) {
        *cost = scale * tot;
        *clearance = (double)dmin;
    }
}

// the workgroup's scene as the kernels read it: its no obstacles (f64 [16] rows, kinds) -> s_ob f32 [16], the sphere table -> s_sph.  All
// 256 threads; the caller's barrier follows
__device__ __forceinline__ void stage_scene(const double* obb, const int32_t* kind, int no, const float* spheres, int ns, float* s_ob, float* s_sph) {
    for (int i = threadIdx.x; i < no * 16; i += 256) {
        const int ob = i >> 4, k = i & 15;
        const bool cyl = kind[ob] == 1;
        const double v = obb[i];
        // a cylinder's (r, r, h) row is stored halved like a box: slot 12 becomes the radius
        s_ob[i] = (k == 15) ? (cyl ? 1.f : 0.f) : ((k == 12 && cyl) ? (float)(2.0 * v) : (float)v);
    }
    for (int i = threadIdx.x; i < ns * 4; i += 256) s_sph[i] = spheres[i];
}

// ROWS = false: the raw gradient of row a.v.rows[blockIdx.x] -> graw / rowsq (the contract of guide_kernel<GM_GRAD>).
// ROWS = true: cost and minimum clearance of row blockIdx.x.  Cost: per lane and wave the hinge terms in f64 in (link, sphere) order,
// the four waves' partials as ((w0 + w1) + w2) + w3, plus the lane's smoothness term, then wave_sum over the lanes.
template <bool ROWS>
__device__ __forceinline__ void sdf_row(const SdfArgs& a, const RobotConst& rc) {
    __shared__ float s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ float s_sph[EDMP_MAX_SPHERES * 4];
    __shared__ float s_g[3][7][64];  // partials of waves 1..3 (ROWS: [w][0] clearance)
    __shared__ double s_c[3][64];    // ROWS: cost partials of waves 1..3
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = ROWS ? (int)blockIdx.x : a.v.rows[blockIdx.x];
    const int scene = __builtin_amdgcn_readfirstlane(a.rps ? r / a.rps : 0);  // (one row, one scene: workgroup-uniform)
    const int L = a.v.L, no = min(a.sc_cnt[scene], EDMP_MAX_OBSTACLES);
    const double* obb = a.obb + (size_t)a.sc_off[scene] * 16;
    const int32_t* kind = a.kind + a.sc_off[scene];
    const float* sg = a.startgoal + scene * 14;  // this row's scene's start | goal
    stage_scene(obb, kind, no, a.spheres, a.ns, s_ob, s_sph);
    __syncthreads();

    const float m = row_margin(a.v, r);
    const float lam = a.smooth ? (float)a.smooth[r] : 0.f;

    // this lane's joint vector: padded waypoint w = lane (0 start, 1..L interior, >= L+1 goal)
    const int w = lane;
    float q[7];
    lane_joints(a.v, rc, r, w, q);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const float vs = sg[j], vg = sg[7 + j];
        q[j] = (w == 0) ? vs : ((w > L) ? vg : q[j]);
    }
    const bool interior = (w >= 1) && (w <= L);

    float g[7] = {0, 0, 0, 0, 0, 0, 0};
    double cacc = 0.0;
    float dmin = INFINITY;
    // the wave walks the chain up to its last link's joint (the loops stay here: as a walk that takes the sphere loop as its per-link
    // action, sdf_guide_kernel compiled to 155 VGPRs instead of 132)
    float R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    float o[3] = {0, 0, 0};
    float zax[7][3], org[7][3];
    const int my_jmax = wave_last_joint(wv);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        if (j > my_jmax) break;  // (wave-uniform)
        joint_step(rc, q, j, R, o, zax, org);
#pragma unroll
        for (int ll = 0; ll < 3; ++ll) {
            if (ll > 0 && j != 6) continue;
            const int l = (ll == 0) ? j : 6 + ll;  // hand and finger ride on joint 6
            if (link_wave(l) != wv) continue;      // another wave's link (wave-uniform)
            float LR[3][3], Lo[3];
            frame_apply(R, o, rc.sf[l], LR, Lo);
            const int s1 = a.link_off[l + 1];
            for (int s = a.link_off[l]; s < s1; ++s) {
                const float* sp = s_sph + s * 4;
                float c[3];
                sphere_world(LR, Lo, sp, c);
                float best = INFINITY;
                int bi = 0;
                for (int ob = 0; ob < no; ++ob) {
                    float p[3], e[3];
                    const float d = sdf_one(s_ob + ob * 16, c[0], c[1], c[2], p, e);
                    if (d < best) {
                        best = d;
                        bi = ob;
                    }
                }
                const float clr = best - sp[3];
                const float h = m - clr;
                if (ROWS) {
                    dmin = fminf(dmin, clr);
                    if (interior && h > 0.f) cacc += (double)h;
                } else if (interior && h > 0.f) {
                    float n[3];
                    sdf_grad(s_ob + bi * 16, c[0], c[1], c[2], n);
                    // d c / d q_i = z_i x (c - o_i), i <= j; the hinge turns the sign
#pragma unroll
                    for (int i = 0; i <= j; ++i) g[i] -= screw_dot(n, zax[i], org[i], c);
                }
            }
        }
    }

    if (!meet_in_wave0<ROWS>(s_g, s_c, wv, lane, g, dmin, cacc)) return;
    // wave 0 holds every joint of its lane's waypoint: the neighbours' joints come by two shuffles
    float qp[7], qn[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        qp[j] = __shfl_up(q[j], 1, 64);
        qn[j] = __shfl_down(q[j], 1, 64);
    }
    if (ROWS) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const float df = qn[j] - q[j];
            ss = fmaf(df, df, ss);
        }
        if (w <= L) cacc += (double)(lam * ss);  // segment (w, w+1)
        if (w > L + 1) dmin = INFINITY;          // lanes behind the goal repeat it
        store_report(cacc, dmin, 1.0, lane, a.v.cost + r, a.v.clearance + r);
    } else {
        const float l2 = 2.f * lam;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const float gi = fmaf(l2, fmaf(2.f, q[i], -qp[i]) - qn[i], g[i]);  // 2 lambda (2 q_w - q_{w-1} - q_{w+1})
            g[i] = interior ? gi : 0.f;
            if (interior) a.v.graw[((size_t)r * 7 + i) * L + (w - 1)] = gi;
        }
        store_rowsq(g, lane, a.v.rowsq + r);
    }
}

__global__ __launch_bounds__(256, 3) void sdf_guide_kernel(SdfArgs a, RobotConst rc) { sdf_row<false>(a, rc); }
__global__ __launch_bounds__(256, 4) void sdf_rows_kernel(SdfArgs a, RobotConst rc) { sdf_row<true>(a, rc); }

struct SelfArgs {
    RowView v;              // rows: the rows whose weight is > 0; margin: self_margin; graw: the row's SDF gradient on entry
    const double* weight;   // [B], or nullptr = 1 (edmp_sdf_self_rows_dev on rows that are not the bound ones)
    const float* spheres;   // [ns][4] sorted by link
    const int32_t* pairs;   // [np][4] = s, u, link_s, link_u
    int np;
};

// ROWS = false: add the self gradient of row a.v.rows[blockIdx.x] to graw and rewrite rowsq.  ROWS = true: weighted self cost and the
// minimum d over interior waypoints and listed pairs of row blockIdx.x (+inf without a pair).
template <bool ROWS>
__device__ __forceinline__ void sdf_self_row(const SelfArgs& a, const RobotConst& rc) {
    __shared__ float s_fr[EDMP_N_LINKS][12][64];  // link frames LR | Lo of every lane's waypoint, k = row * 4 + column
    __shared__ float s_g[3][7][64];               // partials of waves 1..3 (ROWS: [w][0] minimum d)
    __shared__ double s_c[3][64];                 // ROWS: cost partials of waves 1..3
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = ROWS ? (int)blockIdx.x : a.v.rows[blockIdx.x];
    const int L = a.v.L;
    const float m = row_margin(a.v, r);

    // lane = padded waypoint; the end lanes repeat an interior waypoint and are not counted
    const int w = lane;
    const bool interior = (w >= 1) && (w <= L);
    float q[7];
    lane_joints(a.v, rc, r, w, q);

    // every wave walks the whole chain (sdf_row's loops) and stages the frames of its own link group
    float R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    float o[3] = {0, 0, 0};
    float zax[7][3], org[7][3];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        joint_step(rc, q, j, R, o, zax, org);
#pragma unroll
        for (int ll = 0; ll < 3; ++ll) {
            if (ll > 0 && j != 6) continue;
            const int l = (ll == 0) ? j : 6 + ll;  // hand and finger ride on joint 6
            if (link_wave(l) != wv) continue;      // another wave's link (wave-uniform)
            float LR[3][3], Lo[3];
            frame_apply(R, o, rc.sf[l], LR, Lo);
#pragma unroll
            for (int k = 0; k < 12; ++k) s_fr[l][k][lane] = (k & 3) == 3 ? Lo[k >> 2] : LR[k >> 2][k & 3];
        }
    }
    __syncthreads();
    auto centre = [&](int l, const float* sp, float c[3]) {  // sphere_world on link l's staged frame
        float LR[3][3], Lo[3];
#pragma unroll
        for (int k = 0; k < 12; ++k) ((k & 3) == 3 ? Lo[k >> 2] : LR[k >> 2][k & 3]) = s_fr[l][k][lane];
        sphere_world(LR, Lo, sp, c);
    };

    float g[7] = {0, 0, 0, 0, 0, 0, 0};
    double cacc = 0.0;
    float dmin = INFINITY;
    for (int p = wv; p < a.np; p += 4) {  // (wave-uniform: the list entries come by scalar loads)
        const int s = a.pairs[p * 4], u = a.pairs[p * 4 + 1], ls = a.pairs[p * 4 + 2], lu = a.pairs[p * 4 + 3];
        const float* sps = a.spheres + s * 4;
        const float* spu = a.spheres + u * 4;
        float cs[3], cu[3];
        centre(ls, sps, cs);
        centre(lu, spu, cu);
        const float dx = cs[0] - cu[0], dy = cs[1] - cu[1], dz = cs[2] - cu[2];
        const float nrm = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        const float d = nrm - sps[3] - spu[3];
        const float h = m - d;
        if (ROWS) {
            dmin = fminf(dmin, d);
            if (interior && h > 0.f) cacc += (double)h;
        } else if (interior && h > 0.f && nrm > 0.f) {
            const float n[3] = {dx / nrm, dy / nrm, dz / nrm};
            const int fs = min(ls, 6), fu = min(lu, 6);  // joint frame of a link (hand and finger ride on joint 6)
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                if (i <= fs || i > fu) continue;  // (wave-uniform)
                g[i] += screw_dot(n, zax[i], org[i], cu);
            }
        }
    }

    if (!meet_in_wave0<ROWS>(s_g, s_c, wv, lane, g, dmin, cacc)) return;
    const double wt = a.weight ? a.weight[r] : 1.0;
    if (ROWS) {
        if (!interior) dmin = INFINITY;
        store_report(cacc, dmin, wt, lane, a.v.cost + r, a.v.clearance + r);
    } else {
        const float wf = (float)wt;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            float gi = 0.f;
            if (interior) {
                float* dst = a.v.graw + ((size_t)r * 7 + i) * L + (w - 1);
                gi = fmaf(wf, g[i], *dst);
                *dst = gi;
            }
            g[i] = gi;
        }
        store_rowsq(g, lane, a.v.rowsq + r);
    }
}

__global__ __launch_bounds__(256) void sdf_self_kernel(SelfArgs a, RobotConst rc) { sdf_self_row<false>(a, rc); }
__global__ __launch_bounds__(256) void sdf_self_rows_kernel(SelfArgs a, RobotConst rc) { sdf_self_row<true>(a, rc); }

struct GoalArgs {
    RowView v;               // rows: the rows whose weight is > 0; graw: what the kernels before left; cost: the report's first output
    int n;                   // rows that the launch covers (waves past it leave)
    const double* weight;    // [B], or nullptr = 1 (edmp_sdf_goal_rows_dev on rows that are not the bound ones)
    const double* rotation;  // [B], or nullptr = 1
    const int32_t* window;   // [B], or nullptr = L
    const float* target;     // [S][12] row-major (R* | p*) per scene
    int rps;                 // scene batch: rows per scene (row r reads scene r / rps's target), else 0 = one scene
    float tool[12];          // row-major (R | p) behind joint 7
    double* distance;        // rows: [n] ||p_L - p*||
    double* angle;           // rows: [n] rotation angle between R_L and R*
    double* min_distance;    // rows: [n] min_w ||p_w - p*||
};

// ROWS = false: add the goal gradient of row a.v.rows[idx] to graw and rewrite rowsq.  ROWS = true: weighted cost (lane terms summed in
// f64), distance and angle at the last handed column, smallest distance over the handed columns, of row idx.  idx = blockIdx.x * 4 + wave.
template <bool ROWS>
__device__ __forceinline__ void sdf_goal_row(const GoalArgs& a, const RobotConst& rc) {
    const int lane = threadIdx.x & 63;
    const int idx = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (idx >= a.n) return;  // (wave-uniform: the whole wave leaves; nothing below waits for another wave)
    const int r = ROWS ? idx : a.v.rows[idx];
    const int L = a.v.L;
    const float* tg = a.target + (a.rps ? r / a.rps : 0) * 12;
    const float wt = a.weight ? (float)a.weight[r] : 1.f;
    const float rot = a.rotation ? (float)a.rotation[r] : 1.f;
    const int K = a.window ? a.window[r] : L;

    // lane = padded waypoint; the end lanes repeat an interior waypoint and are not counted
    const int w = lane;
    const bool interior = (w >= 1) && (w <= L);
    float q[7];
    lane_joints(a.v, rc, r, w, q);
    float R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    float o[3] = {0, 0, 0};
    float zax[7][3], org[7][3];
#pragma unroll
    for (int j = 0; j < 7; ++j) joint_step(rc, q, j, R, o, zax, org);
    float TR[3][3], p[3];
    frame_apply(R, o, a.tool, TR, p);

    const float dp[3] = {p[0] - tg[3], p[1] - tg[7], p[2] - tg[11]};
    const float epos = fmaf(dp[2], dp[2], fmaf(dp[1], dp[1], dp[0] * dp[0]));
    // tr(R*^T R_w) = sum_k c*_k . c_k and a_w = sum_k c*_k x c_k, k in column order
    float tr = 0.f, av[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sx = tg[k], sy = tg[4 + k], sz = tg[8 + k];
        const float cx = TR[0][k], cy = TR[1][k], cz = TR[2][k];
        tr += fmaf(sz, cz, fmaf(sy, cy, sx * cx));
        av[0] += sy * cz - sz * cy;
        av[1] += sz * cx - sx * cz;
        av[2] += sx * cy - sy * cx;
    }
    const float rho = (float)max(0, w - L + K) / (float)K;

    if (ROWS) {
        const float dist = sqrtf(epos);
        const double term = interior ? (double)(rho * fmaf(rot, 3.f - tr, epos)) : 0.0;
        const double tot = wave_sum(term);
        const float dmin = wave_min(interior ? dist : INFINITY);
        const float an = sqrtf(fmaf(av[2], av[2], fmaf(av[1], av[1], av[0] * av[0])));
        const float ang = atan2f(0.5f * an, 0.5f * (tr - 1.f));  // the form of ik.hip: exact near 0 and near pi
        if (lane == L) {  // the last handed column
            a.v.cost[r] = (double)wt * tot;
            a.distance[r] = (double)dist;
            a.angle[r] = (double)ang;
            a.min_distance[r] = (double)dmin;
        }
    } else {
        const float cf = wt * rho;
        const float dp2[3] = {2.f * dp[0], 2.f * dp[1], 2.f * dp[2]};
        float g[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const float za = fmaf(zax[i][2], av[2], fmaf(zax[i][1], av[1], zax[i][0] * av[0]));
            const float term = fmaf(rot, za, screw_dot(dp2, zax[i], org[i], p));
            float gi = 0.f;
            if (interior) {
                float* dst = a.v.graw + ((size_t)r * 7 + i) * L + (w - 1);
                gi = fmaf(cf, term, *dst);
                *dst = gi;
            }
            g[i] = gi;
        }
        store_rowsq(g, lane, a.v.rowsq + r);
    }
}

__global__ __launch_bounds__(256) void sdf_goal_kernel(GoalArgs a, RobotConst rc) { sdf_goal_row<false>(a, rc); }
__global__ __launch_bounds__(256) void sdf_goal_rows_kernel(GoalArgs a, RobotConst rc) { sdf_goal_row<true>(a, rc); }

struct SweepArgs {
    SdfArgs s;               // the obstacle part's arguments; v.rows: the rows whose weight is > 0; v.graw: what the kernels before left
    const double* weight;    // [B], or nullptr = 1 (the report on rows that are not the bound ones)
    const int32_t* substeps; // [B], or nullptr = K for every row
    int K;
};

// ROWS = false: add the sweep gradient of row a.s.v.rows[blockIdx.x] to graw and rewrite rowsq.  ROWS = true: weighted sweep cost (the
// hinge terms in f64 in (k, link, sphere) order per lane and wave, waves as ((w0 + w1) + w2) + w3, wave_sum over the lanes) and the
// minimum clearance over the interpolants of all L + 1 segments (+inf without one) of row blockIdx.x.
template <bool ROWS>
__device__ __forceinline__ void sdf_sweep_row(const SweepArgs& sa, const RobotConst& rc) {
    constexpr int NG = ROWS ? 1 : 14;
    __shared__ float s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ float s_sph[EDMP_MAX_SPHERES * 4];
    __shared__ float s_g[3][NG][64];  // partials of waves 1..3: [0..6] the (1 - f) set, [7..13] the f set (ROWS: [w][0] clearance)
    __shared__ double s_c[3][64];     // ROWS: cost partials of waves 1..3
    const SdfArgs& a = sa.s;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = __builtin_amdgcn_readfirstlane(ROWS ? (int)blockIdx.x : a.v.rows[blockIdx.x]);
    const int scene = __builtin_amdgcn_readfirstlane(a.rps ? r / a.rps : 0);  // (one row, one scene: workgroup-uniform)
    const int L = a.v.L, no = min(a.sc_cnt[scene], EDMP_MAX_OBSTACLES);
    const float* sg = a.startgoal + scene * 14;  // this row's scene's start | goal
    stage_scene(a.obb + (size_t)a.sc_off[scene] * 16, a.kind + a.sc_off[scene], no, a.spheres, a.ns, s_ob, s_sph);
    __syncthreads();

    const float m = row_margin(a.v, r);
    const int K = __builtin_amdgcn_readfirstlane(sa.substeps ? sa.substeps[r] : sa.K);  // (a workgroup is one row: a scalar)

    // lane = segment w = (padded waypoint w, padded waypoint w + 1); the neighbour's joints come by one shuffle
    const int w = lane;
    float q0[7], q1[7];
    lane_joints(a.v, rc, r, w, q0);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const float vs = sg[j], vg = sg[7 + j];
        q0[j] = (w == 0) ? vs : ((w > L) ? vg : q0[j]);
        q1[j] = __shfl_down(q0[j], 1, 64);
    }
    const bool segment = w <= L;  // (L <= 62: lane w + 1 exists)

    float g[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.f;
    double cacc = 0.0;
    float dmin = INFINITY;
    const int my_jmax = wave_last_joint(wv);
#pragma unroll 1
    for (int k = 1; k < K; ++k) {
        const float f = (float)k / (float)K, f1 = 1.f - f;
        float q[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) q[j] = fmaf(f, q1[j], f1 * q0[j]);
        // sdf_row's walk at the interpolant
        float R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        float o[3] = {0, 0, 0};
        float zax[7][3], org[7][3];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if (j > my_jmax) break;  // (wave-uniform)
            joint_step(rc, q, j, R, o, zax, org);
#pragma unroll
            for (int ll = 0; ll < 3; ++ll) {
                if (ll > 0 && j != 6) continue;
                const int l = (ll == 0) ? j : 6 + ll;  // hand and finger ride on joint 6
                if (link_wave(l) != wv) continue;      // another wave's link (wave-uniform)
                float LR[3][3], Lo[3];
                frame_apply(R, o, rc.sf[l], LR, Lo);
                const int s1 = a.link_off[l + 1];
                for (int s = a.link_off[l]; s < s1; ++s) {
                    const float* sp = s_sph + s * 4;
                    float c[3];
                    sphere_world(LR, Lo, sp, c);
                    float best = INFINITY;
                    int bi = 0;
                    for (int ob = 0; ob < no; ++ob) {
                        float p[3], e[3];
                        const float d = sdf_one(s_ob + ob * 16, c[0], c[1], c[2], p, e);
                        if (d < best) {
                            best = d;
                            bi = ob;
                        }
                    }
                    const float clr = best - sp[3];
                    const float h = m - clr;
                    if constexpr (ROWS) {
                        dmin = fminf(dmin, clr);
                        if (segment && h > 0.f) cacc += (double)h;
                    } else if (segment && h > 0.f) {
                        float n[3];
                        sdf_grad(s_ob + bi * 16, c[0], c[1], c[2], n);
#pragma unroll
                        for (int i = 0; i <= j; ++i) {
                            const float jn = screw_dot(n, zax[i], org[i], c);  // the hinge turns the sign
                            g[i] = fmaf(-f1, jn, g[i]);
                            g[7 + i] = fmaf(-f, jn, g[7 + i]);
                        }
                    }
                }
            }
        }
    }

    if (!meet_in_wave0<ROWS, NG>(s_g, s_c, wv, lane, g, dmin, cacc)) return;
    const double wt = sa.weight ? sa.weight[r] : 1.0;
    if constexpr (ROWS) {
        if (!segment) dmin = INFINITY;  // lanes behind the last segment repeat the goal
        store_report(cacc, dmin, wt, lane, a.v.cost + r, a.v.clearance + r);
    } else {
        const float wf = (float)wt;
        const bool interior = (w >= 1) && (w <= L);
        float gf[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const float prev = __shfl_up(g[7 + i], 1, 64);  // segment w - 1 ends at waypoint w
            float gi = 0.f;
            if (interior) {
                float* dst = a.v.graw + ((size_t)r * 7 + i) * L + (w - 1);
                gi = fmaf(wf, g[i] + prev, *dst);
                *dst = gi;
            }
            gf[i] = gi;
        }
        store_rowsq(gf, lane, a.v.rowsq + r);
    }
}

__global__ __launch_bounds__(256, 2) void sdf_sweep_kernel(SweepArgs a, RobotConst rc) { sdf_sweep_row<false>(a, rc); }
__global__ __launch_bounds__(256, 5) void sdf_sweep_rows_kernel(SweepArgs a, RobotConst rc) { sdf_sweep_row<true>(a, rc); }

struct RepairArgs {
    SdfArgs s;            // v.joints = X with ldw = N, off = 1, L = N - 2, do_clip = 1; v.rows: the listed rows, or nullptr = every row;
                          // startgoal: the call's own block; no margin schedule, no smoothness array
    double* X;            // (n, 7, N) f64, updated in place
    int K, iters;
    float margin, smooth;
    double step, max_step;
    double* cost;         // (n, 2): evaluation 0 | the last evaluation
    double* clearance;    // (n, 2)
    int32_t* iterations;  // (n,)
};

// The whole run of one listed row (the definition: "Repair of finished rows" in the header).  sdf_sweep_row's walk with k from 0; both
// accumulator sets, the f64 hinge sums and the clearances meet in wave 0, which owns the f64 state and the update.
__global__ __launch_bounds__(256, 2) void sdf_repair_kernel(RepairArgs ra, RobotConst rc) {
    __shared__ float s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ float s_sph[EDMP_MAX_SPHERES * 4];
    __shared__ float s_g[3][14][64];  // partials of waves 1..3: [0..6] the (1 - f) set, [7..13] the f set
    __shared__ double s_c[3][64];     // hinge sums of waves 1..3
    __shared__ float s_d[3][64];      // clearances of waves 1..3
    __shared__ float s_q[7][64];      // the padded chain's f32 joints, lane = padded waypoint: wave 0 writes, every wave reads
    __shared__ int s_stop;            // wave 0's decision: -1 a non-finite row, 1 the run is over, 0 another trip
    const SdfArgs& a = ra.s;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = __builtin_amdgcn_readfirstlane(a.v.rows ? a.v.rows[blockIdx.x] : (int)blockIdx.x);
    const int scene = __builtin_amdgcn_readfirstlane(a.rps ? r / a.rps : 0);  // (one row, one scene: workgroup-uniform)
    const int L = a.v.L, N = a.v.ldw, no = min(a.sc_cnt[scene], EDMP_MAX_OBSTACLES);
    const int K = __builtin_amdgcn_readfirstlane(ra.K), iters = __builtin_amdgcn_readfirstlane(ra.iters);
    const float* sg = a.startgoal + scene * 14;  // this row's scene's start | goal
    stage_scene(a.obb + (size_t)a.sc_off[scene] * 16, a.kind + a.sc_off[scene], no, a.spheres, a.ns, s_ob, s_sph);

    // lane = segment w = (padded waypoint w, padded waypoint w + 1); wave 0 holds the f64 element j of interior waypoint w in x[j]
    const int w = lane;
    const bool interior = (w >= 1) && (w <= L);
    const bool segment = w <= L;  // (L <= 62: lane w + 1 exists)
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    if (wv == 0) {
        float q[7];
        lane_joints(a.v, rc, r, w, q);
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            x[j] = a.v.joints[((size_t)r * 7 + j) * N + a.v.off + min(max(w - 1, 0), L - 1)];  // the element lane_joints clipped and cast
            bad = bad || (interior && !__builtin_isfinite(x[j]));
            s_q[j][lane] = (w == 0) ? sg[j] : ((w > L) ? sg[7 + j] : q[j]);
        }
        const int any_bad = __any(bad ? 1 : 0);
        if (lane == 0) s_stop = any_bad ? -1 : 0;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_stop) < 0) {  // (one LDS value behind a barrier: the whole workgroup leaves)
        if (threadIdx.x == 0) {
            ra.cost[(size_t)r * 2] = ra.cost[(size_t)r * 2 + 1] = NAN;
            ra.clearance[(size_t)r * 2] = ra.clearance[(size_t)r * 2 + 1] = NAN;
            ra.iterations[r] = -1;
        }
        return;
    }

    const float m = ra.margin, lam = ra.smooth;
    const int my_jmax = wave_last_joint(wv);
    double cost_last = 0.0;
    float clr_last = INFINITY;
    int it = 0;
    // Barrier uniformity: every trip holds two barriers (meet_in_wave0's and the one behind the update), so all four waves must take the
    // same number of trips.  The only way out is s_stop, ONE LDS value that wave 0 writes between the two barriers and all 256 threads
    // read behind the second; meet_in_wave0's `false` does not let waves 1..3 leave, and nothing per-wave or per-lane (an active hinge
    // of the own link group, the lane's own gradient) may decide.  A workgroup that diverges here hangs.
    for (;;) {
        float q0[7], q1[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            q0[j] = s_q[j][lane];
            q1[j] = __shfl_down(q0[j], 1, 64);
        }
        float g[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) g[i] = 0.f;
        double cacc = 0.0;
        float dmin = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float f = (float)k / (float)K, f1 = 1.f - f;
            const bool hinge = (k == 0) ? interior : segment;           // every configuration except start and goal
            const bool counted = segment || (k == 0 && w == L + 1);     // the clearance sees start and goal too
            float q[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) q[j] = fmaf(f, q1[j], f1 * q0[j]);
            // sdf_row's walk at the configuration
            float R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
            float o[3] = {0, 0, 0};
            float zax[7][3], org[7][3];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                if (j > my_jmax) break;  // (wave-uniform)
                joint_step(rc, q, j, R, o, zax, org);
#pragma unroll
                for (int ll = 0; ll < 3; ++ll) {
                    if (ll > 0 && j != 6) continue;
                    const int l = (ll == 0) ? j : 6 + ll;  // hand and finger ride on joint 6
                    if (link_wave(l) != wv) continue;      // another wave's link (wave-uniform)
                    float LR[3][3], Lo[3];
                    frame_apply(R, o, rc.sf[l], LR, Lo);
                    const int s1 = a.link_off[l + 1];
                    for (int s = a.link_off[l]; s < s1; ++s) {
                        const float* sp = s_sph + s * 4;
                        float c[3];
                        sphere_world(LR, Lo, sp, c);
                        float best = INFINITY;
                        int bi = 0;
                        for (int ob = 0; ob < no; ++ob) {
                            float p[3], e[3];
                            const float d = sdf_one(s_ob + ob * 16, c[0], c[1], c[2], p, e);
                            if (d < best) {
                                best = d;
                                bi = ob;
                            }
                        }
                        const float clr = best - sp[3];
                        const float h = m - clr;
                        if (counted) dmin = fminf(dmin, clr);
                        if (hinge && h > 0.f) {
                            cacc += (double)h;
                            float n[3];
                            sdf_grad(s_ob + bi * 16, c[0], c[1], c[2], n);
#pragma unroll
                            for (int i = 0; i <= j; ++i) {
                                const float jn = screw_dot(n, zax[i], org[i], c);  // the hinge turns the sign
                                g[i] = fmaf(-f1, jn, g[i]);
                                g[7 + i] = fmaf(-f, jn, g[7 + i]);
                            }
                        }
                    }
                }
            }
        }

        if (wv > 0) {
            s_c[wv - 1][lane] = cacc;
            s_d[wv - 1][lane] = dmin;
        }
        if (meet_in_wave0<false, 14>(s_g, s_c, wv, lane, g, dmin, cacc)) {  // (waves 1..3 go on to the barrier below)
            cacc = ((cacc + s_c[0][lane]) + s_c[1][lane]) + s_c[2][lane];
            dmin = fminf(fminf(fminf(dmin, s_d[0][lane]), s_d[1][lane]), s_d[2][lane]);
            const bool active = __any(cacc > 0.0 ? 1 : 0) != 0;  // H > 0: some hinge term of the row is active
            const bool stop = !active || it == iters;            // (wave-uniform)
            float qp[7], ss = 0.f;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                qp[j] = __shfl_up(q0[j], 1, 64);
                const float df = q1[j] - q0[j];
                ss = fmaf(df, df, ss);
            }
            if (segment) cacc += (double)(lam * ss);  // segment (w, w+1), as sdf_row adds it
            cost_last = wave_sum(cacc);
            clr_last = wave_min(dmin);
            if (it == 0 && lane == 0) {
                ra.cost[(size_t)r * 2] = cost_last;
                ra.clearance[(size_t)r * 2] = (double)clr_last;
            }
            const float l2 = 2.f * lam;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const float prev = __shfl_up(g[7 + i], 1, 64);  // segment w - 1 ends at waypoint w
                const float gi = fmaf(l2, fmaf(2.f, q0[i], -qp[i]) - q1[i], g[i] + prev);  // + 2 lambda (2 q_w - q_{w-1} - q_{w+1})
                if (!stop && interior) {
                    const double dx = fmin(fmax(-ra.step * (double)gi, -ra.max_step), ra.max_step);
                    x[i] = fmin(fmax(x[i] + dx, rc.qlo[i]), rc.qhi[i]);
                    s_q[i][lane] = (float)x[i];  // (inside the limits: the clip of lane_joints changes nothing)
                }
            }
            if (lane == 0) s_stop = stop ? 1 : 0;
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(s_stop)) break;  // the same value for all 256 threads
        ++it;
    }

    if (wv == 0) {  // it = the updates that were applied
        if (it > 0 && interior) {
#pragma unroll
            for (int j = 0; j < 7; ++j) ra.X[((size_t)r * 7 + j) * N + w] = x[j];
        }
        if (lane == 0) {
            ra.cost[(size_t)r * 2 + 1] = cost_last;
            ra.clearance[(size_t)r * 2 + 1] = (double)clr_last;
            ra.iterations[r] = it;
        }
    }
}

static RowView row_view(const Guide* g, const double* joints, int ldw, int off, int L, int t, int do_clip, const int32_t* rows, const double* margin) {
    return RowView{joints, ldw, off, L, t, do_clip, rows, margin, g->rows_T, g->graw, g->rowsq, nullptr, nullptr};
}

static void fill_self_args(const Guide* g, SelfArgs& a, const double* joints, int ldw, int off, int L, int t, int do_clip) {
    const SelfTerm& s = g->sdf.self;
    a = SelfArgs{row_view(g, joints, ldw, off, L, t, do_clip, s.rows, s.margin), s.weight, g->sdf.sph, s.pairs, s.np};
}

static void fill_goal_args(const Guide* g, GoalArgs& a, const double* joints, int ldw, int off, int L, int t, int do_clip) {
    const GoalTerm& gt = g->sdf.goal;
    a.v = row_view(g, joints, ldw, off, L, t, do_clip, gt.rows, nullptr);  // (no margin schedule: the term does not depend on t)
    a.n = gt.n;
    a.weight = gt.weight;
    a.rotation = gt.rotation;
    a.window = gt.window;
    a.target = gt.target;
    a.rps = g->is_batch ? g->rps : 0;
    for (int k = 0; k < 12; ++k) a.tool[k] = (float)gt.tool[k];
    a.distance = a.angle = a.min_distance = nullptr;
}

static void fill_args(const Guide* g, SdfArgs& a, const double* joints, int ldw, int off, int L, int t, int do_clip) {
    a.v = row_view(g, joints, ldw, off, L, t, do_clip, g->sdf.rows, g->sdf.margin);
    a.smooth = g->sdf.smooth;
    a.obb = g->obb;
    a.kind = g->kind;
    a.rps = (g->S > 1) ? g->rps : 0;
    for (int s = 0; s < EDMP_MAX_SCENES; ++s) {
        a.sc_off[s] = s < g->S ? g->scene_off_h[s] : 0;
        a.sc_cnt[s] = s < g->S ? g->scene_no_h[s] : 0;
    }
    a.spheres = g->sdf.sph;
    a.ns = g->sdf.ns;
    for (int l = 0; l <= EDMP_N_LINKS; ++l) a.link_off[l] = g->sdf.link_off[l];
    a.startgoal = g->startgoal;
}

static void fill_sweep_args(const Guide* g, SweepArgs& a, const double* joints, int ldw, int off, int L, int t, int do_clip) {
    const SweepTerm& sw = g->sdf.sweep;
    fill_args(g, a.s, joints, ldw, off, L, t, do_clip);  // (margin: the rows' own sdf_margin)
    a.s.v.rows = sw.rows;
    a.s.smooth = nullptr;
    a.weight = sw.weight;
    a.substeps = sw.substeps;
    a.K = 0;
}

// guide.hip's gradient paths, after guide_kernel<GM_GRAD> and before the rowsq reduction: the SDF rows' graw / rowsq are overwritten
int sdf_overlay(edmp_ctx* ctx, const double* joints, int ldw, int off, int L, int t, int do_clip) {
    Guide* g = ctx->guide;
    if (!g || g->sdf.n == 0) return EDMP_OK;
    SdfArgs a;
    fill_args(g, a, joints, ldw, off, L, t, do_clip);
    hipLaunchKernelGGL(sdf_guide_kernel, dim3(g->sdf.n), dim3(256), 0, ctx->stream, a, g->rc);
    EDMP_HIP_CHECK(hipGetLastError());
    if (g->sdf.self.n > 0 && g->sdf.self.np > 0) {  // the self term of the weighted rows, on top of what sdf_guide_kernel left
        SelfArgs sa;
        fill_self_args(g, sa, joints, ldw, off, L, t, do_clip);
        hipLaunchKernelGGL(sdf_self_kernel, dim3(g->sdf.self.n), dim3(256), 0, ctx->stream, sa, g->rc);
        EDMP_HIP_CHECK(hipGetLastError());
    }
    if (g->sdf.goal.n > 0) {  // the goal term of the weighted rows, on top of both: one wave per row, four rows per workgroup
        if (!g->sdf.goal.have_target) {  // (every gradient path hands its pair over first)
            set_error("the goal term's targets are derived from the goal configurations and no start / goal pair has been handed over");
            return EDMP_ERR_STATE;
        }
        GoalArgs ga;
        fill_goal_args(g, ga, joints, ldw, off, L, t, do_clip);
        hipLaunchKernelGGL(sdf_goal_kernel, dim3((ga.n + 3) / 4), dim3(256), 0, ctx->stream, ga, g->rc);
        EDMP_HIP_CHECK(hipGetLastError());
    }
    if (g->sdf.sweep.n > 0) {  // the swept-clearance term of the weighted rows, on top of all three: one workgroup per row
        SweepArgs wa;
        fill_sweep_args(g, wa, joints, ldw, off, L, t, do_clip);
        hipLaunchKernelGGL(sdf_sweep_kernel, dim3(g->sdf.sweep.n), dim3(256), 0, ctx->stream, wa, g->rc);
        EDMP_HIP_CHECK(hipGetLastError());
    }
    return EDMP_OK;
}

// row b as a message names it; rps > 0 (a scene batch): the rows run scene after scene, named by the scene and the row inside it
static const char* row_name(char (&buf)[48], int b, int rps) {
    if (rps) snprintf(buf, sizeof(buf), "scene %d, row %d", b / rps, b % rps);
    else snprintf(buf, sizeof(buf), "row %d", b);
    return buf;
}

// a [n][T] schedule of margins (name: what the message calls a value) is finite and >= 0
static int check_schedule(const char* what, const char* name, const double* v, int n, int T, int rps) {
    char where[48];
    for (size_t i = 0; i < (size_t)n * T; ++i)
        EDMP_REQUIRE(std::isfinite(v[i]) && v[i] >= 0.0, "%s: %s, step %d: %s %g must be finite and >= 0", what, row_name(where, (int)(i / T), rps),
                     (int)(i % T), name, v[i]);
    return EDMP_OK;
}

// Replace device arrays of the bound guide: *slot <- a block of max(bytes, min_bytes) holding the bytes at host.  drop() runs once
// nothing enqueued reads the old arrays and before they go: it takes out of sight what the arrays back (the caller makes the new
// ones visible after the call, when everything succeeded)
struct Upload { void** slot; const void* host; size_t bytes, min_bytes; };
template <class Drop>
static int guide_upload(edmp_ctx* ctx, Drop drop, std::initializer_list<Upload> ups) {
    ctx->epoch++;  // a captured whole-run graph holds the launch sequence of the old arrays
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // nothing enqueued still reads the arrays that are replaced
    drop();
    for (const Upload& u : ups) {
        ctx_release(ctx, *u.slot);
        *u.slot = nullptr;
    }
    for (const Upload& u : ups)
        if (int rc = ctx_alloc(ctx, u.slot, std::max(u.bytes, u.min_bytes))) return rc;
    hipError_t e = hipSuccess;
    for (const Upload& u : ups)
        if (e == hipSuccess && u.bytes) e = hipMemcpyAsync(*u.slot, u.host, u.bytes, hipMemcpyHostToDevice, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);  // the host vectors and the caller's arrays may go away after the call
    EDMP_HIP_CHECK(e);
    EDMP_HIP_CHECK(e2);
    return EDMP_OK;
}

// the start / goal uploads of guide.hip call this (guide.h): derived targets (R* | p*) = T_7(goal_s) . tool, the host side of chain.h in f64
int guide_goal_targets(edmp_ctx* ctx, int S, const double* goals) {
    GoalTerm& gt = ctx->guide->sdf.goal;
    if (!gt.set || !gt.derived) return EDMP_OK;
    double dh[7][4];
    joint_dh64(nullptr, dh);
    for (int s = 0; s < S; ++s) {
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, o[3] = {0, 0, 0}, TR[3][3], p[3];
        for (int j = 0; j < 7; ++j) dh_step(R, o, std::sin(goals[s * 7 + j]), std::cos(goals[s * 7 + j]), dh[j]);
        frame_apply(R, o, gt.tool, TR, p);
        for (int i = 0; i < 3; ++i) {
            for (int c = 0; c < 3; ++c) gt.target_h[s * 12 + i * 4 + c] = (float)TR[i][c];
            gt.target_h[s * 12 + i * 4 + 3] = (float)p[i];
        }
    }
    EDMP_HIP_CHECK(hipMemcpyAsync(gt.target, gt.target_h, (size_t)S * 12 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    gt.have_target = true;
    return EDMP_OK;
}

}  // namespace edmp

using namespace edmp;

// edmp_sdf_set and edmp_scene_batch_set_sdf behind their own state checks: value checks, link sort, upload.  rps > 0 (a scene batch):
// the n rows run scene after scene and a message names the scene and the row inside it.
static int sdf_table_set(edmp_ctx* ctx, const char* what, const float* spheres, int n_spheres, const int32_t* sdf_row, const double* margin,
                         const double* smoothness, int n, int T, int rps) {
    SdfTable& tb = ctx->guide->sdf;
    EDMP_REQUIRE(spheres && sdf_row && margin && smoothness, "%s: null argument", what);
    EDMP_REQUIRE(n_spheres >= 1 && n_spheres <= EDMP_MAX_SPHERES, "%s: %d spheres outside 1..%d", what, n_spheres, EDMP_MAX_SPHERES);
    for (int s = 0; s < n_spheres; ++s) {
        const float* sp = spheres + s * 5;
        EDMP_REQUIRE(std::isfinite(sp[0]) && std::isfinite(sp[1]) && std::isfinite(sp[2]) && std::isfinite(sp[3]) && std::isfinite(sp[4]),
                     "%s: sphere %d holds a non-finite value", what, s);
        EDMP_REQUIRE(sp[0] == std::floor(sp[0]) && sp[0] >= 0.f && sp[0] < (float)EDMP_N_LINKS, "%s: sphere %d: link %g outside 0..%d", what, s,
                     (double)sp[0], EDMP_N_LINKS - 1);
        EDMP_REQUIRE(sp[4] > 0.f, "%s: sphere %d: radius %g must be > 0", what, s, (double)sp[4]);
    }
    char where[48];
    std::vector<int32_t> rows;
    for (int b = 0; b < n; ++b) {
        EDMP_REQUIRE(sdf_row[b] == 0 || sdf_row[b] == 1, "%s: %s: sdf_row must be 0 or 1", what, row_name(where, b, rps));
        EDMP_REQUIRE(std::isfinite(smoothness[b]) && smoothness[b] >= 0.0, "%s: %s: smoothness %g must be finite and >= 0", what, row_name(where, b, rps),
                     smoothness[b]);
        if (sdf_row[b]) rows.push_back(b);
    }
    if (int rc = check_schedule(what, "margin", margin, n, T, rps)) return rc;
    // the table sorted by link, table order kept inside a link: the kernel's wave of a link group walks one contiguous range
    std::vector<float> sph((size_t)n_spheres * 4);
    int k = 0;
    for (int l = 0; l < EDMP_N_LINKS; ++l) {
        tb.link_off[l] = k;
        for (int s = 0; s < n_spheres; ++s)
            if ((int)spheres[s * 5] == l) {
                for (int c = 0; c < 4; ++c) sph[(size_t)k * 4 + c] = spheres[s * 5 + 1 + c];
                ++k;
            }
    }
    tb.link_off[EDMP_N_LINKS] = k;
    if (int rc = guide_upload(ctx, [&] { tb.drop(); },  // (the self term belongs to this table: a new table drops it)
                              {{(void**)&tb.sph, sph.data(), sph.size() * sizeof(float), 0},
                               {(void**)&tb.rows, rows.data(), rows.size() * sizeof(int32_t), sizeof(int32_t)},
                               {(void**)&tb.margin, margin, (size_t)n * T * sizeof(double), 0},
                               {(void**)&tb.smooth, smoothness, (size_t)n * sizeof(double), 0}}))
        return rc;
    tb.row_h.assign(sdf_row, sdf_row + n);
    tb.ns = n_spheres;
    tb.n = (int)rows.size();
    return EDMP_OK;
}

extern "C" int edmp_sdf_set(edmp_ctx* ctx, const float* spheres, int n_spheres, const int32_t* sdf_row, const double* margin, const double* smoothness,
                            int B, int T) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->row_class, "edmp_sdf_set: call edmp_scene_set and edmp_rows_set first");
    Guide* g = ctx->guide;
    if (g->is_batch || g->S > 1) {
        set_error("edmp_sdf_set: the bound guide is a scene batch of %d scenes (edmp_scene_batch_set); a scene batch takes its table from edmp_scene_batch_set_sdf",
                  g->S);
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(B == g->B && T == g->rows_T, "edmp_sdf_set: %d rows x %d steps given, edmp_rows_set holds %d x %d", B, T, g->B, g->rows_T);
    return sdf_table_set(ctx, "edmp_sdf_set", spheres, n_spheres, sdf_row, margin, smoothness, B, T, 0);
}

extern "C" int edmp_scene_batch_set_sdf(edmp_ctx* ctx, const float* spheres, int n_spheres, const int32_t* sdf_row, const double* margin,
                                        const double* smoothness, int S, int B, int T) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scene_batch_set_sdf");
    Guide* g = ctx->guide;
    EDMP_REQUIRE(T == g->rows_T, "edmp_scene_batch_set_sdf: %d steps given, edmp_rows_set holds %d", T, g->rows_T);
    return sdf_table_set(ctx, "edmp_scene_batch_set_sdf", spheres, n_spheres, sdf_row, margin, smoothness, S * B, T, B);
}

// the step and row count of a report call: any n rows at t = 0, the bound rows (their margin schedules) at t >= 1
static int check_report_rows(const char* what, const Guide* g, int n, int t) {
    EDMP_REQUIRE(t >= 0 && t <= g->rows_T, "%s: t=%d outside 0..%d", what, t, g->rows_T);
    EDMP_REQUIRE(t == 0 || n == g->B, "%s: t >= 1 reads the rows' margin schedules: %d rows given, %d bound", what, n, g->B);  // (a batch: always its rows)
    return EDMP_OK;
}

// edmp_sdf_rows_dev and edmp_scenes_sdf_rows_dev behind their own state, table, pointer and shape checks: n rows of S scenes whose L
// interior waypoints lie at columns off .. off + L - 1 of rows of ldw columns; starts / goals [S][7]; rps as SdfArgs::rps
static int sdf_rows(edmp_ctx* ctx, const char* what, const double* joints_dev, int S, int n, int ldw, int off, int L, int t, int rps,
                    const double* starts, const double* goals, double* cost_dev, double* clearance_dev) {
    Guide* g = ctx->guide;
    if (int rc = check_report_rows(what, g, n, t)) return rc;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    sampler_end_run(ctx);  // (the guide's start / goal pairs are replaced)
    if (int rc = guide_set_startgoal_scenes(ctx, S, starts, goals)) return rc;
    SdfArgs a;
    fill_args(g, a, joints_dev, ldw, off, L, t, 0);
    a.rps = rps;
    if (n != g->B) a.smooth = nullptr;  // rows that are not the bound ones carry no smoothness weight
    a.v.cost = cost_dev;
    a.v.clearance = clearance_dev;
    hipLaunchKernelGGL(sdf_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, a, g->rc);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

extern "C" int edmp_sdf_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int L, int t, const double* start, const double* goal,
                                 double* cost_dev, double* clearance_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_sdf_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_sdf_rows_dev");
    EDMP_REQUIRE(ctx->guide->sdf.ns > 0, "edmp_sdf_rows_dev: call edmp_sdf_set first (the sphere table)");  // (EDMP_ERR_ARG; the batch: EDMP_ERR_STATE)
    EDMP_REQUIRE(joints_dev && start && goal && cost_dev && clearance_dev, "edmp_sdf_rows_dev: null pointer");
    EDMP_REQUIRE(n >= 1 && L >= 1 && L + 2 <= 64, "edmp_sdf_rows_dev: need n >= 1 and 1 <= L <= 62 waypoints per row (got %d, %d)", n, L);
    // interior waypoints only, any n at t = 0; one scene: rps = 0
    return sdf_rows(ctx, "edmp_sdf_rows_dev", joints_dev, 1, n, L, 0, L, t, 0, start, goal, cost_dev, clearance_dev);
}

// edmp_sdf_rows_dev for a bound scene batch: every row against its own scene's primitives, kinds and start / goal pair
extern "C" int edmp_scenes_sdf_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int t, const double* starts, const double* goals,
                                        double* cost_dev, double* clearance_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_sdf_rows_dev");
    if (ctx->guide->sdf.ns <= 0) {
        set_error("edmp_scenes_sdf_rows_dev: call edmp_scene_batch_set_sdf first (the sphere table)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(X_dev && starts && goals && cost_dev && clearance_dev, "edmp_scenes_sdf_rows_dev: null pointer");
    EDMP_REQUIRE(N >= 3 && N <= 64, "edmp_scenes_sdf_rows_dev: need 3 <= N <= 64 waypoints per row (got %d)", N);
    // the full state with its start / goal columns; rps = B forced, for a batch of ONE scene too (rows / B = 0)
    return sdf_rows(ctx, "edmp_scenes_sdf_rows_dev", X_dev, S, S * B, N, 1, N - 2, t, B, starts, goals, cost_dev, clearance_dev);
}

// ---- what the optional terms share on the host -------------------------------------------------------------------------------------------
// A term's setter before its own checks: a guide with rows is bound, so is a sphere table (EDMP_ERR_STATE without one), no argument
// is null, and the n rows - with the *T steps where the term has a schedule, T = nullptr where it has none - are those of edmp_rows_set
static int term_precheck(edmp_ctx* ctx, const char* what, bool have_args, int n, const int* T = nullptr) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->row_class, "%s: no guide bound (scene and rows first)", what);
    const Guide* g = ctx->guide;
    if (g->sdf.ns <= 0) {
        set_error("%s: call edmp_sdf_set or edmp_scene_batch_set_sdf first (the term is defined on their sphere table)", what);
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(have_args, "%s: null argument", what);
    if (!T) EDMP_REQUIRE(n == g->B, "%s: %d rows given, edmp_rows_set holds %d", what, n, g->B);
    else EDMP_REQUIRE(n == g->B && *T == g->rows_T, "%s: %d rows x %d steps given, edmp_rows_set holds %d x %d", what, n, *T, g->B, g->rows_T);
    return EDMP_OK;
}

// a term's weights: finite and >= 0, > 0 only on an SDF row of the table tb; rows <- the indices of the weighted rows
static int weighted_rows(const char* what, const double* weight, int n, const SdfTable& tb, int rps, std::vector<int32_t>& rows) {
    char where[48];
    for (int b = 0; b < n; ++b) {
        EDMP_REQUIRE(std::isfinite(weight[b]) && weight[b] >= 0.0, "%s: %s: weight %g must be finite and >= 0", what, row_name(where, b, rps), weight[b]);
        if (weight[b] > 0.0) {
            EDMP_REQUIRE(b < (int)tb.row_h.size() && tb.row_h[b] == 1, "%s: %s: weight %g on a row that is not an SDF row", what, row_name(where, b, rps), weight[b]);
            rows.push_back(b);
        }
    }
    return EDMP_OK;
}

// a report of the self or goal term before its own checks: n rows whose L interior waypoints lie at columns off .. off + L - 1 of rows
// of ldw columns, at a step that the rows allow (check_report_rows)
static int check_term_report(const char* what, const Guide* g, int n, int ldw, int off, int L, int t) {
    EDMP_REQUIRE(n >= 1 && L >= 1 && L + 2 <= 64, "%s: need n >= 1 and 1 <= L <= 62 waypoints per row (got %d, %d)", what, n, L);
    EDMP_REQUIRE(off >= 0 && ldw >= 1 && (int64_t)off + L <= ldw, "%s: columns %d .. %d outside rows of %d", what, off, off + L - 1, ldw);
    return check_report_rows(what, g, n, t);
}

// ---- self-clearance term ------------------------------------------------------------------------------------------------------------
extern "C" int edmp_sdf_set_self(edmp_ctx* ctx, const int32_t* pair_mask, const double* weight, const double* self_margin, int n, int T) {
    if (int rc = term_precheck(ctx, "edmp_sdf_set_self", pair_mask && weight && self_margin, n, &T)) return rc;
    Guide* g = ctx->guide;
    const SdfTable& tb = g->sdf;
    SelfTerm& st = g->sdf.self;
    for (int a = 0; a < EDMP_N_LINKS; ++a)
        for (int b = a + 1; b < EDMP_N_LINKS; ++b)
            EDMP_REQUIRE(pair_mask[a * EDMP_N_LINKS + b] == 0 || pair_mask[a * EDMP_N_LINKS + b] == 1, "edmp_sdf_set_self: pair_mask[%d][%d] = %d must be 0 or 1", a,
                         b, (int)pair_mask[a * EDMP_N_LINKS + b]);
    const int rps = g->is_batch ? g->rps : 0;
    std::vector<int32_t> rows;
    if (int rc = weighted_rows("edmp_sdf_set_self", weight, n, tb, rps, rows)) return rc;
    if (int rc = check_schedule("edmp_sdf_set_self", "self_margin", self_margin, n, T, rps)) return rc;
    // the sphere pairs of the masked link pairs, in the order of the link-sorted table: s ascending, then u
    std::vector<int32_t> pairs;
    for (int la = 0; la < EDMP_N_LINKS; ++la)
        for (int s = tb.link_off[la]; s < tb.link_off[la + 1]; ++s)
            for (int lb = la + 1; lb < EDMP_N_LINKS; ++lb) {
                if (!pair_mask[la * EDMP_N_LINKS + lb]) continue;
                for (int u = tb.link_off[lb]; u < tb.link_off[lb + 1]; ++u) pairs.insert(pairs.end(), {s, u, la, lb});
            }
    if (int rc = guide_upload(ctx, [&] { st.drop(); },
                              {{(void**)&st.pairs, pairs.data(), pairs.size() * sizeof(int32_t), 4 * sizeof(int32_t)},
                               {(void**)&st.rows, rows.data(), rows.size() * sizeof(int32_t), sizeof(int32_t)},
                               {(void**)&st.weight, weight, (size_t)n * sizeof(double), 0},
                               {(void**)&st.margin, self_margin, (size_t)n * T * sizeof(double), 0}}))
        return rc;
    st.np = (int)(pairs.size() / 4);
    st.n = (int)rows.size();
    st.set = true;
    return EDMP_OK;
}

extern "C" int edmp_sdf_self_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int ldw, int off, int L, int t, double* cost_dev,
                                      double* clearance_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_sdf_self_rows_dev: scene not set");
    Guide* g = ctx->guide;
    if (g->sdf.ns <= 0 || !g->sdf.self.set) {
        set_error("edmp_sdf_self_rows_dev: call edmp_sdf_set_self first (the pair mask)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(joints_dev && cost_dev && clearance_dev, "edmp_sdf_self_rows_dev: null pointer");
    if (int rc = check_term_report("edmp_sdf_self_rows_dev", g, n, ldw, off, L, t)) return rc;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    SelfArgs a;
    fill_self_args(g, a, joints_dev, ldw, off, L, t, 0);
    if (n != g->B) a.weight = nullptr;  // rows that are not the bound ones: weight 1, the bare hinge sum
    a.v.cost = cost_dev;
    a.v.clearance = clearance_dev;
    hipLaunchKernelGGL(sdf_self_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, a, g->rc);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

// ---- tool-pose goal term -------------------------------------------------------------------------------------------------------------
// the rotation part of a row-major [R | p] frame is orthonormal to 1e-6
static bool frame_orthonormal(const double* f) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = f[a] * f[b] + f[4 + a] * f[4 + b] + f[8 + a] * f[8 + b] - (a == b ? 1.0 : 0.0);
            if (!(std::fabs(d) <= 1e-6)) return false;
        }
    return true;
}

extern "C" int edmp_sdf_set_goal(edmp_ctx* ctx, const double* weight, const double* rotation, const int32_t* window, const double* tool,
                                 const double* target, int n) {
    if (int rc = term_precheck(ctx, "edmp_sdf_set_goal", weight && rotation && window && tool, n)) return rc;
    Guide* g = ctx->guide;
    const SdfTable& tb = g->sdf;
    GoalTerm& gt = g->sdf.goal;
    const int S = g->S, rps = g->is_batch ? g->rps : 0;
    for (int k = 0; k < 12; ++k) EDMP_REQUIRE(std::isfinite(tool[k]), "edmp_sdf_set_goal: the tool frame holds a non-finite value");
    EDMP_REQUIRE(frame_orthonormal(tool), "edmp_sdf_set_goal: the rotation of the tool frame is not orthonormal to 1e-6");
    for (int s = 0; target && s < S; ++s) {
        for (int k = 0; k < 12; ++k) EDMP_REQUIRE(std::isfinite(target[s * 12 + k]), "edmp_sdf_set_goal: the target of scene %d holds a non-finite value", s);
        EDMP_REQUIRE(frame_orthonormal(target + s * 12), "edmp_sdf_set_goal: the rotation of scene %d's target is not orthonormal to 1e-6", s);
    }
    char where[48];
    std::vector<int32_t> rows;
    if (int rc = weighted_rows("edmp_sdf_set_goal", weight, n, tb, rps, rows)) return rc;
    for (int b = 0; b < n; ++b) {
        EDMP_REQUIRE(std::isfinite(rotation[b]) && rotation[b] >= 0.0, "edmp_sdf_set_goal: %s: rotation %g must be finite and >= 0", row_name(where, b, rps),
                     rotation[b]);
        EDMP_REQUIRE(window[b] >= 1, "edmp_sdf_set_goal: %s: window %d must be >= 1", row_name(where, b, rps), (int)window[b]);
    }
    std::vector<float> tg((size_t)S * 12);
    for (size_t i = 0; target && i < tg.size(); ++i) tg[i] = (float)target[i];
    if (int rc = guide_upload(ctx, [&] { gt.drop(); },
                              {{(void**)&gt.rows, rows.data(), rows.size() * sizeof(int32_t), sizeof(int32_t)},
                               {(void**)&gt.weight, weight, (size_t)n * sizeof(double), 0},
                               {(void**)&gt.rotation, rotation, (size_t)n * sizeof(double), 0},
                               {(void**)&gt.window, window, (size_t)n * sizeof(int32_t), 0},
                               {(void**)&gt.target, tg.data(), target ? tg.size() * sizeof(float) : 0, EDMP_MAX_SCENES * 12 * sizeof(float)}}))
        return rc;
    for (int k = 0; k < 12; ++k) gt.tool[k] = tool[k];
    gt.n = (int)rows.size();
    gt.derived = target == nullptr;
    gt.have_target = target != nullptr;  // derived: the next start / goal upload brings the poses (guide_goal_targets)
    gt.set = true;
    return EDMP_OK;
}

extern "C" int edmp_sdf_goal_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int ldw, int off, int L, int t, double* cost_dev,
                                      double* distance_dev, double* angle_dev, double* min_distance_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_sdf_goal_rows_dev: scene not set");
    Guide* g = ctx->guide;
    if (g->sdf.ns <= 0 || !g->sdf.goal.set) {
        set_error("edmp_sdf_goal_rows_dev: call edmp_sdf_set_goal first (the tool frame and the targets)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(joints_dev && cost_dev && distance_dev && angle_dev && min_distance_dev, "edmp_sdf_goal_rows_dev: null pointer");
    if (int rc = check_term_report("edmp_sdf_goal_rows_dev", g, n, ldw, off, L, t)) return rc;
    EDMP_REQUIRE(!g->is_batch || n == g->B, "edmp_sdf_goal_rows_dev: a scene batch reports its own rows (row r reads scene r / rows-per-scene's target): %d rows given, %d bound",
                 n, g->B);
    if (!g->sdf.goal.have_target) {
        set_error("edmp_sdf_goal_rows_dev: the targets are derived from the goal configurations and no start / goal pair has been handed over since edmp_sdf_set_goal");
        return EDMP_ERR_STATE;
    }
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    GoalArgs a;
    fill_goal_args(g, a, joints_dev, ldw, off, L, t, 0);
    a.n = n;
    if (n != g->B) {  // rows that are not the bound ones: weight 1, rotation 1, the ramp over the whole row
        a.weight = a.rotation = nullptr;
        a.window = nullptr;
    }
    a.v.cost = cost_dev;
    a.distance = distance_dev;
    a.angle = angle_dev;
    a.min_distance = min_distance_dev;
    hipLaunchKernelGGL(sdf_goal_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, a, g->rc);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

// ---- swept-clearance term -------------------------------------------------------------------------------------------------------------
extern "C" int edmp_sdf_set_sweep(edmp_ctx* ctx, const double* weight, const int32_t* substeps, int n) {
    if (int rc = term_precheck(ctx, "edmp_sdf_set_sweep", weight && substeps, n)) return rc;
    Guide* g = ctx->guide;
    SweepTerm& sw = g->sdf.sweep;
    const int rps = g->is_batch ? g->rps : 0;
    char where[48];
    std::vector<int32_t> rows, ks(substeps, substeps + n);
    if (int rc = weighted_rows("edmp_sdf_set_sweep", weight, n, g->sdf, rps, rows)) return rc;
    for (int b = 0; b < n; ++b) {
        const bool in_range = substeps[b] >= 2 && substeps[b] <= EDMP_MAX_SWEEP_SUBSTEPS;
        if (weight[b] > 0.0)
            EDMP_REQUIRE(in_range, "edmp_sdf_set_sweep: %s: substeps %d outside 2..%d under a weight > 0", row_name(where, b, rps), (int)substeps[b],
                         EDMP_MAX_SWEEP_SUBSTEPS);
        else if (!in_range)
            ks[b] = 1;  // a row without a weight: no interpolant (the report's loop stays bounded whatever the caller left there)
    }
    if (int rc = guide_upload(ctx, [&] { sw.drop(); },
                              {{(void**)&sw.rows, rows.data(), rows.size() * sizeof(int32_t), sizeof(int32_t)},
                               {(void**)&sw.weight, weight, (size_t)n * sizeof(double), 0},
                               {(void**)&sw.substeps, ks.data(), (size_t)n * sizeof(int32_t), 0}}))
        return rc;
    sw.n = (int)rows.size();
    sw.set = true;
    return EDMP_OK;
}

// edmp_sdf_sweep_rows_dev and edmp_scenes_sdf_sweep_rows_dev behind their own state, table, pointer and shape checks (the arguments of
// sdf_rows plus substeps).  The S start / goal pairs go into a block of the term's own: the guide's pairs, and so a segmented run, stay
static int sdf_sweep_rows(edmp_ctx* ctx, const char* what, const double* joints_dev, int S, int n, int ldw, int off, int L, int t, int rps,
                          const double* starts, const double* goals, int substeps, double* cost_dev, double* clearance_dev) {
    Guide* g = ctx->guide;
    SweepTerm& sw = g->sdf.sweep;
    if (int rc = check_report_rows(what, g, n, t)) return rc;
    EDMP_REQUIRE(substeps >= 0 && substeps <= EDMP_MAX_SWEEP_SUBSTEPS && substeps != 1, "%s: substeps %d must be 0 (the bound rows' own) or lie in 2..%d", what,
                 substeps, EDMP_MAX_SWEEP_SUBSTEPS);
    if (substeps == 0) {
        if (!sw.set) {
            set_error("%s: substeps = 0 reads the bound rows' weights and substeps: call edmp_sdf_set_sweep first", what);
            return EDMP_ERR_STATE;
        }
        EDMP_REQUIRE(n == g->B, "%s: substeps = 0 reads the bound rows' weights and substeps: %d rows given, %d bound", what, n, g->B);
    } else {
        EDMP_REQUIRE(t == 0, "%s: substeps = %d > 0 reports the bare hinge sum at t = 0 only (t = %d given)", what, substeps, t);
    }
    for (int i = 0; i < S * 7; ++i) EDMP_REQUIRE(std::isfinite(starts[i]) && std::isfinite(goals[i]), "%s: scene %d: non-finite start / goal", what, i / 7);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    if (!sw.startgoal)
        if (int rc = ctx_alloc(ctx, (void**)&sw.startgoal, EDMP_MAX_SCENES * 14 * sizeof(float))) return rc;
    float sg[EDMP_MAX_SCENES * 14];
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < 7; ++i) {
            sg[s * 14 + i] = (float)starts[s * 7 + i];
            sg[s * 14 + 7 + i] = (float)goals[s * 7 + i];
        }
    EDMP_HIP_CHECK(hipMemcpyAsync(sw.startgoal, sg, (size_t)S * 14 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    SweepArgs a;
    fill_sweep_args(g, a, joints_dev, ldw, off, L, t, 0);
    a.s.rps = rps;
    a.s.startgoal = sw.startgoal;
    if (substeps > 0) {  // weight 1 and K = substeps on any rows
        a.weight = nullptr;
        a.substeps = nullptr;
        a.K = substeps;
    }
    a.s.v.cost = cost_dev;
    a.s.v.clearance = clearance_dev;
    hipLaunchKernelGGL(sdf_sweep_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, a, g->rc);
    const hipError_t e = hipGetLastError();
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host pairs live on this frame
    EDMP_HIP_CHECK(e);
    return EDMP_OK;
}

extern "C" int edmp_sdf_sweep_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int L, int t, const double* start, const double* goal,
                                       int substeps, double* cost_dev, double* clearance_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_sdf_sweep_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_sdf_sweep_rows_dev");
    EDMP_REQUIRE(ctx->guide->sdf.ns > 0, "edmp_sdf_sweep_rows_dev: call edmp_sdf_set first (the sphere table)");
    EDMP_REQUIRE(joints_dev && start && goal && cost_dev && clearance_dev, "edmp_sdf_sweep_rows_dev: null pointer");
    EDMP_REQUIRE(n >= 1 && L >= 1 && L + 2 <= 64, "edmp_sdf_sweep_rows_dev: need n >= 1 and 1 <= L <= 62 waypoints per row (got %d, %d)", n, L);
    return sdf_sweep_rows(ctx, "edmp_sdf_sweep_rows_dev", joints_dev, 1, n, L, 0, L, t, 0, start, goal, substeps, cost_dev, clearance_dev);
}

extern "C" int edmp_scenes_sdf_sweep_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int t, const double* starts, const double* goals,
                                              int substeps, double* cost_dev, double* clearance_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_sdf_sweep_rows_dev");
    if (ctx->guide->sdf.ns <= 0) {
        set_error("edmp_scenes_sdf_sweep_rows_dev: call edmp_scene_batch_set_sdf first (the sphere table)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(X_dev && starts && goals && cost_dev && clearance_dev, "edmp_scenes_sdf_sweep_rows_dev: null pointer");
    EDMP_REQUIRE(N >= 3 && N <= 64, "edmp_scenes_sdf_sweep_rows_dev: need 3 <= N <= 64 waypoints per row (got %d)", N);
    return sdf_sweep_rows(ctx, "edmp_scenes_sdf_sweep_rows_dev", X_dev, S, S * B, N, 1, N - 2, t, B, starts, goals, substeps, cost_dev, clearance_dev);
}

// ---- repair of finished rows -----------------------------------------------------------------------------------------------------------
// edmp_sdf_repair_rows_dev and edmp_scenes_sdf_repair_rows_dev behind their own state, table and pointer checks: n rows of S scenes of the
// state X (n, 7, N), starts / goals [S][7], rps as SdfArgs::rps.  Every refusal comes before any device call.  The pairs and the row list
// go into blocks of the call's own: the guide's pairs, and so a segmented run, stay
static int sdf_repair_rows(edmp_ctx* ctx, const char* what, double* X_dev, int S, int n, int N, int rps, const double* starts, const double* goals,
                           const int32_t* rows_host, int n_rows, int substeps, int iters, double margin, double smoothness, double step, double max_step,
                           double* cost_dev, double* clearance_dev, int32_t* iterations_dev) {
    Guide* g = ctx->guide;
    RepairBlocks& rb = g->sdf.repair;
    EDMP_REQUIRE(N >= 3 && N <= 64, "%s: need 3 <= N <= 64 waypoints per row (got %d)", what, N);
    EDMP_REQUIRE(substeps >= 1 && substeps <= EDMP_MAX_SWEEP_SUBSTEPS, "%s: substeps %d outside 1..%d", what, substeps, EDMP_MAX_SWEEP_SUBSTEPS);
    EDMP_REQUIRE(iters >= 0 && iters <= EDMP_MAX_REPAIR_ITERS, "%s: iters %d outside 0..%d", what, iters, EDMP_MAX_REPAIR_ITERS);
    EDMP_REQUIRE(std::isfinite(margin) && margin >= 0.0, "%s: margin %g must be finite and >= 0", what, margin);
    EDMP_REQUIRE(std::isfinite(smoothness) && smoothness >= 0.0, "%s: smoothness %g must be finite and >= 0", what, smoothness);
    EDMP_REQUIRE(std::isfinite(step) && step > 0.0, "%s: step %g must be finite and > 0", what, step);
    EDMP_REQUIRE(std::isfinite(max_step) && max_step > 0.0, "%s: max_step %g must be finite and > 0", what, max_step);
    for (int i = 0; i < S * 7; ++i) EDMP_REQUIRE(std::isfinite(starts[i]) && std::isfinite(goals[i]), "%s: scene %d: non-finite start / goal", what, i / 7);
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;  // (rowlist.h)
    const int launch = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    if (!rb.startgoal)
        if (int rc = ctx_alloc(ctx, (void**)&rb.startgoal, EDMP_MAX_SCENES * 14 * sizeof(float))) return rc;
    if (rows_host && rb.rows_cap < n_rows) {
        EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // nothing enqueued still reads the list that goes
        ctx_release(ctx, rb.rows);
        rb.rows = nullptr;
        rb.rows_cap = 0;
        if (int rc = ctx_alloc(ctx, (void**)&rb.rows, (size_t)n_rows * sizeof(int32_t))) return rc;
        rb.rows_cap = n_rows;
    }
    float sg[EDMP_MAX_SCENES * 14];
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < 7; ++i) {
            sg[s * 14 + i] = (float)starts[s * 7 + i];
            sg[s * 14 + 7 + i] = (float)goals[s * 7 + i];
        }
    EDMP_HIP_CHECK(hipMemcpyAsync(rb.startgoal, sg, (size_t)S * 14 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (rows_host) EDMP_HIP_CHECK(hipMemcpyAsync(rb.rows, rows_host, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    RepairArgs a;
    fill_args(g, a.s, X_dev, N, 1, N - 2, 0, 1);  // the full state with its start / goal columns, clipped as the guide clips; no step
    a.s.v.rows = rows_host ? rb.rows : nullptr;
    a.s.smooth = nullptr;
    a.s.rps = rps;
    a.s.startgoal = rb.startgoal;
    a.X = X_dev;
    a.K = substeps;
    a.iters = iters;
    a.margin = (float)margin;
    a.smooth = (float)smoothness;
    a.step = step;
    a.max_step = max_step;
    a.cost = cost_dev;
    a.clearance = clearance_dev;
    a.iterations = iterations_dev;
    hipLaunchKernelGGL(sdf_repair_kernel, dim3(launch), dim3(256), 0, ctx->stream, a, g->rc);
    const hipError_t e = hipGetLastError();
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host pairs live on this frame, the list in the caller's array
    EDMP_HIP_CHECK(e);
    return EDMP_OK;
}

extern "C" int edmp_sdf_repair_rows_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const double* start, const double* goal, const int32_t* rows_host,
                                        int n_rows, int substeps, int iters, double margin, double smoothness, double step, double max_step,
                                        double* cost_dev, double* clearance_dev, int32_t* iterations_dev) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb, "edmp_sdf_repair_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_sdf_repair_rows_dev");
    EDMP_REQUIRE(ctx->guide->sdf.ns > 0, "edmp_sdf_repair_rows_dev: call edmp_sdf_set first (the sphere table)");
    EDMP_REQUIRE(X_dev && start && goal && cost_dev && clearance_dev && iterations_dev, "edmp_sdf_repair_rows_dev: null pointer");
    EDMP_REQUIRE(n >= 1, "edmp_sdf_repair_rows_dev: need n >= 1 rows (got %d)", n);
    return sdf_repair_rows(ctx, "edmp_sdf_repair_rows_dev", X_dev, 1, n, N, 0, start, goal, rows_host, n_rows, substeps, iters, margin, smoothness, step,
                           max_step, cost_dev, clearance_dev, iterations_dev);
}

// edmp_sdf_repair_rows_dev for a bound scene batch: every row against its own scene's primitives, kinds and start / goal pair
extern "C" int edmp_scenes_sdf_repair_rows_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const double* starts, const double* goals,
                                               const int32_t* rows_host, int n_rows, int substeps, int iters, double margin, double smoothness, double step,
                                               double max_step, double* cost_dev, double* clearance_dev, int32_t* iterations_dev) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_sdf_repair_rows_dev");
    if (ctx->guide->sdf.ns <= 0) {
        set_error("edmp_scenes_sdf_repair_rows_dev: call edmp_scene_batch_set_sdf first (the sphere table)");
        return EDMP_ERR_STATE;
    }
    EDMP_REQUIRE(X_dev && starts && goals && cost_dev && clearance_dev && iterations_dev, "edmp_scenes_sdf_repair_rows_dev: null pointer");
    // rps = B forced, for a batch of ONE scene too (rows / B = 0)
    return sdf_repair_rows(ctx, "edmp_scenes_sdf_repair_rows_dev", X_dev, S, S * B, N, B, starts, goals, rows_host, n_rows, substeps, iters, margin, smoothness,
                           step, max_step, cost_dev, clearance_dev, iterations_dev);
}
