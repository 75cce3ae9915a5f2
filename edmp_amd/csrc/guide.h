// guide.h — the per-scene guide object shared by guide.hip (tables, cost / gradient kernels), sdf.hip, success.hip (the
// geometric success check over the finished batch) and selfcol.hip (the robot tables of the self-collision check).  The chain
// arithmetic behind RobotConst is chain.h.
#pragma once
#include "common.h"

namespace edmp {

struct RobotConst {
    float dh[7][4];      // a, d, cos(alpha), sin(alpha)
    float sf[9][12];     // static frames, row-major 3x4
    float he[9][3];      // link half extents
    double qlo[7], qhi[7];
};

// What the optional terms of the SDF guide (sdf.hip) share.  A term belongs to the sphere table, whose drop() drops it
struct RowTerm {
    bool set = false;          // the term's arrays are bound (edmp_sdf_set_<term>)
    int32_t* rows = nullptr;   // [n] indices of the rows whose weight is > 0
    int n = 0;                 // (0: the gradient paths launch what they launched without the term)
    double* weight = nullptr;  // [B]
    void drop() { n = 0; set = false; }
};

// self-clearance term (edmp_sdf_set_self); set: a pair list is bound (it may be empty)
struct SelfTerm : RowTerm {
    int32_t* pairs = nullptr;  // [np][4] = sphere s, sphere u (link-sorted indices), link of s, link of u; s ascending, then u
    int np = 0;
    double* margin = nullptr;  // [B][T]
    void drop() { RowTerm::drop(); np = 0; }
    std::vector<void*> blocks() const { return {pairs, rows, weight, margin}; }
};

// tool-pose goal term (edmp_sdf_set_goal); set: the row arrays, the tool frame and the target block are bound
struct GoalTerm : RowTerm {
    bool derived = false;        // the targets are the poses of the scenes' goal configurations (guide_goal_targets), not the caller's
    bool have_target = false;    // the target block holds every scene's pose (derived: since the last start / goal upload)
    double* rotation = nullptr;  // [B]
    int32_t* window = nullptr;   // [B]
    float* target = nullptr;     // [EDMP_MAX_SCENES][12] f32 row-major [R* | p*] per scene
    double tool[12] = {};        // the tool frame behind joint 7, row-major [R | p]
    float target_h[EDMP_MAX_SCENES * 12] = {};  // host staging of a derived upload (it outlives the enqueued copy)
    void drop() { RowTerm::drop(); derived = have_target = false; }
    std::vector<void*> blocks() const { return {rows, weight, rotation, window, target}; }
};

// swept-clearance term (edmp_sdf_set_sweep)
struct SweepTerm : RowTerm {
    int32_t* substeps = nullptr;  // [B]; 1 (no interpolant) on a row without a weight whose value lies outside 2..64
    float* startgoal = nullptr;   // [EDMP_MAX_SCENES][14] f32: the pairs of the last report call (the guide's own stay what they are)
    std::vector<void*> blocks() const { return {rows, weight, substeps, startgoal}; }
};

// what a repair call (edmp_sdf_repair_rows_dev) keeps on the device: no term, nothing that a gradient path reads
struct RepairBlocks {
    float* startgoal = nullptr;  // [EDMP_MAX_SCENES][14] f32: the pairs of the last call (the guide's own stay what they are)
    int32_t* rows = nullptr;     // [rows_cap] the listed rows of the last call that listed some, grow-only
    int rows_cap = 0;
    std::vector<void*> blocks() const { return {startgoal, rows}; }
};

// sphere signed-distance guide (sdf.hip, edmp_sdf_set): belongs to the rows it was set for
struct SdfTable {
    float* sph = nullptr;       // [ns][4] centre | radius in link-box frames, sorted by link
    int ns = 0;                 // spheres (0: no table bound)
    int link_off[EDMP_N_LINKS + 1] = {};
    int32_t* rows = nullptr;    // [n] indices of the SDF rows
    int n = 0;                  // SDF rows of the batch (0: the gradient paths launch what they always launched)
    double* margin = nullptr;   // [B][T]
    double* smooth = nullptr;   // [B]
    std::vector<int32_t> row_h; // [B] host copy of edmp_sdf_set's 0/1 flags (the terms' setters check their weights against it)
    SelfTerm self;
    GoalTerm goal;
    SweepTerm sweep;
    RepairBlocks repair;
    void drop() { n = ns = 0; self.drop(); goal.drop(); sweep.drop(); }  // a new table, or new rows, drop the terms too
    std::vector<void*> blocks() const {  // (guide_destroy): the table's own four and what each term reports
        std::vector<void*> b{sph, rows, margin, smooth};
        for (const std::vector<void*>& t : {self.blocks(), goal.blocks(), sweep.blocks(), repair.blocks()}) b.insert(b.end(), t.begin(), t.end());
        return b;
    }
};

struct Guide {
    int no = 0, G = 0, T = 0;
    float* aabb = nullptr;  // [G][T+1][no][6]
    // scene batch (edmp_scene_batch_set): S scenes share this object; class c holds cls_no[c] obstacles in its own [T+1][cls_no][6] block
    // at float offset cls_off[c] of aabb (no = the largest count).  S = 1 / cls_no = nullptr: one scene, the table above
    int S = 1;
    bool is_batch = false;         // built by edmp_scene_batch_set (a batch of ONE scene included): the edmp_scenes_* scoring calls need it
    std::vector<int> scene_no_h;   // [S] obstacles of each scene
    std::vector<int> scene_off_h;  // [S] first obstacle row of each scene in obb / kind
    int32_t* cls_no = nullptr;    // [2][G] device: counts, then float offsets
    std::vector<int> cls_off_h;   // [G] host copy of the offsets (S > 1)
    std::vector<int> cls_no_h;    // [G] host copy (S > 1)
    std::vector<int> cls_scene_h; // [G] scene of each class (S > 1)
    int rps = 0;                  // rows per scene, set by edmp_rows_set (= B for one scene)
    RobotConst rc{};
    // the obstacles as the simulator of the reference spawns them (lib/environment.py:230-268): oriented boxes / cylinders,
    // f64 [no][16] = world rotation (row-major 3x3, columns = axes), centre, half extents, pad; kind 0 cuboid / 1 cylinder
    double* obb = nullptr;
    int32_t* kind = nullptr;
    // rows
    int B = 0;
    int32_t* row_class = nullptr;
    float* method = nullptr;
    double* grad_norm = nullptr;
    double* sched = nullptr;  // [B][T]
    int rows_T = 0;
    // scratch
    float* graw = nullptr;    // [B][7][L] raw f32 gradient
    double* rowsq = nullptr;  // [B]
    double* sumsq = nullptr;  // [EDMP_MAX_SCENES]: one sum(g^2) per scene (index 0 = the whole batch of one scene)
    float* startgoal = nullptr;  // [EDMP_MAX_SCENES][14] f32: start (7) | goal (7) per scene
    int scratch_B = 0, scratch_L = 0;
    float* vol_rows = nullptr;  // [B] for best trajectory
    int32_t* flags = nullptr;   // [3][flags_B] success check: ok, first colliding waypoint, within limits; + [flags_Q][4] counts
    int flags_B = 0, flags_Q = 1;  // (one count quadruple per scene: a scene batch asks for S of them)
    // IK-goal filter of a scene batch (edmp_scenes_goal_filter_dev): one volume and one key per candidate, grow-only
    float* cand_vol = nullptr;   // [cand_cap]
    double* cand_key = nullptr;  // [cand_cap]
    int cand_cap = 0;
    SdfTable sdf;  // row-level like the arrays above: edmp_rows_set drops it
};

// sdf.hip: overwrite graw / rowsq of the bound guide's SDF rows (no SDF rows: nothing is launched)
int sdf_overlay(edmp_ctx* ctx, const double* joints, int ldw, int off, int L, int t, int do_clip);
int guide_set_startgoal(edmp_ctx* ctx, const double* start, const double* goal);  // guide.hip
int guide_set_startgoal_scenes(edmp_ctx* ctx, int S, const double* starts, const double* goals);  // guide.hip: [S][14] of a scene batch
// sdf.hip: a goal term with derived targets takes (R* | p*) = T_7(goal_s) . tool of the S goals [S][7] (f64 on the host) and enqueues its
// upload on the context's stream; the caller's own synchronisation completes it.  No such term: nothing happens
int guide_goal_targets(edmp_ctx* ctx, int S, const double* goals);

// ctx->d_int (EDMP_MAX_SCENES device ints for small read-backs), allocated at its first use and kept for the life of the context
inline int ctx_small_ints(edmp_ctx* ctx) {
    if (!ctx->d_int) EDMP_HIP_CHECK(hipMalloc((void**)&ctx->d_int, EDMP_MAX_SCENES * sizeof(int)));
    return EDMP_OK;
}

// Which entry points take which kind of bound guide (the two macros below are the whole state check; include/edmp_hip.h states the rest):
//   single only (EDMP_REFUSE_SCENE_BATCH: refused on a batch of S > 1 scenes, never answered with scene 0's data):
//     edmp_guide_cost_dev, edmp_guide_swept_cost_dev, edmp_guide_gradient_dev, edmp_row_swept_volumes_dev, edmp_success_rows_dev,
//     edmp_scene_set_shapes, edmp_sdf_rows_dev, edmp_sdf_sweep_rows_dev, edmp_sdf_repair_rows_dev, edmp_shortcut_rows_dev, edmp_shortcut_rows_self_dev, edmp_blend_rows_dev, edmp_blend_rows_self_dev; with checks of their own edmp_sdf_set (a batch of ONE scene refused too) and the
//     single-scene loops and teacher-forced steps of sampler.hip
//   batch only (EDMP_REQUIRE_SCENE_BATCH: the bound guide came from edmp_scene_batch_set, a batch of ONE scene included, and holds
//     exactly S scenes x B rows): edmp_scenes_swept_volumes_dev, edmp_scenes_select_rows_dev, edmp_scenes_success_rows_dev,
//     edmp_scenes_sdf_rows_dev, edmp_scenes_sdf_sweep_rows_dev, edmp_scenes_sdf_repair_rows_dev, edmp_scenes_shortcut_rows_dev, edmp_scenes_shortcut_rows_self_dev, edmp_scenes_blend_rows_dev, edmp_scenes_blend_rows_self_dev, edmp_scenes_goal_filter_dev, edmp_scene_batch_set_sdf; edmp_scene_batch_set_shapes (its own wording)
//   either: edmp_rows_set, edmp_scene_read_aabbs, edmp_argmin_dev, edmp_select_row_dev, edmp_metrics_rows_dev (the last three read no guide),
//     edmp_self_collision_rows_dev (the robot tables only)
#define EDMP_REFUSE_SCENE_BATCH(g, what)                                                                                          \
    do {                                                                                                                          \
        if ((g) && (g)->S > 1) {                                                                                                  \
            edmp::set_error("%s: the bound guide is a scene batch of %d scenes (edmp_scene_batch_set); use one guide per scene", \
                            what, (g)->S);                                                                                        \
            return EDMP_ERR_STATE;                                                                                                \
        }                                                                                                                         \
    } while (0)

#define EDMP_REQUIRE_SCENE_BATCH(ctx, S_, B_, what)                                                                                       \
    do {                                                                                                                                  \
        if (!(ctx) || !(ctx)->guide || !(ctx)->guide->aabb || !(ctx)->guide->obb || !(ctx)->guide->row_class) {                         \
            edmp::set_error("%s: no scene batch bound (edmp_scene_batch_set + edmp_rows_set first)", what);                             \
            return (ctx) ? EDMP_ERR_STATE : EDMP_ERR_ARG;                                                                               \
        }                                                                                                                                 \
        if (!(ctx)->guide->is_batch) {                                                                                                    \
            edmp::set_error("%s: the bound guide is a single-scene guide (edmp_scene_set); it has its own per-scene entry point", what); \
            return EDMP_ERR_STATE;                                                                                                        \
        }                                                                                                                                 \
        if ((S_) != (ctx)->guide->S || (B_) < 1 || (int64_t)(S_) * (B_) != (ctx)->guide->B) {                                          \
            edmp::set_error("%s: %d scenes x %d rows given, the bound scene batch holds %d scenes x %d rows", what, (int)(S_), (int)(B_), \
                            (ctx)->guide->S, (ctx)->guide->rps);                                                                         \
            return EDMP_ERR_ARG;                                                                                                          \
        }                                                                                                                                 \
    } while (0)

}  // namespace edmp
