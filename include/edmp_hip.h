/* edmp_hip.h — C-ABI of libedmp_hip.so: the MI355X (gfx950) implementation of EDMP's guided reverse-diffusion
 * sampler hot path.  This is the drop-in boundary: plain pointers and sizes, opaque context handle,
 * int status return (0 = ok, <0 = error; text via edmp_last_error()).  No torch / Python types.
 *
 * The reference (vishal-2000/EDMP) has no FFI: the path is reached through duck-typed Python objects created in
 * infer_serial.py:43-51,112 and passed to Diffusion.denoise_guided (infer_serial.py:134-143).  Each entry point
 * below names the reference method(s) it replaces (paths relative to the reference checkout); the Python binding
 * that exposes the reference's signatures on top of this ABI is edmp_amd/_capi.py (ctypes), see INTEGRATION.md.
 *
 * Conventions: pointers suffixed _dev are device (HBM) addresses on the context's GPU, all others are host
 * addresses read synchronously before the call returns.  All device work is stream-ordered on the context's
 * stream (edmp_ctx_set_stream); calls return without synchronising unless stated.  One host thread per context.
 * Trajectory tensors use the reference's layout (B, C=7, N) row-major, "f64" = IEEE double, "f32" = float.
 */
#ifndef EDMP_HIP_H
#define EDMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDMP_OK 0
#define EDMP_ERR_ARG (-1)
#define EDMP_ERR_HIP (-2)
#define EDMP_ERR_STATE (-3)
#define EDMP_ERR_LAYOUT (-4) /* edmp_unet_load_packed: the image was packed by another library version / under other builder switches */

#define EDMP_MAX_LEVELS 8
#define EDMP_N_JOINTS 7
#define EDMP_N_LINKS 9
#define EDMP_MAX_OBSTACLES 64
#define EDMP_MAX_SCENES 16
#define EDMP_MAX_SPHERES 128
#define EDMP_MAX_SWEEP_SUBSTEPS 64 /* edmp_sdf_set_sweep: interpolants per segment + 1 */
#define EDMP_MAX_REPAIR_ITERS 1024 /* edmp_sdf_repair_rows_dev: a cap so that a launch stays bounded, not a tuned value */
#define EDMP_MAX_SHORTCUT_PASSES 1024 /* edmp_shortcut_rows_dev: a cap so that a launch stays bounded, not a tuned value */
#define EDMP_MAX_TIMED_SAMPLES 1048576 /* edmp_sample_rows_dev: samples per row; a cap so that a launch stays bounded, not a tuned value */

typedef struct edmp_ctx edmp_ctx;

/* ---- context ------------------------------------------------------------------------------------------- */
const char* edmp_last_error(void);
int edmp_version(void);
/* one context per GPU; creates its own stream */
int edmp_ctx_create(int device, edmp_ctx** out);
void edmp_ctx_destroy(edmp_ctx* ctx);
/* run on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the context's own stream */
int edmp_ctx_set_stream(edmp_ctx* ctx, void* hip_stream);
int edmp_ctx_synchronize(edmp_ctx* ctx);

/* ---- denoiser: TemporalUNet -------------------------------------------------------------------------- */
/* replaces TemporalUNet.__init__/load (diffusion/models/temporalunet.py:11-45, 88-92) */
typedef struct edmp_unet_desc {
    int32_t input_dim;             /* 7 */
    int32_t time_dim;              /* 32 */
    int32_t n_levels;              /* len(dims), 6 */
    int32_t dims[EDMP_MAX_LEVELS]; /* (32,64,128,256,512,512) */
    int32_t horizon;               /* N = 50 */
    int32_t T;                     /* number of diffusion steps the time-bias table covers (255) */
} edmp_unet_desc;

/* number of floats of the flat parameter blob for `desc` (all state-dict tensors, in state-dict order, each in
 * its native torch layout, concatenated) */
int64_t edmp_unet_param_count(const edmp_unet_desc* desc);
/* upload + repack weights, precompute the (T x sum Cout) time-bias table, allocate activations for max_batch */
int edmp_unet_load(edmp_ctx* ctx, const edmp_unet_desc* desc, const float* params, int64_t n_params, int max_batch);
/* Packed weight image = the device-side layout edmp_unet_load produces from the state dict (conv weights as MFMA
 * fragment streams / [tap][Cout][Cin], biases, GroupNorm affine, time-MLP weights), as ONE float blob that loads with a
 * single host-to-device copy (e.g. straight from an mmap'ed file) instead of re-reading, flattening and repacking 120 MB
 * (the reference's load is torch.load + load_state_dict, temporalunet.py:88-92).  edmp_unet_packed_size returns the
 * image's float count of the current model and the library's layout id; an image only loads into the same
 * architecture (desc) and layout id. */
int64_t edmp_unet_packed_size(edmp_ctx* ctx, int* layout);
int edmp_unet_read_packed(edmp_ctx* ctx, float* out_host, int64_t capacity);
int edmp_unet_load_packed(edmp_ctx* ctx, const edmp_unet_desc* desc, const float* packed, int64_t n_packed, int layout,
                          int max_batch);
/* host-only (no context, no GPU): the layer program edmp_unet_load would build for `desc` under the current builder switches.
 * For every op i < min(*n_ops, cap): the kernel instance name (64 bytes each) exactly as edmp_prof_ops reports it for the built model;
 * *layout / *n_packed: the layout id and float count edmp_unet_packed_size reports for it.  No reference counterpart. */
int edmp_unet_plan_describe(const edmp_unet_desc* desc, int cap, int* n_ops, char* names, int* layout, int64_t* n_packed);
/* replaces TemporalUNet.forward (temporalunet.py:47-76): x (B,C,N) f32, integer t in [1,T] -> eps (B,C,N) f32 */
int edmp_unet_forward_dev(edmp_ctx* ctx, const float* x_dev, int B, int t, float* eps_dev);
/* debug/parity: copy an internal activation of the last forward, converted to the reference layout (B, C, L) f32, into
 * out_dev (room for `capacity` floats).  which: 0..n_levels-1 = output of down level i, 100 = middle block, 200+i = output
 * of up level i.  B must lie in 1..max_batch and B*C*L must fit, else nothing is launched.  out_dev == NULL with
 * capacity == 0 only reports the tap's C and L (size the buffer first) */
int edmp_unet_read_activation_dev(edmp_ctx* ctx, int which, int B, float* out_dev, int64_t capacity, int* C_out, int* L_out);
/* algorithmic FLOPs of one forward per trajectory: (a) nominal = every conv tap counted, the reference's own
 * arithmetic (SURVEY.md §8d, 187 339 904 for the full net); (b) executed = taps that fall in the zero padding are
 * skipped by the kernels */
int edmp_unet_flops(edmp_ctx* ctx, double* nominal, double* executed);
/* FLOPs per trajectory of the DIRECT convolution with the taps that only ever meet zero padding removed (round 1's
 * "executed" figure, 122.0 MFLOP for the full-size net).  edmp_unet_flops' `executed` counts the MFMA work actually
 * issued, which is lower where the L = 2 / L = 4 convolutions run in Karatsuba form (wide.hip). */
int edmp_unet_flops_direct(edmp_ctx* ctx, double* direct);
/* Where the issued MFMA work of one forward runs (no reference counterpart; bench.py's roofline): FLOPs per trajectory issued on
 * the fp32 matrix pipe (edmp_unet_flops' `executed` minus the work of the layers that run in bf16x3 form) and on the bf16 matrix
 * pipe (csrc/bf3.hip: six exact bf16 partial products per fp32 product, fp32 accumulation; 0 with EDMP_BF16X3=0). */
int edmp_unet_flops_pipes(edmp_ctx* ctx, double* f32_issued, double* bf16_issued);

/* ---- guide: IntersectionVolumeGuide -------------------------------------------------------------------- */
/* replaces IntersectionVolumeGuide.__init__/define_link_information/define_obstacles
 * (lib/guide.py:13-43, 243-342, 118-158).  obstacle_config (no,10) f64 rows [xyz, quat xyzw, full extents];
 * clearance/expansion (G,T) f64 = one row per distinct guide class; builds the device table of inflated obstacle
 * AABBs for every (class, t in 0..T).  link_half_extents (9,3) f32; dh (7,4) f32 rows [a,d,cos(alpha),sin(alpha)];
 * static_frames (9,3,4) f32. */
int edmp_scene_set(edmp_ctx* ctx, const double* obstacle_config, int n_obstacles, const double* clearance,
                   const double* expansion, int n_classes, int T, const float* link_half_extents, const float* dh,
                   const float* static_frames);
/* per-row parameters (infer_serial.py:56-91): class index, method (0 iv / 1 sv), grad_norm (0/1),
 * guidance_schedule (B,T) f64 */
int edmp_rows_set(edmp_ctx* ctx, const int32_t* row_class, const float* method, const double* grad_norm,
                  const double* guidance_schedule, int B, int T);
/* copy the obstacle AABB table entry (class, t): out (no, 6) f32 = [min xyz, max xyz] (parity checks) */
int edmp_scene_read_aabbs(edmp_ctx* ctx, int cls, int t, float* out_host);
/* replaces IntersectionVolumeGuide.cost (lib/guide.py:354-395): joints (n,7,L) f32 -> volumes (n,L,9*no) f32.
 * row r uses class row_class[r] if use_row_class else class 0; t = 0 means no inflation. */
int edmp_guide_cost_dev(edmp_ctx* ctx, const float* joints_dev, int n, int L, int t, int use_row_class,
                        float* volumes_dev);
/* replaces swept_volume_cost (lib/guide.py:473-537): joints (n,7,L) f32 interior waypoints, start/goal (7,) f32
 * -> volumes (n, L+1, 9*no) f32 */
int edmp_guide_swept_cost_dev(edmp_ctx* ctx, const float* joints_dev, int n, int L, int t, int use_row_class,
                              const float* start, const float* goal, float* volumes_dev);
/* replaces get_gradient (lib/guide.py:597-635) incl. the whole-batch norm mixing: joints (B,7,L) f64 (already
 * clipped) -> gradient (B,7,L) f64.  sumsq_dev (optional, may be NULL) receives sum(g^2) (f64) before mixing. */
int edmp_guide_gradient_dev(edmp_ctx* ctx, const double* joints_dev, int B, int L, const double* start,
                            const double* goal, int t, double* grad_dev, double* sumsq_dev);
/* replaces the volume part of choose_best_trajectory (lib/guide.py:637-653): X (B,7,N) f64 -> per-row t=0 swept
 * volume (B,) f32; the argmin (first on ties) is written to *best_index (host, synchronises) if not NULL */
int edmp_row_swept_volumes_dev(edmp_ctx* ctx, const double* X_dev, int B, int N, const double* start,
                               const double* goal, float* volumes_dev, int* best_index);
/* torch.argmin over n f32 values on the device, as choose_best_trajectory uses it (lib/guide.py:650): first index of the
 * minimum; NaN counts as the smallest value (the first NaN wins).  The selection step of edmp_row_swept_volumes_dev. */
int edmp_argmin_dev(edmp_ctx* ctx, const float* v_dev, int n, int* index_host);

/* ---- sphere signed-distance guide (csrc/sdf.hip) --------------------------------------------------------------------- */
/* A third guidance method beside iv / sv, with no live counterpart in the reference (its sphere / SDF loss sits only in the vendored
 * mpinets/loss.py:47-94, mpinets/geometry.py:238-288, 456-507; its smoothness_cost, lib/guide.py:670-677, is never called).  An SDF row
 * pushes a sphere model of the arm away from the TRUE obstacle primitives of the success check (oriented boxes; cylinders where
 * edmp_scene_set_shapes says so) and, optionally, pulls consecutive waypoints together:
 *   cost = sum_{w=1..L} sum_s max(0, m - d(w, s)) + smoothness * sum_{w=0..L} ||q_{w+1} - q_w||^2,
 *   d(w, s) = min_o sdf_o(centre of sphere s at waypoint w) - radius_s,  m = margin[row][t - 1] for t >= 1 and 0 at t = 0,
 * over the padded chain start, L interior waypoints, goal (the smoothness sum is the FULL chain; lib/guide.py:670-677 drops both end
 * differences).  Arithmetic in f32; the formulas and the sub-gradient conventions are stated at the top of csrc/sdf.hip.
 *
 * edmp_sdf_set, after edmp_rows_set on a single-scene guide (a scene batch is refused with EDMP_ERR_STATE; it takes its table from
 * edmp_scene_batch_set_sdf below): spheres (n,5) f32 rows
 * [link 0..8, centre xyz in the link-box frame, radius > 0], 1 <= n <= EDMP_MAX_SPHERES; sdf_row (B,) int32 0/1; margin (B,T) f64 and
 * smoothness (B,) f64, finite and >= 0; B and T those of edmp_rows_set.  Rows with sdf_row = 1 keep method 0 in edmp_rows_set's table;
 * in edmp_guide_gradient_dev, the teacher-forced steps and the device loops their raw gradient and sum g^2 are written by
 * sdf_guide_kernel after the volume kernel, everything downstream (norm mixing, schedule, update) is unchanged.  With no such row
 * nothing else is launched and every result is what it was.  The table belongs to the rows: a later edmp_rows_set drops it. */
int edmp_sdf_set(edmp_ctx* ctx, const float* spheres, int n_spheres, const int32_t* sdf_row, const double* margin,
                 const double* smoothness, int B, int T);
/* cost (f64 sum of the f32 terms) and minimum clearance min_{w = 0..L+1, s} d(w, s) of EVERY row, SDF row or not: joints (n,7,L) f64 on
 * the device (not clipped), start / goal (7,) f64 host, cost_dev / clearance_dev (n,) f64 on the device.  t = 0: any n, margin 0, and
 * the smoothness weight of row r only when n is the bound row count (else 0); t >= 1: n must be the bound row count.  Ends a segmented
 * run like edmp_guide_gradient_dev (the start / goal pair is replaced).  Does not synchronise. */
int edmp_sdf_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int L, int t, const double* start, const double* goal,
                      double* cost_dev, double* clearance_dev);
/* Self-clearance term of the SDF rows, on the same sphere model (centres in f32 as above): for the sphere pairs (s, u) with
 * pair_mask[link_s][link_u] == 1, link_s < link_u,
 *   self(r) = weight[r] * sum_{w=1..L} sum_{(s,u)} max(0, m - d(w; s, u)),  d = ||c_s - c_u|| - radius_s - radius_u,
 *   m = self_margin[r][t - 1] for t >= 1 and 0 at t = 0,
 * interior waypoints only; the gradient and the sub-gradient conventions are stated at the top of csrc/sdf.hip.  edmp_sdf_set_self comes
 * after edmp_sdf_set or edmp_scene_batch_set_sdf (EDMP_ERR_STATE without a sphere table): pair_mask (host, 81 int32 = (9,9) row-major,
 * entries above the diagonal 0 or 1, the others not read; the links' spheres are paired in the order of the link-sorted table),
 * weight (n,) and self_margin (n,T) f64, finite and >= 0, n = the bound rows (B, or S*B scene after scene) and T those of edmp_rows_set.
 * A weight > 0 on a row that is not an SDF row is refused; the message names the row (and the scene, in a batch).  Every check comes
 * before anything is changed.  In the gradient paths sdf_self_kernel runs after sdf_guide_kernel over the rows whose weight is > 0, adds
 * the term's gradient to those rows' raw gradient and rewrites their sum g^2; with no such row nothing is launched, and a row outside
 * the list keeps the bits it had.  Bumps the context's epoch and synchronises, as edmp_sdf_set.  The term belongs to the sphere table: a
 * later edmp_sdf_set / edmp_scene_batch_set_sdf / edmp_rows_set drops it. */
int edmp_sdf_set_self(edmp_ctx* ctx, const int32_t* pair_mask, const double* weight, const double* self_margin, int n, int T);
/* the report of the term for EVERY row: element (r, j, w) of the L interior waypoints at joints_dev[(r*7 + j)*ldw + off + w], f64 on the
 * device (not clipped), 1 <= L <= 62, off + L <= ldw; cost_dev (n,) f64 = self(r), clearance_dev (n,) f64 = the minimum d over interior
 * waypoints and masked sphere pairs, +inf when the mask selects no pair.  t = 0: any n, margin 0, and the weight of row r only when n
 * is the bound row count (else 1: the bare hinge sum); t >= 1: n must be the bound row count.  Needs edmp_sdf_set_self (EDMP_ERR_STATE
 * without).  It replaces no start / goal pair and does NOT end a segmented run.  Argument errors come before any device call.  Does not
 * synchronise. */
int edmp_sdf_self_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int ldw, int off, int L, int t, double* cost_dev,
                           double* clearance_dev);
/* Tool-pose goal term of the SDF rows (arithmetic in f32; the formulas are stated at the top of csrc/sdf.hip): with
 * (R_w | p_w) = T_7(q_w) . tool, the joint-7 frame of the modified-DH chain times the tool frame, and (R* | p*) the target of the row's scene,
 *   goal(r) = weight[r] * sum_{w=1..L} rho_r(w) * (||p_w - p*||^2 + rotation[r] * (3 - tr(R*^T R_w))),
 *   rho_r(w) = max(0, w - L + window[r]) / window[r]   (a linear ramp over the last window[r] waypoints, 1 at w = L),
 * interior waypoints only, no dependence on t or on the obstacles.  edmp_sdf_set_goal comes after edmp_sdf_set or
 * edmp_scene_batch_set_sdf (EDMP_ERR_STATE without a sphere table), on a single-scene guide (S = 1) or a scene batch of S scenes:
 * weight (n,) and rotation (n,) f64, finite and >= 0; window (n,) int32 >= 1; n = the bound rows (B, or S*B scene after scene); tool
 * (12,) f64 = row-major 3 x 4 [R | p], one for the whole batch; target (S,12) f64 = each scene's [R* | p*], or NULL = the pose of the
 * scene's goal configuration: then every start / goal upload (the gradient, the loops, the swept-volume and SDF reports) also computes
 * T_7(goal_s) . tool on the host in f64 and uploads it in the same stream order.  Rotations must be orthonormal to 1e-6.  A weight > 0
 * on a row that is not an SDF row is refused; the message names the row (and the scene, in a batch).  Every check comes before anything
 * is changed.  In the gradient paths sdf_goal_kernel runs after sdf_guide_kernel and sdf_self_kernel over the rows whose weight is > 0
 * (one wave per row), adds the term's gradient to their raw gradient and rewrites their sum g^2; with no such row nothing is launched
 * and a row outside the list keeps the bits it had.  Bumps the context's epoch and synchronises, as edmp_sdf_set.  The term belongs to
 * the sphere table: a later edmp_sdf_set / edmp_scene_batch_set_sdf / edmp_rows_set drops it. */
int edmp_sdf_set_goal(edmp_ctx* ctx, const double* weight, const double* rotation, const int32_t* window, const double* tool,
                      const double* target, int n);
/* the report of the term for EVERY row, laid out as edmp_sdf_self_rows_dev takes them (not clipped), four (n,) f64 device outputs:
 * cost_dev = goal(r); distance_dev = ||p_L - p*|| in metres and angle_dev = the rotation angle between R_L and R* in radians, both at
 * the last handed column; min_distance_dev = the smallest ||p_w - p*|| over the handed columns.  t = 0: any n on a single-scene guide,
 * with weight 1, rotation 1 and window L when n is not the bound row count; t >= 1: n must be the bound row count (t changes nothing
 * else).  On a scene batch n is the bound row count and row r reads scene r / B's target.  Needs edmp_sdf_set_goal, and with derived
 * targets a start / goal upload since (EDMP_ERR_STATE without).  It replaces no start / goal pair and does NOT end a segmented run.
 * Argument errors come before any device call.  Does not synchronise. */
int edmp_sdf_goal_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int ldw, int off, int L, int t, double* cost_dev,
                           double* distance_dev, double* angle_dev, double* min_distance_dev);
/* Swept-clearance term of the SDF rows (arithmetic in f32; the formulas are stated at the top of csrc/sdf.hip): the obstacle hinge of
 * edmp_sdf_set at the configurations between the waypoints that the success check tests.  With K = substeps[r], over the padded chain
 * w = 0..L+1 (start, the L interior waypoints, goal) and q(w, k) = (1 - k/K) q_w + (k/K) q_{w+1},
 *   sweep(r) = weight[r] * sum_{w=0..L} sum_{k=1..K-1} sum_s max(0, m_r(t) - d(q(w, k), s)),
 * d the obstacle part's clearance of sphere s and m_r(t) the row's own margin schedule (0 at t = 0).  The gradient is taken with respect
 * to the interior waypoints: an active hinge at q(w, k) weighs on waypoint w with 1 - k/K and on waypoint w + 1 with k/K; the parts of
 * the two end segments that belong to start and goal are dropped.  edmp_sdf_set_sweep comes after edmp_sdf_set or
 * edmp_scene_batch_set_sdf (EDMP_ERR_STATE without a sphere table): weight (n,) f64 finite and >= 0, > 0 only on SDF rows; substeps (n,)
 * int32 with 2 <= substeps <= EDMP_MAX_SWEEP_SUBSTEPS wherever the weight is > 0 (elsewhere a value outside that range stands for "no
 * interpolant"); n = the bound rows (B, or S*B scene after scene).  A refusal names the row (and the scene, in a batch) and comes before
 * anything is changed.  In the gradient paths sdf_sweep_kernel runs after sdf_guide_kernel, sdf_self_kernel and sdf_goal_kernel over the
 * rows whose weight is > 0 (one workgroup per row), adds the term's gradient to their raw gradient and rewrites their sum g^2; with no
 * such row nothing is launched and a row outside the list keeps the bits it had.  Bumps the context's epoch and synchronises, as
 * edmp_sdf_set.  The term belongs to the sphere table: a later edmp_sdf_set / edmp_scene_batch_set_sdf / edmp_rows_set drops it. */
int edmp_sdf_set_sweep(edmp_ctx* ctx, const double* weight, const int32_t* substeps, int n);
/* the report of the term for EVERY row: the arguments of edmp_sdf_rows_dev / edmp_scenes_sdf_rows_dev (the same addressing of the L
 * interior waypoints, not clipped) plus substeps.  cost_dev (n,) f64 = sweep(r), the hinge terms summed in f64; clearance_dev (n,) f64 =
 * the smallest clearance over the interpolants of all L + 1 segments (+inf where a row has none).  substeps = 0: the bound rows' own
 * weights and substeps (needs edmp_sdf_set_sweep, n = the bound rows; t >= 1 reads their margin schedules); substeps in
 * 2..EDMP_MAX_SWEEP_SUBSTEPS: weight 1 and that K on any n rows, at t = 0 only.  The start / goal pairs go into a block of the term's
 * own: the calls replace no pair of the guide and do NOT end a segmented run.  Argument errors come before any device call.  They
 * synchronise the stream (the pairs are read from the caller's arrays). */
int edmp_sdf_sweep_rows_dev(edmp_ctx* ctx, const double* joints_dev, int n, int L, int t, const double* start, const double* goal, int substeps,
                            double* cost_dev, double* clearance_dev);
int edmp_scenes_sdf_sweep_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int t, const double* starts, const double* goals,
                                   int substeps, double* cost_dev, double* clearance_dev);
/* Repair of finished rows: projected descent on the swept SDF cost, one 256-thread workgroup per listed row for the whole run of the row
 * (sdf_repair_kernel; no launch per iteration).  X_dev (n, 7, N) f64 is updated IN PLACE: the interior columns 1..N-2 are the L = N - 2
 * waypoints, start / goal form the padded ends (columns 0 and N-1 are never read as joints and never written).  Per call: margin m >= 0,
 * smoothness lambda >= 0, substeps K in 1..EDMP_MAX_SWEEP_SUBSTEPS, iters n in 0..EDMP_MAX_REPAIR_ITERS, step eta > 0, max_step delta > 0.
 * Evaluation E(x), all arithmetic in f32 in the statements of the SDF kernels (csrc/sdf.hip):
 *   q_w = (float) clip(x_w) for w = 1..L, q_0 / q_{L+1} the f32 casts of start / goal;
 *   q(w, k) = fmaf(f, q_{w+1}, (1 - f) q_w), f = (float)k / (float)K, w = 0..L, k = 0..K-1 (q(w, 0) = q_w), and the goal q_{L+1};
 *   H = sum max(0, m - d(c, s)) over every such configuration c except start and goal and over every sphere s - the obstacle part's hinge
 *       of edmp_sdf_set at margin m plus the sweep term at weight 1 and the same margin, with their sub-gradient conventions;
 *   S = lambda * sum_{w=0..L} ||q_{w+1} - q_w||^2;   g = grad (H + S) with respect to the interior waypoints (an active hinge at q(w, k)
 *       sends (1 - f) J^T n to waypoint w and f J^T n to waypoint w + 1; what would land on start or goal is dropped);
 *   cost = H + S with the hinge terms summed in f64; clearance = min d over ALL of the configurations, start and goal included.
 * Iteration, for i = 0, 1, ...: evaluate E(x_i); if no hinge term is active (H = 0) or i = n, stop with iterations = i; otherwise every
 * interior element moves in f64 by delta = min(max(-eta * (double)g, -max_step), max_step), x <- min(max(x + delta, qlo_j), qhi_j) with
 * the joint limits of the robot table.  So a row that is clear by m at every tested configuration keeps its bits (iterations = 0),
 * iters = 0 is a pure report, and there are at most n + 1 evaluations.  Outputs, written for the listed rows only: cost_dev (n, 2) and
 * clearance_dev (n, 2) f64 = evaluation 0 | the last evaluation; iterations_dev (n,) int32.  A row with a non-finite element in its
 * interior columns is not touched: iterations = -1 and NaN in both pairs.  rows_host: n_rows row indices (host, any order, no
 * duplicates), or NULL = every row (n_rows is ignored); a row outside the list keeps its bits in X and its report entries are not
 * written.  Rows are independent (no whole-batch norm, no atomics, one order of every sum).  The self-clearance and goal terms are NOT
 * part of the repaired cost.  edmp_sdf_repair_rows_dev needs a single-scene guide with a sphere table (edmp_sdf_set), any n >= 1;
 * edmp_scenes_sdf_repair_rows_dev a bound scene batch with the table of edmp_scene_batch_set_sdf, X (S*B, 7, N), each row against its
 * own scene's primitives, kinds and pair.  Refusals (3 <= N <= 64, K and iters in range, margin and smoothness finite and >= 0, step and
 * max_step finite and > 0, start / goal finite, rows in range and without duplicates) come before any device call, name the offending
 * value, and leave X and the context untouched.  The start / goal pairs go into a block of the call's own: the calls replace no pair of
 * the guide, read nothing of the sampler and do NOT end a segmented run.  They synchronise the stream (pairs and list are read from the
 * caller's arrays). */
int edmp_sdf_repair_rows_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const double* start, const double* goal, const int32_t* rows_host,
                             int n_rows, int substeps, int iters, double margin, double smoothness, double step, double max_step,
                             double* cost_dev, double* clearance_dev, int32_t* iterations_dev);
int edmp_scenes_sdf_repair_rows_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const double* starts, const double* goals,
                                    const int32_t* rows_host, int n_rows, int substeps, int iters, double margin, double smoothness, double step,
                                    double max_step, double* cost_dev, double* clearance_dev, int32_t* iterations_dev);

/* ---- plan success: the reference's simulator check, restated geometrically ------------------------------------ */
/* The guide sees every obstacle as a box (cylinders enter as (r, r, h) boxes, datasets/load_test_dataset.py:136-139) but the
 * reference's success check spawns TRUE cylinders (RobotEnvironment.spawn_collision_cylinders, lib/environment.py:249-268:
 * radius = config[7], height = config[8], axis = local z).  kind[i] = 0 cuboid (default after edmp_scene_set) / 1 cylinder
 * for obstacle row i of the obstacle_config given to edmp_scene_set.  Only edmp_success_rows_dev reads it. */
int edmp_scene_set_shapes(edmp_ctx* ctx, const int32_t* kind, int n_obstacles);
/* stands for RobotEnvironment.benchmark_trajectory + check_collisions (lib/environment.py:632-680, 591-608), the success
 * tally of infer_serial.py:94-99,165-168, for EVERY row of a batch: X (B,7,N) f64 on the device; a row succeeds iff all its
 * waypoints lie inside the joint limits (:659-661) and none of the 9 link boxes (lib/guide.py:243-342, f64 modified-DH
 * poses) meets an obstacle - exact oriented-box test against cuboids, exact box / finite-cylinder test against cylinders -
 * at any waypoint or at any of `substeps` joint-space interpolated configurations per segment ((1 - s/S) q_i + (s/S) q_i+1,
 * s = 0..S-1; the last waypoint once).  pybullet itself is third-party and absent: a geometric stand-in, not the simulator.
 * dh_f64 (host, optional): (7,4) f64 rows [a, d, cos(alpha), sin(alpha)]; NULL widens the f32 table of edmp_scene_set.
 * Outputs (device, each optional): ok (B,) int32 0/1, first (B,) int32 = first colliding waypoint or -1, within (B,) int32
 * 0/1.  counts_host (optional, synchronises): [rows ok, rows within limits, rows collision-free, B]. */
int edmp_success_rows_dev(edmp_ctx* ctx, const double* X_dev, int B, int N, int substeps, const double* dh_f64, int32_t* ok_dev,
                          int32_t* first_dev, int32_t* within_dev, int32_t* counts_host);

/* ---- shortcutting of finished rows under the exact collision check (csrc/shortcut.hip) ------------------------------------------ */
/* The stage between repair and selection: one 256-thread workgroup per listed row for the whole run of the row (shortcut_rows_kernel; no
 * launch per candidate).  X_dev (n, 7, N) f64 is updated IN PLACE; columns 0 and N-1 are the pinned start and goal and are never written.
 * Per call: passes in 0..EDMP_MAX_SHORTCUT_PASSES, substeps K in 1..64, min_gain >= 0 [rad].  All arithmetic in f64, every operation of
 * the gain and of the piece rounded on its own (no fused multiply-add).  The rule, per row x:
 *   spans: s_0 = N - 1, s_{k+1} = (s_k + 1) / 2 (integer division), ending after the entry s = 2 (N = 50: 49, 25, 13, 7, 4, 2);
 *   for each pass p = 0..passes-1, for each span s in that order: i = 0, and while i + s <= N - 1, with j = i + s:
 *     gain = (sum_{m=i}^{j-1} |x_{m+1} - x_m|) - |x_j - x_i|, the norms over the seven joints (squares summed in joint order), the segment
 *       lengths summed in index order; if not gain > min_gain: i += 1 and nothing is tested;
 *     piece: y_m = x_i + ((double)(m - i) / (double)(j - i)) * (x_j - x_i) for m = i+1..j-1, y_i = x_i, y_j = x_j;
 *     test: every configuration of the piece strictly between waypoint i and waypoint j as edmp_success_rows_dev forms them - y_m itself
 *       and (1.0 - f) * y_m + f * y_{m+1}, f = (double)k / (double)K, k = 1..K-1, on every segment m = i..j-1 - against the scene's
 *       obstacles by that check's own test (nine link boxes, 15-axis test for boxes, clipped-polytope test for cylinders, touching counts);
 *     no hit: x_m <- y_m for m = i+1..j-1, the span (i, j) is logged, i = j; otherwise i += 1;
 *   a pass that accepts nothing ends the row (a further pass would repeat it); passes = 0 is a pure report.
 * So the joint path length never grows, waypoints only move to convex combinations of waypoints (the joint-limit flag cannot get worse),
 * and every configuration the success check tests on the output is either unchanged or was tested here: a row with first < 0 before has
 * first < 0 after.  A colliding row may become free, when its colliding part lies inside an accepted span.  Self-collision is NOT part
 * of THIS test (a joint-space chord can fold the arm; edmp_self_collision_rows_dev stays the check): it is part of the test of
 * edmp_shortcut_rows_self_dev and edmp_scenes_shortcut_rows_self_dev below.
 * Outputs, written for the listed rows only: accepted_dev (n,) int32 accepted spans, tested_dev (n,) int32 tested candidates (true counts,
 * not capped), length_dev (n, 2) f64 = the joint path length (the segment lengths summed in index order) before | after, spans_dev
 * (n, log_cap, 2) int32 = the first log_cap accepted (i, j) in order, the rest -1 (log_cap = 0: not read, may be NULL).  A row with a
 * non-finite element is not touched: accepted = -1, tested = 0, NaN lengths, a log of -1.  rows_host: n_rows row indices (host, any
 * order, no duplicates), or NULL = every row (n_rows is ignored); a row outside the list keeps its bits in X and its report entries are
 * not written.  dh_f64 as in edmp_success_rows_dev.  Rows are independent (no atomics, one order of every sum): a row's result depends
 * on the row and its scene alone.  edmp_shortcut_rows_dev needs a single-scene guide, any n >= 1; edmp_scenes_shortcut_rows_dev a bound
 * scene batch, X (S*B, 7, N), each row against its own scene's obstacles and kinds.  Refusals (3 <= N <= 64, K and passes in range,
 * min_gain finite and >= 0, log_cap >= 0, rows in range and without duplicates, null pointers) come before any device call, name the
 * offending value, and leave X, the outputs and the context untouched.  The calls read nothing of the sampler, replace no start / goal
 * pair and do NOT end a segmented run.  They synchronise the stream (the list is read from the caller's array). */
int edmp_shortcut_rows_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int substeps, int passes,
                           double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                           int32_t* spans_dev, int log_cap);
int edmp_scenes_shortcut_rows_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int substeps,
                                  int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev,
                                  double* length_dev, int32_t* spans_dev, int log_cap);
/* The same stage with the arm's own link boxes in the test: the rule above, with the step
 *     test: ... against the scene's obstacles by that check's own test, AND against the arm itself: at each of those configurations the
 *       boxes of every MASKED pair of links (a, b), a < b, by edmp_self_collision_rows_dev's test (f64 modified-DH poses, the 15-axis
 *       test, touching counts), the interpolants in the bits that check forms ((1.0 - f) * y_m + f * y_{m+1} as ONE fused multiply-add
 *       onto the rounded product f * y_{m+1}: what both checks compute);
 *     no obstacle hit and no masked pair overlapping: x_m <- y_m, the span is logged, i = j; otherwise i += 1.
 * pair_mask (host, 81 int32 = (9, 9) row-major) as in edmp_self_collision_rows_dev: pair (a, b), a < b, is tested iff pair_mask[a*9 + b]
 * == 1; those entries must be 0 or 1 (refused otherwise, naming the entry), entries on or below the diagonal are not read; ONE mask for
 * every row, in a scene batch too.  So, beside the guarantees above: a row that edmp_self_collision_rows_dev (same substeps, same mask,
 * same dh_f64) calls free before is free after - every configuration it tests on the output is unchanged or was tested here, in its
 * bits.  self_rejected_dev (n,) int32, written for the listed rows: the tested candidates that the obstacle test passed and the self test
 * rejected (a candidate hit by both counts in tested only); 0 for a row with a non-finite element.  tested counts candidates as before.
 * An all-zero mask is legal: the rule and the kernel of edmp_shortcut_rows_dev, self_rejected zero-filled for all n rows.  Otherwise
 * shortcut_rows_kernel<true>: the test's work items are (configuration, test) - the obstacle test, then one item per lower link with a
 * masked partner - under two flags per candidate (obstacle hit, self hit; an obstacle item is skipped only when the obstacle flag is up,
 * a self item when either is): deterministic, no atomics.  Everything else - outputs, the NaN row, rows_host, refusals before any device
 * call (pair_mask and self_rejected_dev must not be NULL), what the calls leave alone, the synchronisation - as above. */
int edmp_shortcut_rows_self_dev(edmp_ctx* ctx, double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int substeps, int passes,
                                double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev, double* length_dev,
                                int32_t* spans_dev, int log_cap, const int32_t* pair_mask, int32_t* self_rejected_dev);
int edmp_scenes_shortcut_rows_self_dev(edmp_ctx* ctx, double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int substeps,
                                       int passes, double min_gain, const double* dh_f64, int32_t* accepted_dev, int32_t* tested_dev,
                                       double* length_dev, int32_t* spans_dev, int log_cap, const int32_t* pair_mask,
                                       int32_t* self_rejected_dev);

/* ---- continuous collision certificate of finished rows (csrc/certify.hip, csrc/clearance.h) ------------------------------------ */
/* A check whose answer holds for EVERY configuration of the joint-space polyline of a row, not for a list of them: the success check and
 * the stages built on it test the waypoints and substeps - 1 interpolants per segment, and an obstacle thinner than their spacing can be
 * passed through unseen.  One 256-thread workgroup per listed row (certify_rows_kernel), X_dev (n, 7, N) f64, 2 <= N <= 64, read only.
 * All arithmetic in f64.  Off by default everywhere: no other entry point calls it.
 *   motion radii rho[l][j] (9 x 7, computed on the host from the tables the kernel is handed; radii_out, host, 63 doubles, receives them if
 *     not NULL): for link l riding joint frame k (link l for l < 7, else 6) and j <= k,
 *       rho[l][j] = sum_{i=j+1..k} sqrt(a_i^2 + d_i^2) + max over the 8 corners c = +-he_l of |p_l + S_l c|,   0 for j > k,
 *     (S_l | p_l) the link's static frame: turning joint j by dq moves every point of box l by at most |dq| rho[l][j].
 *   gap(box, obstacle): a lower bound on the Euclidean distance, positive only if the shapes are disjoint - the maximum over unit axes of
 *     the separation of the projections.  Box / box, in the 15-axis test's own R, A = |R| + 1e-12, t: the six face axes and the nine edge
 *     axes, each divided by its norm sqrt(1 - R[i][j]^2) and skipped where 1 - R[i][j]^2 < 1e-6.  Box / cylinder: the cylinder axis, the
 *     three box normals n against the cylinder's extent H |n.z| + r sqrt(1 - (n.z)^2), and the radial direction from the cylinder's axis
 *     line to the box centre (skipped where that distance is < 1e-9).
 *   item (segment w, link l), a = x_w, b = x_{w+1}: L = sum_j |b_j - a_j| rho[l][j].  An in-order walk of the binary tree over the segment
 *     with integer position pos in [0, 2^D) and a level: the interval [pos, pos + size), size = 2^(D - level), has the centre
 *     u = (2 pos + size) / 2^(D+1); the configuration there is the success check's interpolant fma(1 - u, a_j, u b_j); g = the minimum
 *     of gap over the row's scene's obstacles for the box of link l at it; reach = L size / 2^(D+1).  Then
 *       1. g - reach > margin + 1e-9: the interval is certified; min(g - reach) is kept; pos += size, level = D - ctz(pos);
 *       2. else, if the exact test (15-axis / clipped-polytope, touching counts) finds the box overlapping an obstacle here: the item ends
 *          with a hit at this u;
 *       3. else, if level == D or reach == 0: one undecided interval is counted (the first is remembered); advance as in 1;
 *       4. else level += 1.
 *     The walk takes at most 2^(D+1) - 1 evaluations.
 * Outputs, (n,) each, written for the listed rows only: verdict_dev int32 = 1 (hit) if any item hit, else 2 (undecided) if any item counted
 * an undecided interval, else 0 (free: no link box touches an obstacle anywhere on the polyline, and keeps more than bound > margin from
 * every obstacle); 3 (invalid) for a row with a non-finite element, for which nothing is evaluated.  segment_dev int32, fraction_dev f64
 * (= u, dyadic, exact), link_dev int32: the lexicographically smallest (segment, u, link) among the items' hits (verdict 1) or among the
 * items' first undecided intervals (verdict 2); -1, -1.0, -1 otherwise.  evaluations_dev, undecided_dev int32: sums over the items.
 * bound_dev f64: the minimum of g - reach over all accepted intervals, +inf if there is none.  Joint limits are not part of the
 * certificate.  No output depends on the order in which the items finish (integer minima and sums, an f64 minimum).
 * depth D in 0..10, margin finite and >= 0 [m].  rows_host: n_rows row indices (host, any order, no duplicates), or NULL = every row
 * (n_rows is ignored).  dh_f64 as in edmp_success_rows_dev.  edmp_certify_rows_dev needs a single-scene guide, any n >= 1;
 * edmp_scenes_certify_rows_dev a bound scene batch, X (S*B, 7, N), each row against its own scene's obstacles and kinds.  Refusals (N,
 * depth, margin, rows, null pointers) come before any device call and name the argument.  The calls replace nothing of the guide or the
 * sampler and do NOT end a segmented run.  They run on the context's stream and synchronise it. */
int edmp_certify_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int depth, double margin,
                          const double* dh_f64, int32_t* verdict_dev, int32_t* segment_dev, double* fraction_dev, int32_t* link_dev,
                          int32_t* evaluations_dev, int32_t* undecided_dev, double* bound_dev, double* radii_out);
int edmp_scenes_certify_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int depth,
                                 double margin, const double* dh_f64, int32_t* verdict_dev, int32_t* segment_dev, double* fraction_dev,
                                 int32_t* link_dev, int32_t* evaluations_dev, int32_t* undecided_dev, double* bound_dev, double* radii_out);

/* ---- time parameterisation of finished rows (csrc/timing.hip) ---------------------------------------------------- */
/* The stage after shortcutting, which the reference does not ship (it replays plans at constant velocity): the fastest rest-to-rest
 * motion ALONG the polyline of every row under joint velocity, joint acceleration and corner velocity-jump limits, and its samples at a
 * controller period.  X_dev (n, 7, N) f64, 2 <= N <= 64; vmax [rad/s], amax [rad/s^2], jump [rad/s] are host arrays of 7, finite and > 0.
 * All arithmetic in f64, every operation rounded on its own (no fused multiply-add), min(a, b) = b < a ? b : a.  The rule, per row x, with
 * the path parameter s in [0, N-1] and y = (ds/dt)^2:
 *   segment i = 0..N-2: d_i = x_{i+1} - x_i;  V_i = min_j vmax_j / |d_ij|, A_i = min_j amax_j / |d_ij| over the joints with d_ij != 0, in
 *     joint order.  d_i = 0 is a ZERO SEGMENT: it takes no time, has no V_i / A_i and hands y across unchanged.
 *   waypoint caps: c_0 = c_{N-1} = 0 (rest to rest); interior c_i = min(V_{i-1}^2, V_i^2, J_i^2), J_i = min_j jump_j / |d_ij - d_{i-1,j}|;
 *     terms with a zero denominator and the V of a zero segment are left out; nothing left = +inf (y stays finite: y_0 = 0 and every
 *     transfer adds a finite amount).
 *   forward pass:  y_0 = 0, y_{i+1} = min(c_{i+1}, y_i + 2 A_i), a zero segment min(c_{i+1}, y_i);
 *   backward pass: y_i = min(y_i, y_{i+1} + 2 A_i), a zero segment min(y_i, y_{i+1}).
 *   inside a non-zero segment, the optimum given its end values: accelerate at A_i, cruise at V_i, decelerate at A_i, with the peak
 *     p_i = min(V_i^2, (y_i + y_{i+1}) / 2 + A_i) and the phase times t_acc = max(0, (sqrt p_i - sqrt y_i) / A_i),
 *     t_dec = max(0, (sqrt p_i - sqrt y_{i+1}) / A_i), t_cru = max(0, 1 - (p_i - y_i) / (2 A_i) - (p_i - y_{i+1}) / (2 A_i)) / sqrt p_i;
 *     a zero segment has three zeros.  Waypoint times: T_0 = 0 and one running sum t += t_acc, t += t_cru, t += t_dec in index order,
 *     T_{i+1} = t; duration = T_{N-1}.
 *   limit_i: the constraint that binds waypoint i = the first index of the minimum among 0 = rest end, 1 = V_{i-1}^2, 2 = V_i^2,
 *     3 = J_i^2, 4 = y_{i-1} + 2 A_{i-1} with the forward pass's y_{i-1} (a zero segment: y_{i-1}), 5 = y_{i+1} + 2 A_i with the backward
 *     pass's y_{i+1}.  Both ends are 0.
 *   motion at time t < duration: segment i = the largest i <= N-2 with T_i <= t, tau = t - T_i;
 *     tau < t_acc:               sdot = sqrt y_i + A_i tau,            s = sqrt y_i * tau + (A_i / 2) tau^2
 *     else t2 = tau - t_acc < t_cru:  sdot = sqrt p_i,                  s = (p_i - y_i) / (2 A_i) + sqrt p_i * t2
 *     else t3 = t2 - t_cru:      sdot = sqrt p_i - A_i t3,             s = (1 - (p_i - y_{i+1}) / (2 A_i)) + (sqrt p_i * t3 - (A_i / 2) t3^2)
 *     sdot clamped to [0, sqrt p_i], s to [0, 1];  q = x_i + s (x_{i+1} - x_i),  qdot = (x_{i+1} - x_i) sdot.
 *     t >= duration: q = the goal column bit for bit, qdot = 0.
 *   samples: t_k = (double)k * period, k = 0..M-1.  count = 1 + the smallest k with (double)k * period >= duration (duration = 0: 1),
 *     saturated at INT32_MAX; samples at or past count - 1 hold the goal at rest.
 *   a row with a non-finite element is not timed: y, phase, times, duration and its samples are NaN, limit = -1, count = 0.
 * Consequences: |qdot_j| <= vmax_j everywhere and |qddot_j| <= amax_j inside segments; the velocity jump at waypoint i is
 * |d_ij - d_{i-1,j}| sqrt y_i <= jump_j; the path is the input polyline, so what the success, self-collision and shortcut stages said of
 * it holds for what is executed; collinear runs (what edmp_shortcut_rows_dev writes) carry no corner cap; a repeated waypoint is
 * conservative (the speed is handed across instead of optimised over), never unsafe.  y is the component-wise largest point of
 * {0 <= y_i <= c_i, |y_{i+1} - y_i| <= 2 A_i}: the time optimum on this path, zero-segment hand-over excepted.
 *
 * edmp_time_rows_dev (time_rows_kernel: one wave per row, four rows per workgroup, lane = waypoint) writes y (n, N), phase (n, N-1, 3) =
 * t_acc | t_cru | t_dec, times (n, N), duration (n,), limit (n, N) int32 and seg (n, N-1, 2) = A_i | p_i (0 | y_i on a zero segment): the
 * per-segment values the sampler needs, so that the sampler reads the limits nowhere else.  Does not synchronise.
 * edmp_sample_rows_dev (sample_rows_kernel: workgroup = listed row x 256 samples) takes X and that profile, rows_host = n_rows row
 * indices (host, any order, no duplicates) or NULL = every row (n_rows is ignored), period > 0 [s] and M in 1..EDMP_MAX_TIMED_SAMPLES,
 * and writes q, qdot (R, 7, M) f64 and count (R,) int32, R = n_rows (or n): slot k belongs to row rows[k]; nothing else is written.
 * count is the row's true count and may exceed M.  Synchronises (the list is read from the caller's array).
 * Both need a context only - no model, scene, guide or sampler - leave the epoch alone and do NOT end a segmented run.  Refusals (N, n,
 * limits, period, M, rows out of range or listed twice, null pointers) come before any device call and name the offending value. */
int edmp_time_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* vmax, const double* amax, const double* jump,
                       double* y_dev, double* phase_dev, double* times_dev, double* duration_dev, int32_t* limit_dev, double* seg_dev);
int edmp_sample_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* y_dev, const double* phase_dev,
                         const double* times_dev, const double* duration_dev, const double* seg_dev, const int32_t* rows_host, int n_rows,
                         double period, int M, double* q_dev, double* qd_dev, int32_t* count_dev);

/* ---- corner blends of finished rows: chosen under the exact collision check (csrc/blend.hip), timed and sampled (csrc/timing.hip) -- */
/* The stage after the one above, for a motion that may LEAVE the polyline by a bounded amount.  On the polyline every real corner carries
 * the velocity-jump cap and the arm all but stops there.  Here corner i is replaced by a parabolic blend: the quadratic Bezier curve with
 * the control points x_i - beta_i d_{i-1}, x_i, x_i + beta_i d_i, traversed at constant acceleration.  Notation as above: d_i = x_{i+1} -
 * x_i, Delta_i = d_i - d_{i-1}, V_i, A_i, J_i as in edmp_time_rows_dev, and K_i = min_j amax_j / |Delta_ij| over the joints with
 * Delta_ij != 0.  All arithmetic in f64, every operation rounded on its own (no fused multiply-add), min(a, b) = b < a ? b : a.
 *
 * 1. edmp_blend_rows_dev / edmp_scenes_blend_rows_dev choose beta (blend_rows_kernel: one 256-thread workgroup per listed row, thread =
 * (corner, configuration)).  X_dev (n, 7, N) f64, 2 <= N <= 64, is only read; vmax, amax, jump as above; deviation[7] [rad], finite and
 * > 0, the largest departure from the polyline per joint; reach in (0, 0.45], the largest beta; substeps K_b in 1..8; halvings H in 0..8.
 * Per interior waypoint i = 1..N-2, in this order:
 *   code 0, beta = 0: d_{i-1} = 0 or d_i = 0 (a zero segment beside it, a repeated waypoint included) or Delta_i = 0 in every joint.
 *   code 1 (not needed), beta = 0: not J_i^2 < min(V_{i-1}^2, V_i^2) - the corner cap does not bind there, and a blend would only
 *     shorten the straight parts beside it.
 *   otherwise beta0 = min(reach, min_j (4.0 * deviation_j) / |Delta_ij|) in joint order, and for h = 0..H with beta = beta0 * 2^-h:
 *     not (2.0 * beta) * K_i > J_i^2: code 2 (no gain: the blend's cap is no better than the jump cap), beta = 0, stop;
 *     the K_b + 1 configurations at u = (double)k / (double)K_b, k = 0..K_b:
 *       q_j(u) = x_ij + beta * ((u * u) * d_ij - ((1.0 - u) * (1.0 - u)) * d_{i-1,j}),  d_ij = x_{i+1,j} - x_ij, d_{i-1,j} = x_ij - x_{i-1,j},
 *     each tested against the row's own scene's obstacles and kinds by edmp_success_rows_dev's own test (nine link boxes, 15-axis test for
 *     boxes, clipped-polytope test for cylinders, touching counts);  no hit: code 3 (blended), this beta is kept, halved = h, stop.
 *   all H + 1 tries hit: code 4 (blocked), beta = 0.
 * Both ends are code 0, beta 0.  Outputs: beta_dev (n, N) f64, code_dev (n, N) int32, halved_dev (n, N) int32 (0 unless code 3),
 * tested_dev (n,) int32 = the configurations of the row's tries, K_b + 1 for every (corner, h) that reached the test.  A row with a
 * non-finite element is left alone: code -1, beta NaN, halved 0, tested 0.  rows_host: n_rows row indices (host, any order, no
 * duplicates), or NULL = every row (n_rows is ignored); the entries of a row outside the list are NOT written.
 * Guarantees: the blend of corner i runs from x_i - beta d_{i-1} to x_i + beta d_i and is tangent to both segments there; it departs from
 * the polyline by at most beta |Delta_ij| / 4 <= deviation_j in joint j (at u = 1/2; every point of the curve is a convex combination of
 * points of the two segments); beta <= reach <= 0.45 keeps neighbouring blends apart; every accepted blend was tested at its K_b + 1
 * configurations, both ends included, by the success check's own test - what lies between them is as untested as what lies between the
 * success check's own substeps.  Self-collision is NOT tested by these two (edmp_self_collision_rows_dev stays the check); it is by
 * edmp_blend_rows_self_dev and edmp_scenes_blend_rows_self_dev: stage 1 with one more condition on a try - at each of its K_b + 1
 * configurations no MASKED pair of link boxes (a, b), a < b, may overlap, by edmp_self_collision_rows_dev's test (touching counts).  A try
 * is kept iff neither test hits; all H + 1 tries hit, by whichever test: code 4.  pair_mask (host, 81 int32, entries above the diagonal
 * read, each 0 or 1, refused otherwise; ONE mask for every row and scene) as in edmp_self_collision_rows_dev.  self_hits_dev (n, N) int32,
 * written for the listed rows: the tries of corner i that the obstacle test passed and the self test rejected (a try hit by both is not
 * counted); 0 for a row with a non-finite element.  Codes, beta, halved and tested (K_b + 1 per try) as above.  An all-zero mask: the
 * kernel of edmp_blend_rows_dev, self_hits zero-filled for all n rows; otherwise blend_rows_kernel<true>, the items (configuration, test)
 * under two flags per tried corner as in edmp_shortcut_rows_self_dev.  Self-collision BETWEEN the tested configurations is as untested
 * as obstacle collision there.  dh_f64 as in
 * edmp_success_rows_dev.  edmp_blend_rows_dev needs a single-scene guide, any n >= 1; edmp_scenes_blend_rows_dev a bound scene batch,
 * X (S*B, 7, N).  They read nothing of the sampler, do NOT end a segmented run, and synchronise the stream.
 *
 * 2. edmp_time_blended_rows_dev times the blended path (time_rows_kernel's blended instantiation: one wave per row, lane = waypoint).  beta_dev (n, N)
 * as stage 1 wrote it: 0 <= beta_i <= 0.45, 0 at both ends and beside a zero segment.  The rule is edmp_time_rows_dev's with two changes:
 *   l_i = (1.0 - beta_i) - beta_{i+1}: the straight part of segment i, from s = beta_i to s = 1 - beta_{i+1} of it;
 *   c_i = min(V_{i-1}^2, V_i^2, beta_i > 0 ? (2.0 * beta_i) * K_i : J_i^2): on blend i the joint acceleration is y_i Delta_i / (2 beta_i);
 *   forward y_{i+1} = min(c_{i+1}, y_i + (2.0 * A_i) * l_i), backward y_i = min(y_i, y_{i+1} + (2.0 * A_i) * l_i), zero segments as above;
 *   p_i = min(V_i^2, (y_i + y_{i+1}) / 2 + A_i * l_i);  t_acc, t_dec as above,  t_cru = max(0, l_i - (p_i - y_i) / (2 A_i) - (p_i -
 *     y_{i+1}) / (2 A_i)) / sqrt p_i;
 *   blend i is crossed at the constant path speed sqrt y_i in the time b_i = (2.0 * beta_i) / sqrt y_i (beta_i = 0: 0); a blended corner
 *     has non-zero neighbours and l >= 0.1, so y_i > 0 there;
 *   one running sum in the order line 0 (t_acc, t_cru, t_dec), blend 1, line 1, ...: times[i] = (the sum entering blend i, the sum leaving
 *     it); times[0] = (0, 0); duration = the sum after line N-2;
 *   limit_i as above, candidate 3 being the corner's cap: jump cap or blend acceleration cap, candidates 4 and 5 with (2 A) l.
 * Outputs: y (n, N), phase (n, N-1, 3), times (n, N, 2), duration (n,), limit (n, N) int32, seg (n, N-1, 2) = A_i | p_i, blend (n, N) =
 * b_i.  A row with a non-finite element of X or beta is not timed (NaN, limit -1).  With beta = 0 everywhere l_i = 1.0, (2 A_i) 1.0 and
 * A_i 1.0 are exact: y, phase, duration, limit and seg have edmp_time_rows_dev's bits, and times[i] = (T_i, T_i).  Consequences: the
 * velocity is continuous at a blended corner; |qdot_j| <= vmax_j everywhere, |qddot_j| <= amax_j on straight parts and on blends; y is
 * the component-wise largest point of {0 <= y_i <= c_i, |y_{i+1} - y_i| <= 2 A_i l_i}.  Does not synchronise.
 *
 * 3. edmp_sample_blended_rows_dev samples that motion (sample_rows_kernel's blended instantiation: workgroup = listed row x 256 samples); rows_host,
 * period, M, count, the goal's bits at rest at and past the duration and the NaN row as in edmp_sample_rows_dev.  At t < duration: the
 * flat times array F (2 N values) gives the starts of the 2 N - 3 pieces: piece p starts at F[p + 1]; p even is the straight part of
 * segment i = p / 2, p odd is blend i = (p + 1) / 2; the piece is the largest p with F[p + 1] <= t, tau = t - F[p + 1].
 *   straight part: s and sdot from the closed-form quadratic of the phase as above, with l_i in the place of 1 in the third phase, s
 *     clamped to [0, l_i];  q = x_i + (beta_i + s) * d_i,  qdot = d_i * sdot;
 *   blend: u = (tau * sqrt y_i) / (2.0 * beta_i) clamped to [0, 1];  q as in stage 1;  qdot_j = sqrt y_i * ((1.0 - u) * d_{i-1,j} + u * d_ij).
 * With beta = 0 everywhere q, qdot and count have edmp_sample_rows_dev's bits.  Synchronises.
 * Stages 2 and 3 need a context only, leave the epoch alone and do NOT end a segmented run.  Refusals of all four (N, n, limits,
 * deviation, reach, substeps, halvings, period, M, rows out of range or listed twice, null pointers, the wrong kind of bound guide) come
 * before any device call and name the offending value. */
int edmp_blend_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, const double* vmax,
                        const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                        const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev);
int edmp_scenes_blend_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows,
                               const double* vmax, const double* amax, const double* jump, const double* deviation, double reach,
                               int substeps, int halvings, const double* dh_f64, double* beta_dev, int32_t* code_dev,
                               int32_t* halved_dev, int32_t* tested_dev);
int edmp_blend_rows_self_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, const double* vmax,
                             const double* amax, const double* jump, const double* deviation, double reach, int substeps, int halvings,
                             const double* dh_f64, double* beta_dev, int32_t* code_dev, int32_t* halved_dev, int32_t* tested_dev,
                             const int32_t* pair_mask, int32_t* self_hits_dev);
int edmp_scenes_blend_rows_self_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows,
                                    const double* vmax, const double* amax, const double* jump, const double* deviation, double reach,
                                    int substeps, int halvings, const double* dh_f64, double* beta_dev, int32_t* code_dev,
                                    int32_t* halved_dev, int32_t* tested_dev, const int32_t* pair_mask, int32_t* self_hits_dev);
int edmp_time_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* vmax,
                               const double* amax, const double* jump, double* y_dev, double* phase_dev, double* times_dev,
                               double* duration_dev, int32_t* limit_dev, double* seg_dev, double* blend_dev);
int edmp_sample_blended_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const double* beta_dev, const double* y_dev,
                                 const double* phase_dev, const double* times_dev, const double* duration_dev, const double* seg_dev,
                                 const int32_t* rows_host, int n_rows, double period, int M, double* q_dev, double* qd_dev,
                                 int32_t* count_dev);

/* ---- self-collision of every row (csrc/selfcol.hip) ------------------------------------------------------------- */
/* Stands for the `self_collision` metric of the reference's evaluation package (mpinets/metrics.py:278-292, 351-361; a plan with
 * self-collision counts as a physical violation, :505), which asks robofin / pybullet - both absent: like the success check a geometric
 * stand-in, exact on the 9 link boxes.  X (n,7,N) f64 on the device, N >= 2, 1 <= substeps <= 64.  Row r is self-colliding at
 * configuration c - the success check's configurations: every waypoint plus substeps - 1 joint-space interpolants per segment, the same
 * interpolation expression, nc = (N - 1) * substeps + 1 - if the boxes of any MASKED pair of links overlap there: f64 modified-DH poses,
 * static frames and half extents of the bound guide's robot, the 15-axis separating-axis test of the success check, touching counts as
 * overlap.  pair_mask (host, 81 int32 = (9,9) row-major): pair (a, b), a < b, is tested iff pair_mask[a*9 + b] == 1; those entries must
 * be 0 or 1, entries on or below the diagonal are not read; an all-zero mask is legal and gives -1 everywhere.  (The link boxes are AABBs
 * of meshes, neighbouring links overlap by construction: franka.self_collision_pairs() masks the pairs whose joint frames lie at least 3
 * apart.)  dh_f64 as in edmp_success_rows_dev.
 * Outputs (device, each optional): first (n,) int32 = waypoint index c / substeps of the first colliding configuration, or -1;
 * pair (n,) int32 = a*9 + b of the first masked pair in row-major order that overlaps at THAT configuration, or -1.  Both come from one
 * integer minimum over the key c*81 + a*9 + b: deterministic, and a row's answer depends on the row alone.
 * Needs a bound guide for the robot tables - a single-scene guide or a scene batch alike (EDMP_ERR_STATE without one); it reads nothing
 * of the scene, the rows or the sampler, so one entry point serves both for any n >= 1, allocates nothing, leaves the epoch alone and
 * does NOT end a segmented run.  Argument errors (EDMP_ERR_ARG) come before any device call.  Does not synchronise. */
int edmp_self_collision_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, int substeps, const double* dh_f64,
                                 const int32_t* pair_mask, int32_t* first_dev, int32_t* pair_dev);

/* ---- result metrics of a whole batch (csrc/metrics.hip) ----------------------------------------------------------- */
/* stands for MetricsCalculator.path_length_metric and .smoothness_metric / .sparc (lib/metrics.py:32-45, 11-30, 47-125; end effector
 * through get_end_effector_transform, lib/guide.py:100-116: the seven joint rows and the three fixed rows of the modified-DH table),
 * for EVERY row of a batch instead of one trajectory on the host: X (B,7,N) f64 on the device, 3 <= N <= 129, sample time dt > 0
 * (SPARC at fs = 1 / dt with the reference's defaults padlevel 4, fc 10, amp_th 0.05).  out (4,B) f64 on the device: joint path length,
 * end-effector path length, joint SPARC, end-effector SPARC.  A row whose speed profile holds a NaN or an infinity gets SPARC = NaN
 * (the reference raises there); its path lengths follow IEEE.  All f64, every sum in one fixed order: bit-identical between runs and
 * independent of B and of the row's position.  Needs a context only - no scene, no guide - so it also serves the S*B rows of a scene
 * batch in one call.  dh_f64 (host, optional): (7,4) f64 rows [a, d, cos(alpha), sin(alpha)]; NULL = the Franka table of lib/guide.py:29-35.
 * Does not synchronise. */
int edmp_metrics_rows_dev(edmp_ctx* ctx, const double* X_dev, int B, int N, double dt, const double* dh_f64, double* out_dev);
/* choose_best_trajectory's arg-min (lib/guide.py:637-653) widened by the rule of the reference's IK-goal filter (infer_serial.py:119-129:
 * keep everything within volume_trust_region of the minimum, then take the nearest): volumes (B,) f32 and key (B,) f64 on the device.
 * m = edmp_argmin_dev's index (first minimum, NaN is the smallest).  If volumes[m] is NaN the answer is m.  Otherwise the candidates are
 * the rows with (double)v_b < (double)v_m + trust_region and the answer is the candidate with the smallest FINITE key, first index on
 * ties; m if no candidate has a finite key.  *index_host is written on the host (synchronises). */
int edmp_select_row_dev(edmp_ctx* ctx, const float* volumes_dev, const double* key_dev, int B, double trust_region, int* index_host);

/* ---- sampler: Diffusion ------------------------------------------------------------------------------ */
/* replaces Diffusion.__init__/schedule_variance (diffusion/diffusion.py:10-20, 37-49) */
int edmp_sampler_init(edmp_ctx* ctx, int T, double variance_thresh);
int edmp_sampler_read_schedule(edmp_ctx* ctx, double* beta, double* alpha, double* alpha_bar);
/* the `condition` argument of denoise_guided / denoise (diffusion.py:305-307, 347-349): pin the first / last waypoint to
 * start / goal (default on; the reference driver always passes True) */
int edmp_sampler_set_condition(edmp_ctx* ctx, int on);
/* replaces p_sample_using_posterior (diffusion.py:116-135) with the noise draw z made explicit.
 * X (B,C,N) f64 updated in place.  zero_row0: apply quirk Q3 (row 0 of z zeroed when t == 1). */
int edmp_psample_dev(edmp_ctx* ctx, double* X_dev, const float* eps_dev, const double* z_dev, int B, int C, int N,
                     int t, int zero_row0);
/* One reverse step of denoise_guided (diffusion.py:314-349) split at the only cross-row coupling:
 *   step_a: eps = UNet(f32(X), t); X <- posterior(X, eps, z); if guided(t): g = raw gradient(clip(X[:, :, 1:-1])),
 *           partial sum(g^2) -> device scalar.
 *   step_b: if guided(t): X[:, :, 1:-1] -= sched[:, t-1] * mix(g, ||g||); X[:, :, 0] = start; X[:, :, -1] = goal.
 * Between the two a multi-GPU caller may all-reduce edmp_sumsq_ptr_dev() (one f64).  Optional outputs (NULL to
 * skip): eps_out_dev (B,C,N) f32, xpost_out_dev (B,C,N) f64, grad_out_dev (B,C,N-2) f64 (mixed gradient). */
int edmp_step_a_dev(edmp_ctx* ctx, double* X_dev, const double* z_dev, int B, int t, const double* start,
                    const double* goal, int zero_row0, float* eps_out_dev, double* xpost_out_dev);
int edmp_step_b_dev(edmp_ctx* ctx, double* X_dev, int B, int t, const double* start, const double* goal,
                    double* grad_out_dev);
double* edmp_sumsq_ptr_dev(edmp_ctx* ctx);
/* replaces Diffusion.denoise_guided (diffusion.py:300-356): noise (T+1,B,C,N) f64 on device, noise[0] = initial
 * draw, noise[1 + T - t] = draw of step t.  X_out (B,C,N) f64.  guided = 0 runs the unguided loop
 * (Diffusion.denoise, diffusion.py:253-278, batched).  t_stop: run steps T..t_stop+1 (0 = all).
 * zero_row0: this shard holds global row 0 (quirk Q3). */
int edmp_denoise_guided_dev(edmp_ctx* ctx, const double* noise_dev, int B, const double* start, const double* goal,
                            int guided, int t_stop, int zero_row0, double* X_out_dev);

/* The same loop in segments (steps t_hi .. t_lo+1), for callers that produce the noise stream while the GPU works:
 * init != 0 starts a run at t_hi = T (noise_dev[0] is the X_T draw, then one (B,C,N) draw per step; a run that begins below T is
 * started by edmp_sampler_seed_dev instead, see below); init == 0 continues
 * from the state kept in the context (noise_dev[0] is the draw of step t_hi) and performs no host synchronisation.
 * X_out_dev may be NULL except for the last segment.  Used by Diffusion.denoise_guided to overlap NumPy's RandomState
 * (the reference's noise contract, ~0.85 s per 1024-row scene on the host) with the denoising itself.
 * The context remembers where the run stands: a segment that returns with t_lo > 0 leaves a run in progress at step t_lo, and
 * a continuing segment must bring t_hi == that step, the same B, and a context whose model, scene, rows and sampler tables are
 * those of the previous segment; anything else is refused with EDMP_ERR_STATE (the message names the expected and the given
 * step) and launches nothing.  A run ends when a segment reaches t_lo == 0, and is ended by every other loop entry point
 * (edmp_denoise_guided_dev / _rng_dev / edmp_denoise_scenes_dev), by the teacher-forced steps, edmp_guide_gradient_dev,
 * edmp_guide_swept_cost_dev, edmp_row_swept_volumes_dev, edmp_scenes_swept_volumes_dev, edmp_sdf_rows_dev and edmp_scenes_sdf_rows_dev (they replace a
 * start / goal pair), by edmp_unet_forward_dev (the
 * model's input buffer carries the next segment's input), by a changed edmp_sampler_set_condition and by edmp_sampler_init: a
 * continuing segment after any of them is refused.  A run started with guided = 0 cannot be continued with guided = 1 (the guide
 * never received its pair).  Calls that read neither the guide's start / goal pairs, nor the sampler, nor the model's buffers leave a run
 * as it stands, and the next segment continues as if they had not been made: edmp_scenes_goal_filter_dev, edmp_ik_solve_dev,
 * edmp_self_collision_rows_dev, edmp_sdf_self_rows_dev, edmp_sdf_goal_rows_dev, edmp_sdf_sweep_rows_dev, edmp_scenes_sdf_sweep_rows_dev,
 * edmp_sdf_repair_rows_dev and edmp_scenes_sdf_repair_rows_dev.
 * start / goal are read by the init segment only (uploaded once, kept on the device); a continuing segment IGNORES its start /
 * goal arguments and goes on with the init segment's pair. */
int edmp_denoise_guided_segment_dev(edmp_ctx* ctx, const double* noise_dev, int B, const double* start, const double* goal,
                                    int guided, int t_hi, int t_lo, int init, int zero_row0, double* X_out_dev);

/* Warm start: the init of a segmented run that begins at step t_start <= T from a prior plan instead of at T from pure noise (no
 * reference counterpart; the forward process is Diffusion.q_sample_from_x0's, diffusion.py:79-105).  One kernel builds the run's state
 *   X = sqrt(alpha_bar[t_start - 1]) * x0 + sqrt(1 - alpha_bar[t_start - 1]) * eps      (rounded as edmp_q_sample_dev, cumulative = 1)
 * or X = x0 when eps_dev is NULL (a resume from a saved state), pins X[:, :, 0] / X[:, :, -1] to start / goal - the run's pair, not x0's
 * own end columns - when conditioning is on, and writes the first step's UNet input.  x0 (x0_rows, C, N) f64 on the device: x0_rows = B
 * is one plan per row, x0_rows = 1 one plan for the whole batch; eps (B, C, N) f64 on the device.  1 <= t_start <= T and x0_rows in
 * {1, B}, else EDMP_ERR_ARG.  X_out_dev (B, C, N) f64 or NULL receives the seeded state.
 * The call is an init segment in every other respect: the same checks (model and sampler present, B <= max_batch, a bound single-scene
 * guide with B rows when guided), the same upload of start / goal (to the guide too when guided; that upload is the call's only host
 * synchronisation, X_out_dev or not), and it leaves a run in progress at step t_start.  edmp_denoise_guided_segment_dev continues it with
 * init = 0 and t_hi = t_start (noise_dev[0] = the draw of step t_start); everything said above about what ends or invalidates a run
 * holds unchanged, the guided = 0 rule included.  A refused call launches nothing.  Segments are never replayed from a hipGraph
 * (edmp_sampler_set_graph), so a warm-started run is always enqueued eagerly. */
int edmp_sampler_seed_dev(edmp_ctx* ctx, const double* x0_dev, int x0_rows, const double* eps_dev, int B, const double* start,
                          const double* goal, int guided, int t_start, double* X_out_dev);

/* ---- scene batch: several scenes in one launch chain ------------------------------------------------------ */
/* S scenes of B rows each run as ONE (S*B, C, N) state through the device-resident loop; scene s owns rows [s*B, (s+1)*B).  The
 * reference plans one scene per Diffusion.denoise_guided call (infer_serial.py:108-157); its only coupling between rows is the
 * whole-batch norm of lib/guide.py:629, which a scene batch forms PER SCENE, so every scene's rows equal its own serial run bit for bit.
 *
 * edmp_scene_batch_set replaces S calls of edmp_scene_set (lib/guide.py:13-43, 118-158) with ONE guide object in the current guide
 * slot: n_obstacles (S,) int32 with 1..EDMP_MAX_OBSTACLES each; obstacle_config (sum n_obstacles, 10) f64, scene after scene;
 * n_classes (S,) int32; clearance / expansion (sum n_classes, T) f64, scene after scene.  Classes are numbered across the scenes
 * (scene s's follow scene s-1's) and each keeps its own scene's obstacle count.  link_half_extents, dh, static_frames as
 * edmp_scene_set (one robot).  edmp_rows_set is then called ONCE for all S*B rows with row_class in that numbering; rows / S is the
 * rows per scene (rows that do not split evenly over S are refused).  On a bound scene batch the single-scene loop (guided), the
 * teacher-forced steps, the cost / gradient / best-trajectory / success entry points and edmp_scene_set_shapes are refused
 * (EDMP_ERR_STATE): use one guide per scene for those, or - for the scoring of the finished state - the edmp_scenes_* calls below. */
int edmp_scene_batch_set(edmp_ctx* ctx, int S, const int32_t* n_obstacles, const double* obstacle_config, const int32_t* n_classes,
                         const double* clearance, const double* expansion, int T, const float* link_half_extents, const float* dh,
                         const float* static_frames);
/* replaces S calls of Diffusion.denoise_guided (diffusion.py:300-356), one per scene, with one loop: noise (T+1, S*B, C, N) f64 on the
 * device, noise[k] rows [s*B, (s+1)*B) = scene s's own draw k.  starts / goals (S,7) f64 host (may be NULL only when neither
 * conditioning nor guided).  X_out (S*B, C, N) f64.  zero_row0 applies quirk Q3 to row 0 of EVERY scene.  guided = 0: the unguided
 * loop with per-scene conditioning (no guide needed).  Guided needs a bound scene batch of S scenes and S*B rows.  The device noise
 * mode and the all-reduce hook are refused (the hook sums ONE scalar). */
int edmp_denoise_scenes_dev(edmp_ctx* ctx, const double* noise_dev, int S, int B, const double* starts, const double* goals, int guided,
                            int t_stop, int zero_row0, double* X_out_dev);
/* the same loop in segments, with the t_hi / t_lo / init contract of edmp_denoise_guided_segment_dev (run bookkeeping included:
 * the continuing segment's S, B and t_hi must be the run's; its starts / goals are ignored) */
int edmp_denoise_scenes_segment_dev(edmp_ctx* ctx, const double* noise_dev, int S, int B, const double* starts, const double* goals,
                                    int guided, int t_hi, int t_lo, int init, int zero_row0, double* X_out_dev);

/* edmp_sampler_seed_dev for a scene batch: x0 (x0_rows, C, N) with x0_rows = S*B (one plan per row) or S (scene s's plan for all its B
 * rows), eps (S*B, C, N), starts / goals (S,7) as edmp_denoise_scenes_dev; every row is pinned to its own scene's pair.  Guided needs the
 * bound scene batch of S scenes and S*B rows; on a single-scene guide it is refused with EDMP_ERR_STATE, as edmp_sampler_seed_dev is on a
 * bound scene batch.  edmp_denoise_scenes_segment_dev continues the run with init = 0 and t_hi = t_start. */
int edmp_sampler_seed_scenes_dev(edmp_ctx* ctx, const double* x0_dev, int x0_rows, const double* eps_dev, int S, int B, const double* starts,
                                 const double* goals, int guided, int t_start, double* X_out_dev);

/* ---- scoring a bound scene batch: best row and success per scene ------------------------------------------------ */
/* What the reference does once per scene after its loop - choose_best_trajectory (lib/guide.py:637-653) and the success tally
 * (infer_serial.py:94-99, 165-168 on lib/environment.py:632-680) - for the finished (S*B, 7, N) state of a scene batch, in one launch
 * per step instead of one guide per scene.  Every call needs the bound guide to be a scene batch (edmp_scene_batch_set, a batch of ONE
 * scene included, + edmp_rows_set) and S, B to be that batch's scenes and rows per scene: on a single-scene guide they are refused with
 * EDMP_ERR_STATE, with another S or B with EDMP_ERR_ARG, and nothing is launched.  Scene s's results equal, bit for bit, what the
 * per-scene entry point returns for rows [s*B, (s+1)*B) on scene s's own guide.
 *
 * edmp_scene_batch_set_shapes: edmp_scene_set_shapes (lib/environment.py:249-268) for the batch: kind (n_total,) int32, 0 cuboid / 1
 * cylinder, for all sum n_obstacles obstacles, scene after scene (all cuboids after edmp_scene_batch_set).  n_total must be the batch's
 * total (EDMP_ERR_ARG otherwise); refused on a single-scene guide (EDMP_ERR_STATE), which has edmp_scene_set_shapes. */
int edmp_scene_batch_set_shapes(edmp_ctx* ctx, const int32_t* kind, int n_total);
/* edmp_row_swept_volumes_dev (the volume part of choose_best_trajectory, lib/guide.py:637-653) per scene: X (S*B,7,N) f64 on the device,
 * 3 <= N <= 64; starts / goals (S,7) f64 host (required); volumes (S*B,) f32 on the device (NULL: kept in the guide's scratch): every row's
 * t = 0 swept volume against its OWN scene's obstacles and start / goal pair.  best_index_host (S,) int or NULL: the arg-min of each
 * scene's B volumes as edmp_argmin_dev defines it (first index on ties, the first NaN wins), relative to the scene; synchronises only
 * when given.  Replaces the guide's start / goal pairs, so it ends a segmented run like its single-scene sibling. */
int edmp_scenes_swept_volumes_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const double* starts, const double* goals,
                                  float* volumes_dev, int* best_index_host);
/* edmp_select_row_dev's rule (lib/guide.py:637-653 widened by infer_serial.py:119-129) per scene: volumes (S*B,) f32 and key (S*B,) f64 on
 * the device; minimum, candidates and pick all lie inside the scene's own B rows.  index_host (S,) int, relative to the scene
 * (synchronises).  One launch for the whole batch. */
int edmp_scenes_select_rows_dev(edmp_ctx* ctx, const float* volumes_dev, const double* key_dev, int S, int B, double trust_region,
                                int* index_host);
/* edmp_success_rows_dev (RobotEnvironment.benchmark_trajectory + check_collisions, lib/environment.py:632-680, 591-608; tally of
 * infer_serial.py:94-99, 165-168) per scene: X (S*B,7,N) f64 on the device, N >= 2, 1 <= substeps <= 64; a row is checked against the
 * obstacles and kinds of its own scene only.  ok / first / within (S*B,) int32 on the device, each optional.  counts_host (S,4) int32 or
 * NULL (synchronises when given): per scene [rows ok, rows within limits, rows collision-free, B]. */
int edmp_scenes_success_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int substeps, const double* dh_f64,
                                 int32_t* ok_dev, int32_t* first_dev, int32_t* within_dev, int32_t* counts_host);

/* ---- the sphere signed-distance guide inside a scene batch (csrc/sdf.hip) ------------------------------------------ */
/* edmp_sdf_set for a bound scene batch, after edmp_scene_batch_set and edmp_rows_set: ONE sphere table (a batch has one robot),
 * spheres (n,5) f32 as edmp_sdf_set; sdf_row (S*B,) int32 0/1, margin (S*B,T) f64 and smoothness (S*B,) f64, scene after scene, so the
 * masks, margins and weights may differ from scene to scene.  The value checks are edmp_sdf_set's; a message names the scene and the row
 * inside it.  Needs the bound guide to be a scene batch of exactly S scenes x B rows (a batch of ONE scene included): EDMP_ERR_STATE on a
 * single-scene guide, EDMP_ERR_ARG for another S, B or T.  Bumps the context's epoch and synchronises, as edmp_sdf_set; a later
 * edmp_rows_set drops the table.  In edmp_denoise_scenes_dev, its segments and edmp_sampler_seed_scenes_dev an SDF row of scene s is
 * one workgroup of sdf_guide_kernel that stages the primitives and kinds of scene s only, loops over scene s's own obstacle count and
 * reads scene s's start / goal pair; sum g^2 is formed per scene.  Scene s's rows - the SDF rows, and the grad_norm rows that share
 * their norm - therefore equal, bit for bit, scene s's own serial run on a guide with edmp_sdf_set, whatever its neighbours and its
 * position in the batch.  With no SDF row in the batch nothing else is launched and every result is what it was. */
int edmp_scene_batch_set_sdf(edmp_ctx* ctx, const float* spheres, int n_spheres, const int32_t* sdf_row, const double* margin,
                             const double* smoothness, int S, int B, int T);
/* edmp_sdf_rows_dev per scene: X (S*B,7,N) f64 on the device (not clipped), 3 <= N <= 64, its interior columns 1..N-2 are the waypoints;
 * starts / goals (S,7) f64 host; cost_dev / clearance_dev (S*B,) f64 on the device.  Every row is scored against its OWN scene's
 * primitives, kinds and start / goal pair, with margin[row][t - 1] for t >= 1 (0 at t = 0) and the row's own smoothness weight: scene s's
 * values equal, bit for bit, what edmp_sdf_rows_dev returns for X[s*B .. (s+1)*B)[:, :, 1:-1] on scene s's own guide.  Needs the table of
 * edmp_scene_batch_set_sdf (EDMP_ERR_STATE without it).  Refused on a single-scene guide with EDMP_ERR_STATE, with another S or B, an N
 * outside 3..64 or a t outside 0..T with EDMP_ERR_ARG; a refused call launches nothing.  Replaces the guide's start / goal pairs, so it
 * ends a segmented run like edmp_scenes_swept_volumes_dev.  Does not synchronise. */
int edmp_scenes_sdf_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, int t, const double* starts, const double* goals,
                             double* cost_dev, double* clearance_dev);

/* The reference's IK-goal filter (infer_serial.py:117-129: guide.cost of every candidate at t = 0, summed; everything within
 * volume_trust_region of the minimum; of those the goal nearest to the start) for ALL scenes of a bound scene batch in two launches,
 * where the per-scene route is one guide object, one edmp_guide_cost_dev launch, a reduction and a copy back per scene.
 * goals (sum n_goals, 7) f64 on the device, scene after scene; n_goals (S,) int32 on the host, each >= 1 (scenes bring unequal numbers
 * of candidates); starts (S,7) f64 on the host.
 *   volumes (sum n_goals,) f32: candidate r of scene s against scene s's uninflated (t = 0) obstacles: every (link, obstacle) element
 *     is bit for bit the element edmp_guide_cost_dev(goal.reshape(1,7,1), t = 0) writes on scene s's own guide (the joints are cast to
 *     f32, nothing is clipped); they are added as (float) sum_{l=0..8} ( sum_{ob=0..no-1} (double) v[l][ob] ), both sums sequential in
 *     f64 in index order, rounded to f32 once.  The reference's torch f32 .sum(axis=(1,2)) differs from this by summation rounding only.
 *   key (sum n_goals,) f64: sqrt(sum_j (start_s[j] - goal_r[j])^2), the squares added in joint order without contraction and the root
 *     correctly rounded = np.linalg.norm(start - goals, axis=1) bit for bit (infer_serial.py:129).
 *   index_host (S,) int, inside the scene: edmp_select_row_dev's rule on the scene's own rows - m = the first minimum volume (NaN counts
 *     as smallest and keeps m); the candidates are the rows with (double) v < (double) v_m + trust_region; of those the smallest finite
 *     key; on equal keys the smaller volume, then the lower index (the reference takes the arg-min over the volume-sorted list,
 *     infer_serial.py:121-129); m if no candidate has a finite key.
 * volumes_dev / key_dev may be NULL (kept in the guide object's scratch: pool blocks, grow-only; the context's epoch is bumped when a
 * block moves).  The call synchronises (index_host).  No floating-point atomics: results are bit-identical between runs, and a scene's
 * results depend neither on its neighbours nor on its position in the batch.
 * Needs a bound scene batch of exactly S scenes (a batch of ONE scene included): refused with EDMP_ERR_STATE on a single-scene guide,
 * with EDMP_ERR_ARG for another S, any n_goals[s] < 1, a NULL goals / n_goals / starts / index_host or a negative trust_region; a
 * refused call launches nothing and changes nothing.
 * The call reads the scene tables only: it does not touch the guide's start / goal pairs, the sampler or the model's buffers, so -
 * unlike edmp_scenes_swept_volumes_dev - it does NOT end a segmented run: the next segment continues as if the call had not been made.
 * (The scratch rule above is the one way it can still get in a run's way: a call whose scratch has to grow bumps the epoch, and a run in
 * progress under the old epoch refuses its next segment.  A call of at least that many candidates before the run - the driver's order
 * of events - leaves nothing to grow.) */
int edmp_scenes_goal_filter_dev(edmp_ctx* ctx, const double* goals_dev, int S, const int32_t* n_goals, const double* starts,
                                double trust_region, float* volumes_dev, double* key_dev, int* index_host);

/* ---- IK goal candidates (csrc/ik.hip) ---------------------------------------------------------------------- */
/* Stands for FrankaRobot.ik of the problem's target pose (datasets/load_test_dataset.py:170-187: robofin's ikfast, not part of this
 * package): a batched NUMERICAL inverse kinematics of the 7-DoF arm, damped least squares from many seeds, for all targets of a scene
 * group in ONE launch (one lane per seed, f64 throughout).  The candidates are points of the same solution continuum as the
 * reference's, not its numbers.
 *   targets (T,12) f64 on the host: row-major 3x4 [R | p] of the tool frame in the base frame;  n_seeds (T,) int32 on the host, each >= 1
 *   (ragged);  seeds (sum n_seeds, 7) f64 on the device, target after target;  tool (12,) f64 on the host: the fixed 3x4 frame behind
 *   the joint-7 frame of the modified-DH chain (lib/guide.py:29-35) whose pose is matched.
 * Per seed, `iters` times: FK; e = [p_t - p ; 1/2 sum_k R[:,k] x R_t[:,k]]; the geometric 6x7 Jacobian J; dq = J^T (J J^T + lambda^2 I)^-1 e
 * by a Cholesky factorisation; dq scaled so that max|dq| <= max_step; q clamped to the joint limits (diffusion/diffusion.py:282-296).
 * After the last step, per seed (row r of the flat seed array):
 *   q (sum,7) f64: the final configuration, inside the limits;
 *   residuals (sum,2) f64: |p_t - p| [m] and the rotation angle of R^T R_t [rad], atan2(|vee|, (trace - 1) / 2) - the true angle: a pose
 *     turned by pi has a vanishing cross-product error and must not pass;
 *   valid (sum,) int32: 1 iff q and both residuals are finite, position <= tol_pos and angle <= tol_ang.
 * A seed's outputs depend on (its target, the seed, the parameters) only - not on the other seeds or targets of the call - and are
 * bit-identical between runs.  edmp_amd/ik.py's defaults: iters 64, lambda 0.01, max_step 0.5, tol_pos 1e-6, tol_ang 1e-6.
 * EDMP_ERR_ARG, before anything is launched: a NULL pointer, T < 1, a count < 1, iters < 1, lambda <= 0, max_step <= 0, a negative
 * tolerance, a non-finite parameter, target or tool entry, a target or tool rotation that is not orthonormal to 1e-9 (or a reflection).
 * Context-level: needs no model, scene or rows, reads and replaces nothing of theirs, and does not end a segmented run.  Synchronises
 * (the targets' device copy is a temporary of the call).
 *
 * edmp_ik_compact_dev: the valid rows of q, densely, in seed order, target after target -> goals (n_valid_total, 7) f64 on the device
 * (room for sum n_seeds rows), counts_host (T,) int32 - exactly edmp_scenes_goal_filter_dev's goals_dev + n_goals, whose tie-breaks go
 * by index, so the order is part of the result (stable; no atomics).  A target may come out with count 0; the filter refuses such a
 * scene.  Same binding rules; synchronises (counts_host). */
int edmp_ik_solve_dev(edmp_ctx* ctx, const double* targets, int T, const int32_t* n_seeds, const double* seeds_dev, const double* tool,
                      int iters, double lambda, double max_step, double tol_pos, double tol_ang, double* q_dev, double* residuals_dev,
                      int32_t* valid_dev);
int edmp_ik_compact_dev(edmp_ctx* ctx, const double* q_dev, const int32_t* valid_dev, int T, const int32_t* n_seeds, double* goals_dev,
                        int32_t* counts_host);

/* Device noise source — explicitly NOT the reference's NumPy RandomState stream (that contract is served by
 * edmp_denoise_guided_dev): Philox4x32-10 counter RNG + Box-Muller inside the sampler kernels, no noise tensor, no
 * host draw, no upload.  Same loop otherwise (replaces diffusion.py:300-356 with z ~ N(0, I) drawn on the GPU).
 * edmp_rng_normal_dev materialises the z tensor (B,C,N) f64 the loop uses at step_index (0 = initial X_T,
 * 1 + T - t = reverse step t) so the two entry points can be cross-checked. */
int edmp_denoise_guided_rng_dev(edmp_ctx* ctx, uint64_t seed, int B, const double* start, const double* goal, int guided,
                                int t_stop, int zero_row0, double* X_out_dev);
int edmp_rng_normal_dev(edmp_ctx* ctx, uint64_t seed, int step_index, int B, int C, int N, double* out_dev);

/* The device noise source in the other run forms: segments, scene batches, warm starts.
 *
 * The stream contract.  Philox counter = (element, step, block, 0), key = seed (what edmp_denoise_guided_rng_dev and
 * edmp_rng_normal_dev have always drawn), with
 *   element = the (row, waypoint) index inside the row's OWN scene: (b - s * B) * N + l for row b of scene s = b / B of a scene batch,
 *             b * N + l for a single scene;
 *   key     = the seed of the row's scene: a scene batch takes S seeds on the host, one per scene, any uint64 values, equal ones allowed;
 *   step    = 0 for the X_T draw of a full run - and for the eps draw of a re-noising warm start, which draws no X_T -,
 *             1 + T - t for reverse step t.  The step is absolute, so a segment carries no stream state.
 * Hence, bit for bit: scene s of a scene batch is the single-scene run of that scene under seeds[s], whatever its neighbours, their
 * seeds and its position; every run equals the explicit-noise run fed the streams edmp_rng_normal_dev(seeds[s], step, B, ...)
 * materialises; a segmented run equals the unsegmented one.
 *
 * edmp_denoise_guided_rng_segment_dev / edmp_denoise_scenes_rng_segment_dev are edmp_denoise_guided_segment_dev /
 * edmp_denoise_scenes_segment_dev with the seed(s) in the place of noise_dev; edmp_denoise_scenes_rng_dev is edmp_denoise_scenes_dev
 * likewise.  edmp_sampler_seed_rng_dev / edmp_sampler_seed_scenes_rng_dev are the seed calls with the seed(s) and `renoise` in the place
 * of eps_dev: renoise != 0 forward-noises x0 with eps = the step-0 draw of every row's stream (products and sum rounded separately, as
 * with eps_dev), renoise == 0 draws nothing and takes x0 as the state at t_start.
 *
 * A run records its noise source with the rest of its record: an init (init != 0, a whole run, a seed call) stores the source and,
 * for the device source, the seeds in the context.  A continuing segment (init == 0) of a device-noise run reads the RECORDED seeds -
 * its own seed argument is not read, like its start / goal pair (seeds may be NULL there) - and a continuing segment that brings
 * the other source is refused with EDMP_ERR_STATE, the message naming both; a refused call changes nothing.  Segments are enqueued
 * eagerly; edmp_denoise_scenes_rng_dev replays a hipGraph under edmp_sampler_set_graph like the other whole-run calls, and a replay
 * draws under THIS call's seeds: the kernels read them from the context's seed table, uploaded before the launch.  With an
 * all-reduce hook installed these five calls are refused with EDMP_ERR_ARG (a row shard's element indices are not the logical
 * batch's). */
int edmp_denoise_guided_rng_segment_dev(edmp_ctx* ctx, uint64_t seed, int B, const double* start, const double* goal, int guided,
                                        int t_hi, int t_lo, int init, int zero_row0, double* X_out_dev);
int edmp_denoise_scenes_rng_dev(edmp_ctx* ctx, const uint64_t* seeds, int S, int B, const double* starts, const double* goals, int guided,
                                int t_stop, int zero_row0, double* X_out_dev);
int edmp_denoise_scenes_rng_segment_dev(edmp_ctx* ctx, const uint64_t* seeds, int S, int B, const double* starts, const double* goals, int guided,
                                        int t_hi, int t_lo, int init, int zero_row0, double* X_out_dev);
int edmp_sampler_seed_rng_dev(edmp_ctx* ctx, const double* x0_dev, int x0_rows, uint64_t seed, int renoise, int B, const double* start,
                              const double* goal, int guided, int t_start, double* X_out_dev);
int edmp_sampler_seed_scenes_rng_dev(edmp_ctx* ctx, const double* x0_dev, int x0_rows, const uint64_t* seeds, int renoise, int S, int B,
                                     const double* starts, const double* goals, int guided, int t_start, double* X_out_dev);

/* Replay mode of the device-resident loop: on = 1 captures the stream work of one edmp_denoise_guided*_dev call
 * (255 reverse steps, ~16k kernel nodes) into a hipGraph the first time and replays it while the call's arguments,
 * scene, rows and weights stay the same (start/goal are read from a device buffer and may change freely).  Results are
 * bit-identical to the eager enqueue.  Off by default:
 * measured neutral on MI355X at B = 4..1024 - the loop is bound by kernel execution, not by launch. */
int edmp_sampler_set_graph(edmp_ctx* ctx, int on);

/* ---- training-side forward process --------------------------------------------------------- */
/* replaces the arithmetic of Diffusion.q_sample (diffusion/diffusion.py:52-77, cumulative = 0: a = alpha),
 * Diffusion.q_sample_from_x0 (:79-105, cumulative = 1: a = alpha_bar) and the conditioning of generate_q_sample
 * (:239-242):   xt = sqrt(a[t_b - 1]) * x + sqrt(1 - a[t_b - 1]) * eps,   mean = sqrt(a[t_b - 1]) * x
 * with one timestep per row (t_host: B int32 on the HOST, each in 1..T); condition != 0 then pins xt[:, :, 0] and
 * xt[:, :, -1] to x.  x, eps, xt, mean: (B,C,N) f64 on the device; mean_dev may be NULL.  Rounded like NumPy's f64
 * expression (two products, one sum, no FMA contraction), so results are bit-identical to the reference's. */
int edmp_q_sample_dev(edmp_ctx* ctx, const double* x_dev, const double* eps_dev, const int32_t* t_host, int B, int C, int N,
                      int cumulative, int condition, double* xt_dev, double* mean_dev);

/* ---- resident objects ----------------------------------------------------------------------------------- */
/* The reference keeps Python objects alive side by side: one TemporalUNet per process, one IntersectionVolumeGuide per
 * scene (infer_serial.py:50, 112).  A context holds up to 3 models and 8 guides (scene tables + row arrays) resident
 * in HBM, addressed by a caller-chosen non-zero key; edmp_unet_load / edmp_scene_set / edmp_rows_set always act on the
 * CURRENT slot.  edmp_*_slot(key) makes `key` current (parking the previous one, evicting the least recently used
 * beyond the capacity) and returns 1 if the slot already holds a loaded object - nothing to upload -, 0 if it is
 * empty (load into it next), < 0 on error.  Key 0 is the default slot of callers that never use slots. */
int edmp_unet_slot(edmp_ctx* ctx, uint64_t key);
int edmp_guide_slot(edmp_ctx* ctx, uint64_t key);

/* ---- one logical batch over several GPUs ------------------------------------------------------------------ */
/* The reference has no distributed code; its only coupling between batch rows is the whole-batch gradient norm
 * gradient1 / np.linalg.norm(gradient1) (lib/guide.py:629).  When one reference batch is row-sharded over ranks, the
 * device-resident loop calls `fn(user, hip_stream, sumsq_dev)` once per guided step, between the gradient kernels
 * and the state update: the callee must enqueue, ON THAT STREAM, an in-place sum over ranks of the f64 device scalar
 * (e.g. ncclAllReduce / torch.distributed.all_reduce with that stream current) and return 0.  fn = NULL (default)
 * restores the single-GPU behaviour.  hipGraph replay is disabled while a caller hook is installed (an arbitrary callee is not
 * capturable; the native RCCL hook below is). */
typedef int (*edmp_allreduce_fn)(void* user, void* hip_stream, double* sumsq_dev);
int edmp_sampler_set_allreduce(edmp_ctx* ctx, edmp_allreduce_fn fn, void* user);

/* The hook as native code (csrc/rccl_hook.hip): one ncclAllReduce of the f64 scalar on the context's stream per guided step - no
 * Python / GIL inside the device-resident loop (the round-5 hook was a ctypes callback into torch.distributed.all_reduce:
 * edmp_amd/diffusion.py; it stays available through edmp_sampler_set_allreduce).  RCCL is resolved at run time, never linked:
 *   edmp_rccl_load(path)       path = NULL: the RCCL already in the process (the one torch brought), else librccl.so.1; or a path
 *   edmp_rccl_unique_id(id)    ncclGetUniqueId into 128 caller bytes: one rank calls it and hands the bytes to the others by any
 *                              means (torch.distributed.broadcast_object_list over gloo or nccl, MPI, a file)
 *   edmp_rccl_attach(ctx, id, nranks, rank)   ncclCommInitRank on the context's device (collective over the ranks), installs the hook
 *   edmp_rccl_attach_comm(ctx, comm)          borrow a communicator the host already has (torch: ProcessGroupNCCL._comm_ptr())
 *   edmp_rccl_enable(ctx, on)  attach leaves the hook ON; 0 switches the collective off and keeps the communicator (runs of this
 *                              context that are NOT shards of one logical batch), 1 switches it on again
 *   edmp_rccl_detach(ctx)      remove the hook, destroy an owned communicator (also done by edmp_ctx_destroy).  edmp_sampler_set_allreduce
 *                              replaces the ACTIVE hook only; an attached communicator stays and edmp_rccl_enable brings it back
 *   edmp_rccl_info(ctx, out)   out = {nranks, rank, 0 none | 1 own communicator | 2 borrowed}
 * ncclAllReduce is stream-capturable: whole-run hipGraph replay (edmp_sampler_set_graph) stays legal with THIS hook installed.
 * edmp_sampler_allreduce_stats: host time spent inside the hook (any hook) since the last reset: {calls, total ns, max ns}. */
int edmp_rccl_load(const char* path);
int edmp_rccl_unique_id(void* id128);
int edmp_rccl_attach(edmp_ctx* ctx, const void* id128, int nranks, int rank);
int edmp_rccl_attach_comm(edmp_ctx* ctx, void* nccl_comm);
int edmp_rccl_enable(edmp_ctx* ctx, int on);
int edmp_rccl_detach(edmp_ctx* ctx);
int edmp_rccl_info(edmp_ctx* ctx, int32_t out[3]);
int edmp_sampler_allreduce_stats(edmp_ctx* ctx, uint64_t out[3], int reset);

/* ---- instrumentation ----------------------------------------------------------------------------------- */
/* accumulate HIP-event time of the dominant kernel family (the MFMA conv kernels of the UNet layer program) while enabled:
 * on = 1: one event pair around every conv launch (per-op table, edmp_prof_ops; ~2 events of overhead per launch);
 * on = 2: one event pair around the whole layer program of each reverse step (the family's total, negligible overhead);
 * on = 0: off.  Events are recorded on the context's stream. */
int edmp_prof_enable(edmp_ctx* ctx, int on);
/* total ms and launch count of the MFMA conv kernels since the last reset (synchronises) */
int edmp_prof_read(edmp_ctx* ctx, double* conv_ms, int64_t* conv_launches, int reset);
/* Per-op view of the same instrumentation (bench.py's per-kernel roofline table; no reference counterpart): for every
 * op i < min(*n_ops, cap) of the loaded UNet's layer program: summed event time [ms], launches, executed FLOPs per
 * trajectory per launch, and the kernel instance name (64 bytes each, as rocprofv3 prints it without "edmp::"). */
int edmp_prof_ops(edmp_ctx* ctx, int cap, int* n_ops, double* ms, int64_t* calls, double* flops_exec, char* names);
/* per op of the same program: FLOPs per trajectory per launch issued on the bf16 matrix pipe (0 for an fp32-MFMA op) */
int edmp_prof_ops_bf16(edmp_ctx* ctx, int cap, int* n_ops, double* flops_bf16);
/* per op of the same program, as the HIP runtime reports them when the model is built (no reference counterpart): kernel instance
 * name (64 bytes each), VGPRs per lane (arch + acc), threads per workgroup, dynamic LDS bytes and workgroups per CU at that size.
 * Filled for the bf16x3 ops, whose CU claim the build checks (profiles/r06_coresidency_fault.md); 0 for every other op. */
int edmp_unet_op_attrs(edmp_ctx* ctx, int cap, int* n_ops, char* names, int* regs, int* block, int* lds_bytes, int* wg_per_cu);
/* host-only: 1 if a workgroup with these runtime attributes owns its CU (one workgroup per CU, and its waves' VGPRs, allocated in
 * granules of 8, fill the 512-entry file of every SIMD it runs on, so that no wave of another kernel fits beside it); else 0.
 * The decision edmp_unet_load applies to every bf16x3 op, refusing the model (EDMP_BF16X3=0 builds it without them). */
int edmp_cu_claim(int regs, int block, int lds_bytes, int wg_per_cu);

#ifdef __cplusplus
}
#endif
#endif /* EDMP_HIP_H */
