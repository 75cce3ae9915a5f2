// certify.hip — a CONTINUOUS collision certificate for finished rows: an answer that holds for every configuration of the joint-space
// polyline, not for a list of them.  success.hip, shortcut.hip and blend.hip test the exact f64 link-box check at the waypoints and at
// `substeps` - 1 interpolants per segment; an obstacle thinner than the spacing of those configurations can be passed through unseen.
// This stage closes that gap by conservative advancement: clearance.h gives a lower bound g on the distance between a link box and the
// obstacles at one configuration, and motion radii rho[l][j] that bound how far any point of link box l moves when joint j turns; at
// the centre of an interval of a segment a -> b the box stays inside its pose grown by reach = (half the interval) x sum_j |b_j - a_j|
// rho[l][j], so g - reach > margin certifies the whole interval.  Where it does not, the exact test decides whether the centre is a hit;
// otherwise the interval is halved, down to depth D.  Per row the verdict is free (a proof), hit (an exact collision at a stated
// configuration) or undecided (at the depth limit).  The rule, interval by interval, is stated in include/edmp_hip.h and as plain Python
// in tests/certify_inputs.py.
//
// Design: one 256-thread workgroup per listed row; the row's scene's obstacles and kinds staged in LDS as success_rows_kernel stages
// them.  The (N - 1) x 9 items (segment w, link l) are dealt link-major (item = l (N - 1) + w): the lanes of a wave walk the same chain
// prefix and meet similar depths.  An item re-walks the chain to its link's frame per evaluation (configuration_self_hit's rule: no
// per-thread array indexed by the joint number, the joint loop is not unrolled), so nothing goes to scratch.  Items combine through LDS
// by integer minimum / sum, and the bound by an f64 minimum through a tree reduction: no float atomics, nothing across workgroups, and
// no output depends on the order in which lanes finish.  All f64.
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "linkbox.h"    // Robot64, robot64_of, SceneSlices, obb_overlap, obb_cylinder_overlap_body, interp_joint
#include "clearance.h"  // box_box_gap, box_cylinder_gap, motion_radii
#include "rowlist.h"    // check_rows, rows_upload, rows_call_end: shared with shortcut.hip, timing.hip and blend.hip

namespace edmp {

static_assert(kGapSatEps == kSatEps, "the gap's projection radii are the exact test's");

constexpr int kCertifyN = 64;           // waypoints per row at most
constexpr int kCertifyMaxDepth = 10;    // 2^10 leaves per segment; the hit / undecided key holds 2^(D + 1) positions in 11 bits
constexpr double kCertifySlack = 1e-9;  // an interval is accepted if g - reach > margin + this
constexpr int kNoKey = 0x7fffffff;

struct CertifyArgs {
    const double* X;      // (n, 7, N)
    const int32_t* rows;  // the listed rows, or nullptr = row blockIdx.x
    int N, depth;
    double margin;
    const double* obb;
    const int32_t* kind;
    int32_t *verdict, *segment, *link, *evaluations, *undecided;
    double *fraction, *bound;
};

struct MotionRadii {
    double rho[EDMP_N_LINKS * 7];
};

// the exact test of ONE link box against the scene's obstacles, as configuration_hits makes it (touching counts); the cylinder test in
// its register form: no frame of its own
__device__ __forceinline__ bool link_box_hits(const double LR[3][3], const double Lc[3], const double he[3], const double* ob_all, const int* kind, int no) {
    bool hit = false;
#pragma unroll 1
    for (int ob = 0; ob < no && !hit; ++ob) {
        const double* od = ob_all + ob * 16;
        hit = kind[ob] == 1 ? obb_cylinder_overlap_body<false>(LR, Lc, he, od) : obb_overlap(LR, Lc, he, od);
    }
    return hit;
}

__global__ __launch_bounds__(256) void certify_rows_kernel(CertifyArgs a, SceneSlices sl, Robot64 rc, MotionRadii mr) {
    __shared__ double s_ob[EDMP_MAX_OBSTACLES * 16];
    __shared__ int s_kind[EDMP_MAX_OBSTACLES];
    __shared__ double s_min[256];
    __shared__ int s_bad, s_hit, s_und, s_evals, s_nund;
    const int r = a.rows ? a.rows[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int N = a.N, D = a.depth;
    const int scene = r / sl.rps;
    const int no = min(sl.cnt[scene], EDMP_MAX_OBSTACLES);
    const double* obb = a.obb + (size_t)sl.off[scene] * 16;
    const int32_t* kind = a.kind + sl.off[scene];
    for (int i = tid; i < no * 16; i += 256) s_ob[i] = obb[i];
    for (int i = tid; i < no; i += 256) s_kind[i] = kind[i];
    if (tid == 0) {
        s_bad = 0;
        s_hit = kNoKey;
        s_und = kNoKey;
        s_evals = 0;
        s_nund = 0;
    }
    __syncthreads();
    const double* xr = a.X + (size_t)r * 7 * N;
    {  // a non-finite element anywhere: the row is invalid, nothing is evaluated
        int bad = 0;
        for (int e = tid; e < 7 * N; e += 256) bad |= !isfinite(xr[e]);
        if (bad) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    const bool invalid = s_bad != 0;  // (uniform over the workgroup)
    double minb = INFINITY;
    if (!invalid) {
        const double inv = 1.0 / (double)(2 << D);  // 2^-(D + 1)
        const int full = 1 << D;
        const int trips = (2 << D) - 1;  // the nodes of the whole tree: no input makes the walk run on
#pragma unroll 1
        for (int item = tid; item < EDMP_N_LINKS * (N - 1); item += 256) {
            const int l = item / (N - 1), w = item - l * (N - 1);
            const int k = link_frame(l);
            double L = 0.0;
#pragma unroll 1
            for (int j = 0; j <= k; ++j) L = L + fabs(xr[j * N + w + 1] - xr[j * N + w]) * mr.rho[l * 7 + j];  // (rho = 0 beyond k: the full sum's bits)
            int pos = 0, level = 0, evals = 0, nund = 0, hit_key = kNoKey, und_key = kNoKey;
#pragma unroll 1
            for (int trip = 0; trip < trips && pos < full; ++trip) {
                const int size = 1 << (D - level);
                const int un = 2 * pos + size;  // the centre on the 2^(D + 1) grid
                const double u = (double)un * inv;
                double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
                double o[3] = {0, 0, 0};
#pragma unroll 1
                for (int j = 0; j <= k; ++j) {
                    double sq, cq;
                    sincos(interp_joint(xr[j * N + w], xr[j * N + w + 1], u), &sq, &cq);
                    dh_step(R, o, sq, cq, rc.dh[j]);
                }
                double LR[3][3], Lc[3], he[3];
                frame_apply(R, o, rc.sf[l], LR, Lc);
#pragma unroll
                for (int m = 0; m < 3; ++m) he[m] = rc.he[l][m];
                double g = INFINITY;
#pragma unroll 1
                for (int ob = 0; ob < no; ++ob) {
                    const double* od = s_ob + ob * 16;
                    g = fmin(g, s_kind[ob] == 1 ? box_cylinder_gap(LR, Lc, he, od) : box_box_gap(LR, Lc, he, od));
                }
                ++evals;
                const double reach = L * ((double)size * inv);
                const double slack = g - reach;
                bool advance = false;
                if (slack > a.margin + kCertifySlack) {
                    minb = fmin(minb, slack);
                    advance = true;
                } else if (!(g > 0.0) && link_box_hits(LR, Lc, he, s_ob, s_kind, no)) {  // (g > 0: the shapes are disjoint, the exact test has nothing to say)
                    hit_key = (w << 15) | (un << 4) | l;
                    break;
                } else if (level == D || reach == 0.0) {
                    if (nund == 0) und_key = (w << 15) | (un << 4) | l;
                    ++nund;
                    advance = true;
                } else {
                    ++level;
                }
                if (advance) {
                    pos += size;
                    level = D - (__ffs(pos) - 1);
                }
            }
            atomicAdd(&s_evals, evals);
            if (nund) atomicAdd(&s_nund, nund);
            if (hit_key != kNoKey) atomicMin(&s_hit, hit_key);
            if (und_key != kNoKey) atomicMin(&s_und, und_key);
        }
    }
    s_min[tid] = minb;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s_min[tid] = fmin(s_min[tid], s_min[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        const int v = invalid ? 3 : s_hit != kNoKey ? 1 : s_nund > 0 ? 2 : 0;
        const int key = v == 1 ? s_hit : v == 2 ? s_und : kNoKey;
        a.verdict[r] = v;
        a.segment[r] = key == kNoKey ? -1 : key >> 15;
        a.fraction[r] = key == kNoKey ? -1.0 : (double)((key >> 4) & 0x7ff) / (double)(2 << D);
        a.link[r] = key == kNoKey ? -1 : key & 15;
        a.evaluations[r] = s_evals;
        a.undecided[r] = s_nund;
        a.bound[r] = s_min[0];
    }
}

}  // namespace edmp

using namespace edmp;

// edmp_certify_rows_dev and edmp_scenes_certify_rows_dev behind their own state checks: n = S x rps rows of the state X (n, 7, N).  Every
// refusal comes before any device call.  The row list goes into a block of the call's own (rowlist.h); nothing of the guide is replaced,
// so a segmented run goes on.
static int certify_rows(edmp_ctx* ctx, const char* what, bool batch, const double* X_dev, int S, int rps, int N, const int32_t* rows_host, int n_rows,
                        int depth, double margin, const double* dh_f64, int32_t* verdict_dev, int32_t* segment_dev, double* fraction_dev,
                        int32_t* link_dev, int32_t* evaluations_dev, int32_t* undecided_dev, double* bound_dev, double* radii_out) {
    Guide* g = ctx->guide;
    const int n = S * rps;
    EDMP_REQUIRE(X_dev && verdict_dev && segment_dev && fraction_dev && link_dev && evaluations_dev && undecided_dev && bound_dev, "%s: null pointer", what);
    EDMP_REQUIRE(N >= 2 && N <= kCertifyN, "%s: need 2 <= N <= %d waypoints per row (got %d)", what, kCertifyN, N);
    EDMP_REQUIRE(depth >= 0 && depth <= kCertifyMaxDepth, "%s: depth %d outside 0..%d", what, depth, kCertifyMaxDepth);
    EDMP_REQUIRE(std::isfinite(margin) && margin >= 0.0, "%s: margin %g must be finite and >= 0", what, margin);
    if (int rc = check_rows(what, rows_host, n_rows, n)) return rc;
    const Robot64 rc = robot64_of(g, dh_f64);
    MotionRadii mr;
    motion_radii(rc.dh, rc.sf, rc.he, mr.rho);
    if (radii_out) memcpy(radii_out, mr.rho, sizeof(mr.rho));
    const int launch = rows_host ? n_rows : n;
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    int32_t* rows_dev = nullptr;
    if (int e = rows_upload(ctx, rows_host, n_rows, &rows_dev)) return e;
    CertifyArgs a;
    a.X = X_dev;
    a.rows = rows_dev;
    a.N = N;
    a.depth = depth;
    a.margin = margin;
    a.obb = g->obb;
    a.kind = g->kind;
    a.verdict = verdict_dev;
    a.segment = segment_dev;
    a.link = link_dev;
    a.evaluations = evaluations_dev;
    a.undecided = undecided_dev;
    a.fraction = fraction_dev;
    a.bound = bound_dev;
    hipLaunchKernelGGL(certify_rows_kernel, dim3(launch), dim3(256), 0, ctx->stream, a, scene_slices_of(g, batch, S, rps), rc, mr);
    return rows_call_end(ctx, rows_dev);
}

extern "C" int edmp_certify_rows_dev(edmp_ctx* ctx, const double* X_dev, int n, int N, const int32_t* rows_host, int n_rows, int depth, double margin,
                                     const double* dh_f64, int32_t* verdict_dev, int32_t* segment_dev, double* fraction_dev, int32_t* link_dev,
                                     int32_t* evaluations_dev, int32_t* undecided_dev, double* bound_dev, double* radii_out) {
    EDMP_REQUIRE(ctx && ctx->guide && ctx->guide->obb && ctx->guide->kind, "edmp_certify_rows_dev: scene not set");
    EDMP_REFUSE_SCENE_BATCH(ctx->guide, "edmp_certify_rows_dev");
    EDMP_REQUIRE(n >= 1, "edmp_certify_rows_dev: need n >= 1 rows (got %d)", n);
    return certify_rows(ctx, "edmp_certify_rows_dev", false, X_dev, 1, n, N, rows_host, n_rows, depth, margin, dh_f64, verdict_dev, segment_dev, fraction_dev,
                        link_dev, evaluations_dev, undecided_dev, bound_dev, radii_out);
}

// edmp_certify_rows_dev for a bound scene batch: every row against its own scene's obstacles and kinds
extern "C" int edmp_scenes_certify_rows_dev(edmp_ctx* ctx, const double* X_dev, int S, int B, int N, const int32_t* rows_host, int n_rows, int depth,
                                            double margin, const double* dh_f64, int32_t* verdict_dev, int32_t* segment_dev, double* fraction_dev,
                                            int32_t* link_dev, int32_t* evaluations_dev, int32_t* undecided_dev, double* bound_dev, double* radii_out) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_certify_rows_dev");
    return certify_rows(ctx, "edmp_scenes_certify_rows_dev", true, X_dev, S, B, N, rows_host, n_rows, depth, margin, dh_f64, verdict_dev, segment_dev,
                        fraction_dev, link_dev, evaluations_dev, undecided_dev, bound_dev, radii_out);
}
