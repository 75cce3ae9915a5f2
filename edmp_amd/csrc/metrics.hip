// metrics.hip — the reference's result metrics for every row of the finished batch, on the GPU, and the
// trust-region pick of the plan that those metrics make possible.
//
// Stands for (reference): MetricsCalculator (lib/metrics.py:11-125) — path_length_metric (:32-45: joint-space and end-effector path
// length), smoothness_metric (:11-30: SPARC of the two speed profiles ||diff / dt||) and sparc (:47-125, a restatement of
// mpinets/third_party/sparc.py, defaults padlevel 4, fc 10, amp_th 0.05) — with the end effector of
// IntersectionVolumeGuide.get_end_effector_transform (lib/guide.py:100-116: the seven joint rows of the modified-DH table followed by
// the three fixed rows d = 0.107, theta = -pi/4, d = 0.1034).  The reference evaluates ONE trajectory on the host; so does
// edmp_amd/evaluation.py (path_lengths, smoothness_metric), which is the checker of this kernel (pinned to the reference by
// tests/golden/g13_metrics.npz).  select_row_kernel applies the rule of the reference's IK-goal filter (infer_serial.py:119-129:
// everything within volume_trust_region of the minimum, then the nearest) to choose_best_trajectory's volumes (lib/guide.py:637-653).
//
// Design: one workgroup per trajectory row (the shape of success_rows_kernel), all arithmetic f64.
//   1. thread = waypoint: the DH chain -> end-effector position p_i (LDS)
//   2. thread = segment: ||q_i+1 - q_i||, ||p_i+1 - p_i|| and the two speed samples (LDS); the path lengths are sums in index order
//   3. per profile: the zero-padded DFT as a direct sum (M = N - 1 <= 128 terms per bin, k n mod nfft reduced in integers, twiddles
//      from a per-block LDS table built once with sincospi), |.|, the maximum (order-free), first / last bin over the amplitude
//      threshold among the bins with f <= fc (integer min / max), and the arc length as per-thread partial sums in bin order, a
//      wave butterfly and four wave partials added in wave order.
// Every sum runs in one fixed order that depends on the row's own data only: results are bit-identical between runs, for any B and
// any position of the row in the batch.  No floating-point atomics.
#include "common.h"
#include "chain.h"
#include "guide.h"
#include "pick.h"

#include <cmath>

namespace edmp {

constexpr int kSparcPadLevel = 4;       // lib/metrics.py:47 padlevel
constexpr double kSparcFc = 10.0;       // fc: bins with f <= fc are kept
constexpr double kSparcAmpTh = 0.05;    // amp_th on the spectrum normalised by its maximum
constexpr double kSparcZeroTol = 1e-8;  // np.allclose(profile, 0): every |v_i| <= atol
constexpr int kMetricsMinN = 3, kMetricsMaxN = 129;
constexpr int kMetricsMaxM = kMetricsMaxN - 1;  // samples of a speed profile
constexpr int kMetricsMaxNfft = 2048;           // 2^(ceil(log2 128) + 4)
constexpr int kMetricsThreads = kPickThreads;  // (block_pick reduces over a workgroup of this size)
constexpr int kDftBins = 4;  // bins a thread accumulates side by side (1024 bins at N = 50: one pass)

struct Chain64 {
    double dh[7][4];  // a, d, cos(alpha), sin(alpha)
    double ee[3][6];  // a, d, cos(alpha), sin(alpha), cos(theta), sin(theta): rows 8-10 of the table (chain.h: kEeStaticDh)
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// X (B, 7, N) f64 -> out (4, B) f64: joint path length, end-effector path length, joint SPARC, end-effector SPARC.
// Dynamic LDS: 3 * nfft doubles = twiddles (cos, sin) [nfft] + spectrum [nfft].  step = (1 / dt) / nfft = the bin spacing.
__global__ __launch_bounds__(kMetricsThreads) void metrics_rows_kernel(const double* __restrict__ X, int B, int N, double dt, int nfft, double step,
                                                                       Chain64 ch, double* __restrict__ out) {
    extern __shared__ __align__(16) double s_dyn[];
    __shared__ double s_p[kMetricsMaxN][3];
    __shared__ double s_len[2][kMetricsMaxM];  // segment lengths: joint, end effector
    __shared__ double s_v[2][kMetricsMaxM];    // speed profiles
    __shared__ double s_wave[kMetricsThreads / kWave];
    __shared__ int s_flag[2][2];  // per profile: holds a non-finite sample, holds a sample beyond the zero tolerance
    __shared__ int s_k0, s_k1;
    const int r = blockIdx.x;
    if (r >= B) return;
    const int tid = threadIdx.x;
    const int M = N - 1;
    double* tw = s_dyn;             // [nfft][2]
    double* A = s_dyn + 2 * nfft;   // [nfft]
    const double* xr = X + (size_t)r * 7 * N;
    for (int m = tid; m < nfft; m += kMetricsThreads) {
        double s, c;
        sincospi(2.0 * (double)m / (double)nfft, &s, &c);  // the argument is exact: nfft is a power of two
        tw[2 * m] = c;
        tw[2 * m + 1] = s;
    }
    if (tid < 4) s_flag[tid >> 1][tid & 1] = 0;
    // 1. end-effector positions                                                                      lib/guide.py:100-116
    for (int i = tid; i < N; i += kMetricsThreads) {
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        double o[3] = {0, 0, 0};
#pragma unroll 1
        for (int j = 0; j < 7; ++j) {
            double sq, cq;
            sincos(xr[j * N + i], &sq, &cq);
            dh_step(R, o, sq, cq, ch.dh[j]);  // (chain.h)
        }
#pragma unroll 1
        for (int j = 0; j < 3; ++j) dh_step(R, o, ch.ee[j][5], ch.ee[j][4], ch.ee[j]);
        s_p[i][0] = o[0];
        s_p[i][1] = o[1];
        s_p[i][2] = o[2];
    }
    __syncthreads();
    // 2. segments: lengths and speed samples                                                        lib/metrics.py:11-45
    for (int i = tid; i < M; i += kMetricsThreads) {
        double lj = 0.0, vj = 0.0, le = 0.0, ve = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double d = xr[j * N + i + 1] - xr[j * N + i];
            const double e = d / dt;
            lj += d * d;
            vj += e * e;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double d = s_p[i + 1][a] - s_p[i][a];
            const double e = d / dt;
            le += d * d;
            ve += e * e;
        }
        s_len[0][i] = sqrt(lj);
        s_len[1][i] = sqrt(le);
        const double v[2] = {sqrt(vj), sqrt(ve)};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            s_v[p][i] = v[p];
            if (!isfinite(v[p])) atomicOr(&s_flag[p][0], 1);
            if (fabs(v[p]) > kSparcZeroTol) atomicOr(&s_flag[p][1], 1);
        }
    }
    __syncthreads();
    if (tid == 0 || tid == kWave) {  // two waves, one sum each, in index order
        const int p = tid ? 1 : 0;
        double s = 0.0;
        for (int i = 0; i < M; ++i) s += s_len[p][i];
        out[(size_t)p * B + r] = s;
    }
    // 3. SPARC of the two profiles                                                                  lib/metrics.py:47-125
    const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
        double* res = out + (size_t)(2 + p) * B + r;
        if (s_flag[p][0] || !s_flag[p][1]) {  // block-uniform
            if (tid == 0) *res = s_flag[p][0] ? (double)NAN : 0.0;
            continue;
        }
        const double* v = s_v[p];
        double lmax = 0.0;
        // kDftBins bins per thread at once: one read of v_n feeds that many independent twiddle reads and accumulator pairs, so the
        // LDS latency of one bin hides behind the others'.  Each bin's own sum still runs over n = 0..M-1 in order.
        for (int kb = tid; kb < nfft; kb += kDftBins * kMetricsThreads) {
            double re[kDftBins], im[kDftBins];
            int idx[kDftBins], inc[kDftBins];
#pragma unroll
            for (int j = 0; j < kDftBins; ++j) {
                re[j] = im[j] = 0.0;
                idx[j] = 0;
                inc[j] = (kb + j * kMetricsThreads) & (nfft - 1);  // a bin beyond nfft wraps onto a valid one and is not stored
            }
            for (int n = 0; n < M; ++n) {
                const double vn = v[n];
#pragma unroll
                for (int j = 0; j < kDftBins; ++j) {
                    const double2 cs = reinterpret_cast<const double2*>(tw)[idx[j]];  // (cos, sin): one 16-byte LDS read
                    re[j] += vn * cs.x;
                    im[j] -= vn * cs.y;
                    idx[j] = (idx[j] + inc[j]) & (nfft - 1);  // k n mod nfft
                }
            }
#pragma unroll
            for (int j = 0; j < kDftBins; ++j) {
                const int k = kb + j * kMetricsThreads;
                if (k < nfft) {
                    const double a = hypot(re[j], im[j]);
                    A[k] = a;
                    lmax = fmax(lmax, a);
                }
            }
        }
        lmax = wave_max(lmax);
        if (lane == 0) s_wave[wave] = lmax;
        if (tid == 0) {
            s_k0 = 0x7fffffff;
            s_k1 = -1;
        }
        __syncthreads();
        const double mx = fmax(fmax(s_wave[0], s_wave[1]), fmax(s_wave[2], s_wave[3]));
        int lk0 = 0x7fffffff, lk1 = -1;
        for (int k = tid; k < nfft; k += kMetricsThreads) {
            const double an = A[k] / mx;
            A[k] = an;
            if ((double)k * step <= kSparcFc && an >= kSparcAmpTh) {
                lk0 = min(lk0, k);
                lk1 = max(lk1, k);
            }
        }
        if (lk1 >= 0) {
            atomicMin(&s_k0, lk0);
            atomicMax(&s_k1, lk1);
        }
        __syncthreads();  // also: every thread has read s_wave
        const int k0 = s_k0, k1 = s_k1;
        double acc = 0.0;
        if (k1 > k0) {
            const double span = (double)k1 * step - (double)k0 * step;
            for (int k = k0 + tid; k < k1; k += kMetricsThreads) {
                const double df = ((double)(k + 1) * step - (double)k * step) / span;
                const double da = A[k + 1] - A[k];
                acc += sqrt(df * df + da * da);
            }
        }
        acc = wave_sum(acc);
        __syncthreads();  // s_k0 / s_k1 read by everyone before the next profile resets them
        if (lane == 0) s_wave[wave] = acc;
        __syncthreads();
        if (tid == 0) *res = (k1 < 0) ? (double)NAN : (k1 == k0 ? 0.0 : -(((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3]));
        __syncthreads();  // A and s_wave are reused by the next profile
    }
}

// volumes (B,) f32, key (B,) f64 -> out[0]: m = first minimum of the volumes with NaN as the smallest value (argmin_kernel's rule,
// lib/guide.py:650); a NaN minimum keeps m; else among the rows with (double)v_b < (double)v_m + trust the one with the smallest
// finite key, first index on ties (infer_serial.py:119-129); m when no such row has a finite key.
// Block s applies the rule to the rows [s*B, (s+1)*B) - candidates, minimum and pick all inside them - and writes the index inside that
// segment to out[s]: grid 1 is one batch, grid S a scene batch with B rows per scene.
__global__ __launch_bounds__(kMetricsThreads) void select_row_kernel(const float* __restrict__ vol, const double* __restrict__ key, int B, double trust,
                                                                     int* __restrict__ out) {
    __shared__ Pick s_pick[kMetricsThreads / kWave];
    const int idx = segment_select<false>(vol + (size_t)blockIdx.x * B, key + (size_t)blockIdx.x * B, B, trust, s_pick);
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

}  // namespace edmp

using namespace edmp;

extern "C" int edmp_metrics_rows_dev(edmp_ctx* ctx, const double* X_dev, int B, int N, double dt, const double* dh_f64, double* out_dev) {
    EDMP_REQUIRE(ctx && X_dev && out_dev && B >= 1, "edmp_metrics_rows_dev: need a context, X, out and B >= 1");
    EDMP_REQUIRE(N >= kMetricsMinN && N <= kMetricsMaxN, "edmp_metrics_rows_dev: N = %d outside %d..%d waypoints (padded spectrum of at most %d bins)", N,
                 kMetricsMinN, kMetricsMaxN, kMetricsMaxNfft);
    EDMP_REQUIRE(std::isfinite(dt) && dt > 0.0, "edmp_metrics_rows_dev: dt must be finite and > 0 (got %g)", dt);
    const int M = N - 1;
    int e = 0;
    while ((1 << e) < M) ++e;  // ceil(log2 M)
    const int nfft = 1 << (e + kSparcPadLevel);
    const double fs = 1.0 / dt, step = fs / (double)nfft;
    EDMP_REQUIRE(nfft <= kMetricsMaxNfft && std::isfinite(fs) && step > 0.0, "edmp_metrics_rows_dev: dt = %g gives no usable frequency axis", dt);
    Chain64 ch;
    joint_dh64(dh_f64, ch.dh);
    for (int j = 0; j < 3; ++j) {
        ch.ee[j][0] = kEeStaticDh[j][0];
        ch.ee[j][1] = kEeStaticDh[j][1];
        ch.ee[j][2] = std::cos(kEeStaticDh[j][2]);
        ch.ee[j][3] = std::sin(kEeStaticDh[j][2]);
        ch.ee[j][4] = std::cos(kEeStaticDh[j][3]);
        ch.ee[j][5] = std::sin(kEeStaticDh[j][3]);
    }
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t lds = (size_t)3 * nfft * sizeof(double);  // <= 48 KiB
    hipLaunchKernelGGL(metrics_rows_kernel, dim3(B), dim3(kMetricsThreads), lds, ctx->stream, X_dev, B, N, dt, nfft, step, ch, out_dev);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

// edmp_select_row_dev and edmp_scenes_select_rows_dev behind their own state and pointer checks: the pick inside each of S segments of B rows
static int select_rows(edmp_ctx* ctx, const char* what, const float* volumes_dev, const double* key_dev, int S, int B, double trust_region,
                       int* index_host) {
    EDMP_REQUIRE(!std::isnan(trust_region) && trust_region >= 0.0, "%s: trust_region must be >= 0 (got %g)", what, trust_region);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = ctx_small_ints(ctx)) return rc;
    hipLaunchKernelGGL(select_row_kernel, dim3(S), dim3(kMetricsThreads), 0, ctx->stream, volumes_dev, key_dev, B, trust_region, ctx->d_int);
    EDMP_HIP_CHECK(hipGetLastError());
    EDMP_HIP_CHECK(hipMemcpyAsync(index_host, ctx->d_int, S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return EDMP_OK;
}

extern "C" int edmp_select_row_dev(edmp_ctx* ctx, const float* volumes_dev, const double* key_dev, int B, double trust_region, int* index_host) {
    EDMP_REQUIRE(ctx && volumes_dev && key_dev && index_host && B >= 1, "edmp_select_row_dev: need a context, volumes, key, index and B >= 1");
    return select_rows(ctx, "edmp_select_row_dev", volumes_dev, key_dev, 1, B, trust_region, index_host);  // (needs no guide: any binding will do)
}

extern "C" int edmp_scenes_select_rows_dev(edmp_ctx* ctx, const float* volumes_dev, const double* key_dev, int S, int B, double trust_region,
                                           int* index_host) {
    EDMP_REQUIRE_SCENE_BATCH(ctx, S, B, "edmp_scenes_select_rows_dev");
    EDMP_REQUIRE(volumes_dev && key_dev && index_host, "edmp_scenes_select_rows_dev: need volumes, key and index");
    return select_rows(ctx, "edmp_scenes_select_rows_dev", volumes_dev, key_dev, S, B, trust_region, index_host);
}
