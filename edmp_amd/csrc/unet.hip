// unet.hip — TemporalUNet eps-prediction for gfx950 (MI355X), fp32 end to end.
//
// Replaces TemporalUNet.forward and the blocks it is built from (reference: diffusion/models/temporalunet.py:47-76,
// diffusion/models/blocks.py:13-34 Conv1dBlock, :38-92 time embedding, :137-166 ResidualConvolutionBlock,
// :202-260 Down/Middle/Up samplers).  Design:
//   * activations live in HBM as [B][L][C] fp32 (channels innermost); conv weights are repacked once at load into MFMA
//     B-fragment streams (wide.hip: pack_fragments) that the kernels read straight into registers.
//   * all matrix work is exact-fp32 MFMA.  Round-2 kernel families of the full-size network (42 launches per forward):
//       wide_conv_kernel (wide.hip)   every level with >= 128 channels: the position-tile kernel - Conv1d k5 + bias +
//                                     GroupNorm + Mish + add (+ folded residual 1x1 conv), k3s2 / ConvTranspose resamplers,
//                                     Karatsuba forms at L = 2 / L = 4
//       level_kernel (level.hip)      the 32/64-channel levels: two residual blocks + resampling conv (+ final conv) per launch
//     and, for architectures those have no instance for (the tiny test networks) or EDMP_NO_FUSED / EDMP_NO_LEVEL runs, the
//     round-1 kernels of this file: conv_mfma_kernel (generic implicit GEMM), rcb_rows_kernel, rcb_block_kernel, gn_mish_kernel.
//     Taps that fall into the zero padding are never issued.
//   * the whole time-embedding MLP chain depends on t only and is precomputed for t = 1..T at load (time_table_kernel).
//   * the layer program (which kernel, which buffers) is built once in edmp_unet_load / edmp_unet_load_packed (unet_build):
//       1. the architecture walk (Walk), layout-only and unbound: image size and layout id, buffer count and size, time-bias
//          stride, every refusal.  No weights are read, nothing is written (edmp_unet_plan_describe is this pass alone).
//       2. the device image, the activation buffers and the time-bias table are allocated.
//       3. the same walk again, bound to them (Binder): it packs the image (unless a packed one is being loaded) and emits the
//          program's ops - parameter struct, instance row, FLOP counts, name - the taps and the head / input pointers.
//     An op is stated in one place, the emitter of its kind; unet_run_program launches what the walk emitted.
#include <memory>
#include <variant>

#include "common.h"
#define EDMP_STAMPS_DEFINE 1  // unity builds with -DEDMP_STAMPS: the stamp buffer lives here
#include "params.h"

namespace edmp {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---------------------------------------------------------------------------------------------------------------
// parameter inventory (state-dict order; mirrors edmp_amd/weights.py:unet_param_shapes)
// ---------------------------------------------------------------------------------------------------------------
struct RawT {
    int64_t off;  // float offset in the flat blob
    int d0, d1, d2;
};
struct RawConvBlock {
    RawT w, b, gw, gb;
};
struct RawRCB {
    RawConvBlock cb[2];
    RawT tw, tb;
    bool has_res;
    RawT rw, rb;
    int cin, cout;
};
struct RawNet {
    RawT t1w, t1b, t3w, t3b;
    std::vector<RawRCB> rcbs;  // down (2 per level), middle (2), up (2 per level)
    std::vector<RawT> down_w, down_b, up_w, up_b;
    RawConvBlock final_cb;
    RawT final_w, final_b;
    int64_t total = 0;
};

static RawT take(int64_t& off, int d0, int d1 = 1, int d2 = 1) {
    RawT t{off, d0, d1, d2};
    off += (int64_t)d0 * d1 * d2;
    return t;
}
static RawConvBlock take_cb(int64_t& off, int cin, int cout, int k) {
    RawConvBlock c;
    c.w = take(off, cout, cin, k);
    c.b = take(off, cout);
    c.gw = take(off, cout);
    c.gb = take(off, cout);
    return c;
}
static RawRCB take_rcb(int64_t& off, int cin, int cout, int time_dim) {
    RawRCB r;
    r.cin = cin;
    r.cout = cout;
    r.cb[0] = take_cb(off, cin, cout, 5);
    r.cb[1] = take_cb(off, cout, cout, 5);
    r.tw = take(off, cout, time_dim);
    r.tb = take(off, cout);
    r.has_res = cin != cout;
    if (r.has_res) {
        r.rw = take(off, cout, cin, 1);
        r.rb = take(off, cout);
    }
    return r;
}
static RawNet inventory(const edmp_unet_desc& d) {
    RawNet n;
    int64_t off = 0;
    std::vector<int> dm{d.input_dim};
    for (int i = 0; i < d.n_levels; ++i) dm.push_back(d.dims[i]);
    const int td = d.time_dim;
    n.t1w = take(off, td * 4, td);
    n.t1b = take(off, td * 4);
    n.t3w = take(off, td, td * 4);
    n.t3b = take(off, td);
    const int nd = d.n_levels;
    for (int i = 0; i < nd; ++i) {
        n.rcbs.push_back(take_rcb(off, dm[i], dm[i + 1], td));
        n.rcbs.push_back(take_rcb(off, dm[i + 1], dm[i + 1], td));
        if (i != nd - 1) {
            n.down_w.push_back(take(off, dm[i + 1], dm[i + 1], 3));
            n.down_b.push_back(take(off, dm[i + 1]));
        }
    }
    n.rcbs.push_back(take_rcb(off, dm[nd], dm[nd], td));
    n.rcbs.push_back(take_rcb(off, dm[nd], dm[nd], td));
    for (int i = nd; i > 1; --i) {
        n.rcbs.push_back(take_rcb(off, dm[i] * 2, dm[i - 1], td));
        n.rcbs.push_back(take_rcb(off, dm[i - 1], dm[i - 1], td));
        n.up_w.push_back(take(off, dm[i - 1], dm[i - 1], 4));
        n.up_b.push_back(take(off, dm[i - 1]));
    }
    n.final_cb = take_cb(off, dm[1], dm[1], 5);
    n.final_w = take(off, d.input_dim, dm[1], 1);
    n.final_b = take(off, d.input_dim);
    n.total = off;
    return n;
}

// ---------------------------------------------------------------------------------------------------------------
// device program
// ---------------------------------------------------------------------------------------------------------------
// OP_RCB: Conv1dBlock of a wide level on wide_conv_kernel; OP_WRS: down/up-sampling conv of a wide level on wide_conv_kernel;
// OP_LVL: a whole 32/64-channel level (level.hip); OP_CONV / OP_GN: the generic fallback (any architecture)
enum OpKind { OP_CONV = 0, OP_GN = 1, OP_RCB = 2, OP_WRS = 4, OP_LVL = 5 };
struct ConvInst;    // rows of the instance tables (below, behind the kernels)
struct LevelInst;
struct Level2Inst;
// One op of the layer program, as the architecture walk (Walk, below) emits it and unet_run_program launches it.
struct Op {
    OpKind kind;
    // the kernel parameters of the op's kind (OP_RCB and OP_WRS: RcbP), complete but for what a launch sets: B, the time-bias
    // pointers of step t and the step tail
    std::variant<ConvP, GnP, RcbP, LevelP> p;
    const ConvP& cv() const { return std::get<ConvP>(p); }
    const GnP& gn() const { return std::get<GnP>(p); }
    const RcbP& rc() const { return std::get<RcbP>(p); }
    const LevelP& lv() const { return std::get<LevelP>(p); }
    const ConvInst* inst = nullptr;       // OP_RCB / OP_WRS: the instance the walk chose (choose_conv)
    const LevelInst* lv_inst = nullptr;   // OP_LVL (choose_level)
    const Level2Inst* lv_pair = nullptr;  // OP_LVL: set = this level and the NEXT op (the following level) run as one launch (level.hip: level2_kernel)
    int tb1 = -1, tb2 = -1;  // offsets into the time-bias row, -1 = none.  OP_RCB / OP_GN: tb1 (a block's conv1); OP_LVL: the level's two blocks

    double flops_nominal = 0, flops_exec = 0;  // per trajectory: every tap | MFMA work actually issued (padding taps skipped, Karatsuba forms)
    double flops_direct = 0;                   // per trajectory: the direct form with padding taps skipped (round-1 'executed' accounting)
    double flops_bf16 = 0;                     // per trajectory: MFMA work issued on the bf16 pipe (bf3.hip ops: 6 partial products x the direct form; else 0)
    char name[64] = {};                        // kernel instance as rocprofv3 prints it (without the edmp:: prefix)
    KernelAttrs attrs;                         // bf16x3 ops: what the runtime reports for the instance (check_bf3_cu_claim); else zeros
};
// The second level of a merged pair runs inside the launch of the op before it; an op is a launch of its own (timed, counted, carrying
// FLOPs) unless it is that second level or a GroupNorm of the generic path (which rides untimed behind its conv).
static bool second_of_pair(const std::vector<Op>& prog, size_t i) { return i > 0 && prog[i - 1].lv_pair; }
static bool own_launch(const std::vector<Op>& prog, size_t i) { return prog[i].kind != OP_GN && !second_of_pair(prog, i); }

struct UNet {
    edmp_unet_desc desc{};
    int max_batch = 0;
    float* wpack = nullptr;    // repacked conv weights + biases + gn affine
    size_t wpack_floats = 0;
    float* tbias = nullptr;    // [T][tb_stride]
    int tb_stride = 0;
    std::vector<float*> bufs;  // activation buffers
    size_t buf_cap = 0;        // floats per buffer
    std::vector<Op> prog;
    float* x_in = nullptr;   // [B][N][8]
    float* h_last = nullptr;  // [B][N][C1] input of the 1x1 head
    const float* head_w = nullptr;
    const float* head_b = nullptr;
    int head_cin = 0;
    // taps of intermediate activations for parity (buffer, C, L); valid right after a forward
    struct Tap { int which; const float* p; int C, L; };
    std::vector<Tap> taps;
    double flops_nominal = 0, flops_exec = 0, flops_direct = 0;
    double flops_bf16 = 0, flops_f32_moved = 0;  // issued on the bf16 pipe | the fp32 work (direct form) those ops replace
    int layout = 0;  // layout id of the packed weight image (Packer::layout_id)
};

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------

// (B, C, N) f32 -> [B][N][CP] f32 with zero padding of channels C..CP-1.
__global__ void pack_input_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int N, int CP) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;  // over B*N*CP
    int total = B * N * CP;
    if (i >= total) return;
    int c = i % CP;
    int l = (i / CP) % N;
    int b = i / (CP * N);
    out[i] = (c < C) ? x[((size_t)b * C + c) * N + l] : 0.0f;
}


// Implicit-GEMM Conv1d / ConvTranspose1d on the fp32 MFMA.  Block = 256 threads = 4 waves, tile BM samples x BN
// output channels at ONE output position; K runs over (valid tap, source, channel chunk of KC).
// LDS tiles are [rows][KC + 4] so that the ds_read_b128 of a 16-lane group hits 16 distinct 4-bank slots.
// The valid taps of one output position form an arithmetic sequence (tap = k0 + i*dk, input position = l0 + i*dl), so
// the whole K walk is scalar arithmetic; global loads are unconditional (row indices clamped, results masked at the
// store) so that the loop body is straight-line: 4 global_load_dwordx4, 8 ds_read_b128, 16 MFMA, 4 ds_write_b128.
template <int BM, int BN, int KC>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvP p) {
    constexpr int LDK = KC + 4;
    constexpr int WN = BN / 32;
    constexpr int F4R = KC / 4;
    constexpr int A_F4 = BM * F4R;
    constexpr int B_F4 = BN * F4R;
    constexpr int A_IT = (A_F4 + 255) / 256;
    constexpr int B_IT = (B_F4 + 255) / 256;
    constexpr bool A_FULL = (A_F4 % 256) == 0;
    constexpr bool B_FULL = (B_F4 % 256) == 0;
    constexpr int STAGE = (BM + BN) * LDK;  // floats per pipeline stage: A tile then B tile
    constexpr int TS = BN + 4;              // row stride of the output tile staged for the float4 store pass
    constexpr int LDS_FL = (2 * STAGE > BM * TS) ? 2 * STAGE : BM * TS;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FL];

#define EDMP_CSTAMP(i) if constexpr (BM == 64 && BN == 64 && KC == 64) { EDMP_STAMP(6, i) }
    EDMP_CSTAMP(0)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ntn = (p.Cout + BN - 1) / BN;
    const int lo = blockIdx.y / ntn;
    const int n0 = (blockIdx.y % ntn) * BN;
    const int b0 = blockIdx.x * BM;
    const int Cin = p.C1 + p.C2;

    int k0, dk, l0, dl, nvt;
    if (!p.transposed) {  // li = lo*stride + k - pad must lie in [0, Lin)
        const int base = lo * p.stride - p.pad;
        const int kmin = max(0, -base);
        const int kmax = min(p.ntaps - 1, p.Lin - 1 - base);
        k0 = kmin;
        dk = 1;
        l0 = base + kmin;
        dl = 1;
        nvt = max(0, kmax - kmin + 1);
    } else {  // li*stride + k - pad = lo  ->  k = r + i*stride, li = (lo + pad - r)/stride - i
        const int r = (lo + p.pad) % p.stride;
        const int li_first = (lo + p.pad - r) / p.stride;
        const int i_lo = max(0, li_first - (p.Lin - 1));
        const int i_hi = (p.ntaps - 1 - r) >= 0 ? min(li_first, (p.ntaps - 1 - r) / p.stride) : -1;
        k0 = r + i_lo * p.stride;
        dk = p.stride;
        l0 = li_first - i_lo;
        dl = -1;
        nvt = max(0, i_hi - i_lo + 1);
    }
    const int ch1 = p.C1 / KC, ch2 = p.C2 / KC;
    const int cpt = ch1 + ch2;  // chunks per tap
    const int nK = nvt * cpt;

    // per-thread, chunk-invariant parts of the global addresses (element offsets).  Scalars, not arrays: hipcc keeps
    // small runtime-looking arrays in scratch memory once scheduling barriers are present.
#define EDMP_DECL_A(i)                                                     \
    const int fa##i = tid + i * 256;                                       \
    const int ba##i = min(b0 + fa##i / F4R, p.B - 1);                      \
    const int a1_##i = ba##i * p.Lin * p.C1 + (fa##i % F4R) * 4;           \
    const int a2_##i = ba##i * p.Lin * p.C2 + (fa##i % F4R) * 4;           \
    const int al_##i = (fa##i / F4R) * LDK + (fa##i % F4R) * 4;            \
    const bool ap_##i = (i < A_IT) && (A_FULL || fa##i < A_F4);            \
    float4 ra##i = make_float4(0.f, 0.f, 0.f, 0.f);
#define EDMP_DECL_B(i)                                                     \
    const int fb##i = tid + i * 256;                                       \
    const int w_##i = min(n0 + fb##i / F4R, p.Cout - 1) * Cin + (fb##i % F4R) * 4; \
    const int bl_##i = BM * LDK + (fb##i / F4R) * LDK + (fb##i % F4R) * 4; \
    const bool bp_##i = (i < B_IT) && (B_FULL || fb##i < B_F4);            \
    float4 rb##i = make_float4(0.f, 0.f, 0.f, 0.f);
    EDMP_DECL_A(0) EDMP_DECL_A(1) EDMP_DECL_A(2) EDMP_DECL_A(3)
    EDMP_DECL_B(0) EDMP_DECL_B(1) EDMP_DECL_B(2) EDMP_DECL_B(3)
    static_assert(A_IT <= 4 && B_IT <= 4, "tile too large for the staging code");
    int ld_ti = 0, ld_cc = 0;  // next chunk to fetch (block-uniform)

#define EDMP_LDA(i) \
    if (ap_##i) ra##i = *reinterpret_cast<const float4*>(abase_ + (first_ ? a1_##i : a2_##i));
#define EDMP_LDB(i) \
    if (bp_##i) rb##i = *reinterpret_cast<const float4*>(wbase_ + w_##i);
// issue the global loads of chunk (ld_ti, ld_cc) and advance the chunk cursor
#define EDMP_LOAD_NEXT()                                                                                      \
    {                                                                                                         \
        const int tap_ = k0 + ld_ti * dk;                                                                     \
        const int li_ = l0 + ld_ti * dl;                                                                      \
        const bool first_ = ld_cc < ch1;                                                                      \
        const float* src_ = first_ ? p.src1 : p.src2;                                                         \
        const int Cs_ = first_ ? p.C1 : p.C2;                                                                 \
        const int ci0_ = (first_ ? ld_cc : ld_cc - ch1) * KC;                                                 \
        const float* abase_ = src_ + (size_t)li_ * Cs_ + ci0_;                                                \
        const float* wbase_ = p.W + (size_t)tap_ * p.Cout * Cin + (first_ ? 0 : p.C1) + ci0_;                 \
        EDMP_LDA(0) EDMP_LDA(1) EDMP_LDA(2) EDMP_LDA(3) EDMP_LDB(0) EDMP_LDB(1) EDMP_LDB(2) EDMP_LDB(3)                              \
        if (++ld_cc == cpt) {                                                                                 \
            ld_cc = 0;                                                                                        \
            ++ld_ti;                                                                                          \
        }                                                                                                     \
    }
#define EDMP_STA(i) \
    if (ap_##i) *reinterpret_cast<float4*>(st_ + al_##i) = ra##i;
#define EDMP_STB(i) \
    if (bp_##i) *reinterpret_cast<float4*>(st_ + bl_##i) = rb##i;
#define EDMP_STORE_STAGE(buf)                                                     \
    {                                                                             \
        float* st_ = lds + (buf) * STAGE;                                         \
        EDMP_STA(0) EDMP_STA(1) EDMP_STA(2) EDMP_STA(3) EDMP_STB(0) EDMP_STB(1) EDMP_STB(2) EDMP_STB(3) \
    }

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    // requested now, used by the store epilogue: loaded there it would expose a full memory round trip
    const float bias_v = p.bias[min(n0 + wn * 32 + (lane & 31), p.Cout - 1)];

    const int arow = (wm * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    const int brow = BM * LDK + (wn * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    if (nK > 0) {
        EDMP_LOAD_NEXT();
        EDMP_STORE_STAGE(0);
        __syncthreads();
        EDMP_CSTAMP(1)
        // steady state: every iteration prefetches chunk kk+1 while the MFMAs consume chunk kk
        for (int kk = 0; kk < nK - 1; ++kk) {
            const int cur = kk & 1;
            EDMP_LOAD_NEXT();
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMAs (hipcc otherwise sinks it)
            const float* a_s = lds + cur * STAGE + arow;
            const float* b_s = lds + cur * STAGE + brow;
#pragma unroll
            for (int j = 0; j < KC / 8; ++j) {
                const float4 a4 = *reinterpret_cast<const float4*>(a_s + 8 * j);
                const float4 b4 = *reinterpret_cast<const float4*>(b_s + 8 * j);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            EDMP_STORE_STAGE(cur ^ 1);
            __syncthreads();
        }
        {  // last chunk: nothing left to prefetch
            const int cur = (nK - 1) & 1;
            const float* a_s = lds + cur * STAGE + arow;
            const float* b_s = lds + cur * STAGE + brow;
#pragma unroll
            for (int j = 0; j < KC / 8; ++j) {
                const float4 a4 = *reinterpret_cast<const float4*>(a_s + 8 * j);
                const float4 b4 = *reinterpret_cast<const float4*>(b_s + 8 * j);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
            }
        }
    }
#undef EDMP_LOAD_NEXT
#undef EDMP_STORE_STAGE
#undef EDMP_LDA
#undef EDMP_LDB
#undef EDMP_STA
#undef EDMP_STB
#undef EDMP_DECL_A
#undef EDMP_DECL_B

    EDMP_CSTAMP(2)
    // epilogue: + bias, store [b][lo][co].  acc[r]: row = (r&3) + 8*(r>>2) + 4*(lane>>5), col = lane&31.
    // Sixteen dword stores per lane are store-issue-bound (~4.8 k cycles measured); the tile is transposed through LDS
    // instead and leaves as BM*BN/1024 float4 stores per thread (128-byte runs along the channels).
    const int co = n0 + wn * 32 + (lane & 31);
    if ((p.Cout & 3) == 0) {
        __syncthreads();  // every wave is done with the stages
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            lds[(wm * 32 + row) * TS + wn * 32 + (lane & 31)] = acc[r] + bias_v;
        }
        __syncthreads();
        constexpr int NF = (BM * (BN / 4) + 255) / 256;
#pragma unroll
        for (int it = 0; it < NF; ++it) {
            const int f = tid + it * 256;
            const int row = f / (BN / 4), c4 = (f % (BN / 4)) * 4;
            const int b = b0 + row;
            if (f < BM * (BN / 4) && b < p.B && n0 + c4 < p.Cout)
                *reinterpret_cast<float4*>(p.dst + ((size_t)b * p.Lout + lo) * p.Cout + n0 + c4) = *reinterpret_cast<const float4*>(lds + row * TS + c4);
        }
    } else if (co < p.Cout) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            int b = b0 + wm * 32 + row;
            if (b < p.B) p.dst[((size_t)b * p.Lout + lo) * p.Cout + co] = acc[r] + bias_v;
        }
    }
    EDMP_CSTAMP(3)
#undef EDMP_CSTAMP
}

}  // namespace edmp
#include "wide.hip"
#include "bf3.hip"
#include "level.hip"
#include "kernel_instances.h"
namespace edmp {
#ifdef EDMP_SHARDED  // the position-tile and whole-level kernels are compiled in parallel translation units (kernel_shard.hip)
#define EDMP_X(sh, K, MS, CG, GS, L, R) extern template int launch_wide_t<K, MS, CG, GS, L, R>(const RcbP&, hipStream_t);
EDMP_WIDE_INSTANCES(EDMP_X)
#undef EDMP_X
#define EDMP_X(sh, K, MS, CG, GS, L, R) extern template int launch_bf3_t<K, MS, CG, GS, L, R>(const RcbP&, hipStream_t, KernelAttrs*);
EDMP_BF3_INSTANCES(EDMP_X)
#undef EDMP_X
#define EDMP_X(sh, M, C, L, SB, CIN) extern template int launch_level_t<M, C, L, SB, CIN>(const LevelP&, hipStream_t);
EDMP_LEVEL_INSTANCES(EDMP_X)
#undef EDMP_X
#define EDMP_X(sh, MA, CA, LA, CINA, MB, CB, LB, CINB, SB) extern template int launch_level2_t<MA, CA, LA, CINA, MB, CB, LB, CINB, SB>(const LevelP&, const LevelP&, hipStream_t);
EDMP_LEVEL2_INSTANCES(EDMP_X)
#undef EDMP_X
#endif

// ---- the instance tables: the lists of kernel_instances.h expanded once more, into rows of {template arguments, launcher}.
// A layer has a kernel instance exactly when its row exists (find_*); the walk's op keeps the row (choose_conv / choose_level /
// choose_pair below), and the packer's arguments, the launch and the printed kernel name all come from it.  These expansions are
// the only place in this file that spells a template argument list (the unity build instantiates the kernels through them).
struct ConvInst {  // wide.hip (fp32 MFMA) | bf3.hip (bf16x3: exact products on the bf16 matrix pipe)
    bool bf3;
    int kind, ms, cg, gs, L;  // WideKind, samples per workgroup, channels per workgroup, channels per GroupNorm group, input positions
    bool res;                 // folds the block's residual 1x1 conv
    int (*launch)(const RcbP&, hipStream_t, KernelAttrs*);  // KernelAttrs*: launch_bf3_t's query mode (ignored by a wide.hip row)
};
static const ConvInst kConvInst[] = {
#define EDMP_X(sh, K, MS, CG, GS, L, R) {false, K, MS, CG, GS, L, R, [](const RcbP& p, hipStream_t s, KernelAttrs*) { return launch_wide_t<K, MS, CG, GS, L, R>(p, s); }},
    EDMP_WIDE_INSTANCES(EDMP_X)
#undef EDMP_X
#define EDMP_X(sh, K, MS, CG, GS, L, R) {true, K, MS, CG, GS, L, R, &launch_bf3_t<K, MS, CG, GS, L, R>},
    EDMP_BF3_INSTANCES(EDMP_X)
#undef EDMP_X
};
struct LevelInst {  // level.hip: a whole 32/64-channel level
    int mode, C, L, sb, cin;  // LevelMode, channels, positions, samples per workgroup, stored input channels
    int (*launch)(const LevelP&, hipStream_t);
};
static const LevelInst kLevelInst[] = {
#define EDMP_X(sh, M, C, L, SB, CIN) {M, C, L, SB, CIN, &launch_level_t<M, C, L, SB, CIN>},
    EDMP_LEVEL_INSTANCES(EDMP_X)
#undef EDMP_X
};
struct Level2Inst {  // level.hip: two consecutive levels in one launch (level2_kernel)
    int ma, ca, la, cina, mb, cb, lb, cinb, sb;
    int (*launch)(const LevelP&, const LevelP&, hipStream_t);
};
static const Level2Inst kLevel2Inst[] = {
#define EDMP_X(sh, MA, CA, LA, CINA, MB, CB, LB, CINB, SB) {MA, CA, LA, CINA, MB, CB, LB, CINB, SB, &launch_level2_t<MA, CA, LA, CINA, MB, CB, LB, CINB, SB>},
    EDMP_LEVEL2_INSTANCES(EDMP_X)
#undef EDMP_X
};
static const ConvInst* find_conv(bool bf3, int kind, int ms, int cg, int gs, int L, bool res) {
    for (const ConvInst& r : kConvInst)
        if (r.bf3 == bf3 && r.kind == kind && r.ms == ms && r.cg == cg && r.gs == gs && r.L == L && r.res == res) return &r;
    return nullptr;
}
static const LevelInst* find_level(int mode, int C, int L, int sb, int cin) {
    for (const LevelInst& r : kLevelInst)
        if (r.mode == mode && r.C == C && r.L == L && r.sb == sb && r.cin == cin) return &r;
    return nullptr;
}
static const Level2Inst* find_level2(const LevelInst& a, const LevelInst& b) {  // (the pair's tile height is its own)
    for (const Level2Inst& r : kLevel2Inst)
        if (r.ma == a.mode && r.ca == a.C && r.la == a.L && r.cina == a.cin && r.mb == b.mode && r.cb == b.C && r.lb == b.L && r.cinb == b.cin) return &r;
    return nullptr;
}
}  // namespace edmp
namespace edmp {

// GroupNorm(8 groups, eps 1e-5, biased variance) -> Mish -> (+ time bias[c] | + residual[b,l,c]) in place.
// One wave per (sample, group); the (C/8) x L elements of the group stay in registers between the passes.
template <int EPL>  // elements per lane
__global__ __launch_bounds__(256) void gn_mish_kernel(GnP p) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);  // global wave = b*8 + g
    if (gw >= p.B * 8) return;
    const int b = gw >> 3, g = gw & 7;
    const int cg = p.C >> 3;
    const int n = cg * p.L;
    float* base = p.y + (size_t)b * p.L * p.C + g * cg;
    float v[EPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        int e = lane + i * 64;
        float x = 0.f;
        if (e < n) {
            int l = e / cg, c = e - l * cg;
            x = base[(size_t)l * p.C + c];
        }
        v[i] = x;
        s += x;
    }
    const float mean = wave_sum(s) / (float)n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        int e = lane + i * 64;
        float d = (e < n) ? (v[i] - mean) : 0.f;
        q += d * d;
    }
    const float var = wave_sum(q) / (float)n;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        int e = lane + i * 64;
        if (e < n) {
            int l = e / cg, c = e - l * cg;
            int ch = g * cg + c;
            float scale = rstd * p.gamma[ch];
            float shift = p.beta[ch] - scale * mean;
            float y = mish_fast(v[i] * scale + shift);
            if (p.add_tbias) y += p.add_tbias[ch];
            if (p.add_res) y += p.add_res[((size_t)b * p.L + l) * p.C + ch];
            base[(size_t)l * p.C + c] = y;
        }
    }
}

// final 1x1 conv (final_conv.1, temporalunet.py:36): h [B][N][Cin] -> eps (B, Cout, N) in the reference layout.
__global__ void head_1x1_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                float* __restrict__ eps, int B, int N, int Cin, int Cout) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;  // over B*N
    if (i >= B * N) return;
    int b = i / N, l = i - b * N;
    const float* hp = h + (size_t)i * Cin;
    for (int co = 0; co < Cout; ++co) {
        float a = bias[co];
        for (int ci = 0; ci < Cin; ++ci) a = fmaf(hp[ci], w[co * Cin + ci], a);
        eps[((size_t)b * Cout + co) * N + l] = a;
    }
}

// [B][L][C] -> (B, C, L)   (parity/debug only)
__global__ void unpack_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int L, int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L * C) return;
    int l = i % L;
    int c = (i / L) % C;
    int b = i / (L * C);
    dst[i] = src[((size_t)b * L + l) * C + c];
}

// time-bias table: for t = 1..T (blockIdx.x = t-1): temb = Linear(Mish(Linear(sinusoid(t))));  row[c] = tb[c] +
// sum_k tw[c][k] * Mish(temb[k]) for the concatenated per-RCB time MLPs.  blocks.py:46-54, 83-88, 64-67.
__global__ void time_table_kernel(const float* __restrict__ t1w, const float* __restrict__ t1b, const float* __restrict__ t3w,
                                  const float* __restrict__ t3b, const float* __restrict__ tw, const float* __restrict__ tb,
                                  float* __restrict__ out, int time_dim, int stride) {
    extern __shared__ float sm[];  // emb[time_dim] | hid[4*time_dim] | temb[time_dim]
    float* emb = sm;
    float* hid = sm + time_dim;
    float* temb = hid + 4 * time_dim;
    const float t = (float)(blockIdx.x + 1);
    const int half = time_dim / 2;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        float e = (float)(log(10000.0) / (double)(half - 1));  // python float, then cast when multiplied into f32
        float f = expf((float)i * -e);
        float a = t * f;
        emb[i] = sinf(a);
        emb[i + half] = cosf(a);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 4 * time_dim; o += blockDim.x) {
        float a = t1b[o];
        for (int k = 0; k < time_dim; ++k) a = fmaf(emb[k], t1w[o * time_dim + k], a);
        hid[o] = mish_f(a);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < time_dim; o += blockDim.x) {
        float a = t3b[o];
        for (int k = 0; k < 4 * time_dim; ++k) a = fmaf(hid[k], t3w[o * 4 * time_dim + k], a);
        temb[o] = mish_f(a);  // every consumer applies Mish first (TimeMLP, blocks.py:64-67)
    }
    __syncthreads();
    for (int c = threadIdx.x; c < stride; c += blockDim.x) {
        float a = tb[c];
        for (int k = 0; k < time_dim; ++k) a = fmaf(temb[k], tw[(size_t)c * time_dim + k], a);
        out[(size_t)blockIdx.x * stride + c] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host: load / build program
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int KC>
static void launch_conv_t(const ConvP& p, hipStream_t s) {
    dim3 grid((p.B + BM - 1) / BM, p.Lout * ((p.Cout + BN - 1) / BN));
    hipLaunchKernelGGL((conv_mfma_kernel<BM, BN, KC>), grid, dim3(256), 0, s, p);
}
static int pick_kc(int c1, int c2) {
    auto ok = [&](int kc) { return c1 % kc == 0 && (c2 == 0 || c2 % kc == 0); };
    return ok(64) ? 64 : ok(32) ? 32 : ok(16) ? 16 : 8;
}
static void launch_conv(const ConvP& p, hipStream_t s) {
    const int kc = pick_kc(p.C1, p.C2);
    const bool wide = (p.Cout % 64 == 0);
    if (wide) {
        if (kc == 64) launch_conv_t<64, 64, 64>(p, s);
        else if (kc == 32) launch_conv_t<64, 64, 32>(p, s);
        else if (kc == 16) launch_conv_t<64, 64, 16>(p, s);
        else launch_conv_t<64, 64, 8>(p, s);
    } else {
        if (kc >= 32) launch_conv_t<128, 32, 32>(p, s);
        else if (kc == 16) launch_conv_t<128, 32, 16>(p, s);
        else launch_conv_t<128, 32, 8>(p, s);
    }
}
static int launch_gn(const GnP& p, hipStream_t s) {
    const int n = (p.C / 8) * p.L;
    dim3 grid((p.B * 8 + 3) / 4);
    if (n <= 128) hipLaunchKernelGGL((gn_mish_kernel<2>), grid, dim3(256), 0, s, p);
    else if (n <= 256) hipLaunchKernelGGL((gn_mish_kernel<4>), grid, dim3(256), 0, s, p);
    else if (n <= 512) hipLaunchKernelGGL((gn_mish_kernel<8>), grid, dim3(256), 0, s, p);
    else {
        set_error("GroupNorm group of %d elements exceeds the register-resident limit (512)", n);
        return EDMP_ERR_ARG;
    }
    return EDMP_OK;
}

// Builder switches, read from the environment ONCE WHEN A MODEL IS BUILT (BuildSwitches::read, the only getenv of this file) and
// frozen into its layer program and packed-image layout id: two models built under different settings can live side by side
// in one process (A/B runs, the adversarial-weights test).
//   EDMP_NO_FUSED / EDMP_NO_RESFOLD / EDMP_NO_LEVEL: every conv on the generic kernels | the residual 1x1 conv as its own launch |
//     no whole-level kernels.
//   EDMP_NO_KARATSUBA=1: the L = 2 convolutions of the 512-channel levels in the direct form instead of the Karatsuba form (3 instead
//     of 4 matrix products; wide.hip WK_K5K2) and the L = 4 convolutions of the 256/512-channel levels (nested form, 9 instead of 14
//     products; WK_K5K4).
//   EDMP_BF16X3=<mask>: bf16x3 split (bf3.hip): the direct-form instances whose weights meet >= 7 positions run on the bf16 matrix
//     pipe with exact products and fp32 accumulation - measured x1.2-1.55 per launch at HALF the fp32-MFMA kernel's error against
//     float64 (profiles/r06_bf16x3.md).  Bits: kConvFamilies below.  0 = every conv on the fp32-MFMA kernels (bench.py's A/B leg).
//   EDMP_MS16=<mask>: 16-sample tiles for DIRECT-form fp32 instances of the 256 / 512-channel levels (choose_conv).  Bits: kConvFamilies.
//   EDMP_LEVEL_SB=<d1><d2><d3><d4> (digits 2 / 4): samples per workgroup of the level kernels - down level at 32 channels, down level at
//     64, up level, last up level.  4 = one workgroup per CU at B = 1024; 2 = two co-resident workgroups per CU (two waves per SIMD: one
//     workgroup's GroupNorm / Mish epilogues, barriers and staging run under the other's MFMAs).
//   EDMP_LEVEL_MERGE=<mask>: bit 0 = the two down levels of the 32/64-channel resolutions as ONE launch, level 1's k3s2 output handed to
//     level 2 in LDS (level.hip: level2_kernel; two samples per workgroup); bit 1 = the two last up levels likewise, the ConvTranspose
//     output of the 64-channel level going into the first half of the last level's input tile (the skip half still comes from HBM).
static const int kBf3Default = 0xff;  // same-box bench A/Bs (profiles/r06_bf16x3.md): 0 -> 1 001 k, 0x7 -> 1 083 k, 0x3f -> 1 102 k traj-steps/s; another box: 0x3f 1 067 k, 0x7f 1 101 k, 0xbf 1 087 k, 0xff -> 1 120 k
static const int kMs16Default = 0x05;  // same-box bench A/B, three alternated runs each: 986.5 k -> 989.8 k traj-steps/s (profiles/r05_forkjoin.md); bits 1, 3, 4 measured x0.98-1.01 per launch: off
static const char kLevelSbDefault[] = "4222";  // same-box A/B (scripts/ab_models.py, round 3): -1.2 / -1.6 / -2.8 us per launch for digits 2 / 3 / 4, nothing for 1
static const int kLevelMergeDefault = 0x3;  // same-box bench A/B, three alternated runs each: bit 0 986.5 k -> 988.2 k; bits 0 + 1 993.8 k -> 997.7 k, bit 1 alone 992.5 k (profiles/r05_level_kernels.md)
struct BuildSwitches {
    bool fused, resfold, level, karatsuba;
    int bf3, ms16, level_merge;  // masks
    int level_sb[4];
    static BuildSwitches read() {
        auto env = [](const char* name) { return getenv(name); };
        auto mask = [&](const char* name, int dflt) { const char* e = env(name); return e ? (int)strtol(e, nullptr, 0) : dflt; };
        BuildSwitches s;
        s.fused = env("EDMP_NO_FUSED") == nullptr;
        s.resfold = env("EDMP_NO_RESFOLD") == nullptr;
        s.level = s.fused && env("EDMP_NO_LEVEL") == nullptr;
        s.karatsuba = env("EDMP_NO_KARATSUBA") == nullptr;
        s.bf3 = mask("EDMP_BF16X3", kBf3Default);
        s.ms16 = mask("EDMP_MS16", kMs16Default);
        s.level_merge = mask("EDMP_LEVEL_MERGE", kLevelMergeDefault);
        const char* e = env("EDMP_LEVEL_SB");
        for (int d = 0; d < 4; ++d) s.level_sb[d] = ((e && strlen(e) == 4) ? e : kLevelSbDefault)[d] == '2' ? 2 : 4;
        return s;
    }
};

// packing forms of the weight image (Packer::tag); F_FRAG .. F_FRAG_BF3 are the weight-stream layouts of the position-tile kernels
enum PackForm : uint64_t { F_CONV = 1, F_CONVT = 2, F_FRAG = 3, F_FRAG_K2 = 4, F_FRAG_K4 = 5, F_RESAMPLE = 6, F_VEC = 7, F_FRAG_BF3 = 8 };

// The conv families a switch bit governs: kind (WK_K5: a Conv1dBlock; WK_DOWN / WK_UP: the k3s2 / ConvTranspose resamplers), Cout / 8,
// L (input positions) -> bit of EDMP_BF16X3 (the family runs on bf3.hip) and bit of EDMP_MS16 (16-sample tiles on wide.hip); -1: none
static const struct { int kind, cg, L, bf3_bit, ms16_bit; } kConvFamilies[] = {
    {WK_K5, 32, 7, 0, 0},    {WK_K5, 16, 7, 1, -1},   {WK_K5, 16, 13, 2, -1},   // Conv1dBlock L = 7 / 256 ch, L = 7 / 128 ch, L = 13 / 128 ch
    {WK_K5, 64, 4, 6, -1},   {WK_K5, 32, 4, 7, -1},   // Conv1dBlock L = 4 / 512 ch, / 256 ch: direct form on the bf16 pipe instead of the nested Karatsuba form on the fp32 pipe
    {WK_DOWN, 32, 7, 3, 1},  {WK_UP, 32, 4, 3, 2},    // the resamplers at 256 channels
    {WK_DOWN, 64, 4, 4, 3},  {WK_UP, 64, 2, 4, 4},    // at 512 channels
    {WK_DOWN, 16, 13, 5, -1}, {WK_UP, 16, 7, 5, -1},  // at 128 channels
};

// What the walk decides for one conv op of a wide level (>= 128 channels), once: everything downstream - the packer (stream, row->ms),
// the FLOP counts (form), the launch and the kernel name (row) - reads it from here.
struct ConvChoice {
    const ConvInst* row[2] = {nullptr, nullptr};  // [RES]: without | with the folded residual 1x1 conv (WK_K5); family, MS, GS are the row's.  row[0] == nullptr: no instance, the generic path runs the layer
    int form = 0;                                 // 0 direct | 2 Karatsuba at L = 2 | 4 nested Karatsuba at L = 4
    PackForm stream = F_FRAG;                     // layout of the weight stream
};
// kind: WK_K5 (a Conv1dBlock; L = its length), WK_DOWN / WK_UP (L = input length); c1, c2: stored input channels (c2: the skip half of a concat)
static ConvChoice choose_conv(const BuildSwitches& sw, int kind, int cout, int L, int c1, int c2) {
    ConvChoice c;
    if (!sw.fused || cout % 8 != 0 || c1 % 32 != 0 || c2 % 32 != 0 || (c2 != 0 && c2 != c1)) return c;  // wide.hip: whole K groups, equal halves of a concat
    const int cg = cout / 8;
    int bf3_bit = -1, ms16_bit = -1;
    for (const auto& f : kConvFamilies)
        if (f.kind == kind && f.cg == cg && f.L == L) bf3_bit = f.bf3_bit, ms16_bit = f.ms16_bit;
    const bool bf3 = bf3_bit >= 0 && (sw.bf3 >> bf3_bit & 1);
    int ms, cgw = std::max(cg, 32), gs = cg;  // a workgroup covers whole GroupNorm groups, at least 32 channels
    if (bf3) {
        ms = cg >= 32 ? 32 : 16;  // bf3.hip runs the direct form: 32-sample workgroups at 256 channels and above (256 workgroups), 16 at 128
        // no GroupNorm behind a resampler, so its INSTANCE has 32-channel workgroups at every width; a launch of a 32-sample one that is
        // larger than the chip runs them in pairs, 64 channels per workgroup (bf3.hip: Bf3Cfg::PAIRABLE, the rule in launch_bf3_t)
        if (kind != WK_K5) cgw = 32, gs = std::min(cg, 32);
        c.stream = F_FRAG_BF3;
    } else {
        if (kind == WK_K5 && sw.karatsuba) c.form = (cg == 64 && L == 2) ? 2 : (cg >= 32 && L == 4) ? 4 : 0;
        // The tile height MS = samples per workgroup.  16 for the 128-channel levels (32-sample workgroups would leave half the CUs
        // idle); 32 for the Karatsuba forms of the 256 / 512-channel levels (their weight stream per FLOP doubles with 16-sample tiles:
        // 16 TB/s out of the L2s at L = 4); and for the DIRECT-form instances of the 256 / 512-channel levels 16 where EDMP_MS16 says so
        // (round 5): 512 workgroups per launch, two co-resident per CU (160 registers, 48 KB of LDS), one workgroup's prologue /
        // epilogue / barriers run under the other's fp32 MFMAs (a wave's own VALU work cannot: profiles/r05_coissue_control.md).
        // Same-stream A/B on isolated layer chains x1.06-1.08 (tools/dualbench.hip, profiles/r05_forkjoin.md).
        ms = (cg < 32 || (c.form == 0 && ms16_bit >= 0 && (sw.ms16 >> ms16_bit & 1))) ? 16 : 32;
        c.stream = c.form == 2 ? F_FRAG_K2 : c.form == 4 ? F_FRAG_K4 : F_FRAG;
    }
    const int ikind = c.form == 2 ? WK_K5K2 : c.form == 4 ? WK_K5K4 : kind;
    c.row[0] = find_conv(bf3, ikind, ms, cgw, gs, L, false);
    c.row[1] = find_conv(bf3, ikind, ms, cgw, gs, L, true);
    return c;
}
// whole-level kernel (level.hip) for a level of `C` channels and `L` positions reading c1 (+ c2: the skip) stored channels; nullptr = none
static const LevelInst* choose_level(const BuildSwitches& sw, int mode, int C, int L, int c1, int c2) {
    if (!sw.level || (mode == LV_DOWN ? c2 != 0 : c2 != c1)) return nullptr;
    const int digit = mode == LV_DOWN ? (C == 32 ? 0 : 1) : mode == LV_UP ? 2 : 3;
    return find_level(mode, C, L, sw.level_sb[digit], c1 + c2);
}
// level `a` and the level behind it as one launch (nullptr: two launches)
static const Level2Inst* choose_pair(const BuildSwitches& sw, const LevelInst* a, const LevelInst* b) {
    if (!a || !b || !(sw.level_merge >> (a->mode == LV_DOWN ? 0 : 1) & 1)) return nullptr;
    return find_level2(*a, *b);
}

// ---- the bf16x3 kernels' CU claim (bf3.hip: bf3_conv_kernel; profiles/r06_coresidency_fault.md) ------------------------------------
// A bf16x3 workgroup must own its CU: one workgroup per CU, and its waves' registers fill the 512-entry file of every SIMD
// (allocated in granules of 8 per lane), so that no wave of another kernel fits beside it.  Host-only: a function of what the
// runtime reports, unit-tested on the CPU through edmp_cu_claim.
static bool owns_cu(int regs, int block, int lds, int wg_per_cu) {
    if (regs <= 0 || block <= 0 || lds < 0) return false;
    const int alloc = (regs + 7) / 8 * 8, waves_per_simd = ((block + 63) / 64 + 3) / 4;
    const int free_regs = 512 - alloc * waves_per_simd;  // per lane, on a SIMD that holds this workgroup's waves
    const int wg_by_regs = (512 / alloc) / waves_per_simd, wg_by_lds = lds > 0 ? 160 * 1024 / lds : wg_by_regs;
    return free_regs < 8 && std::min(wg_by_regs, wg_by_lds) == 1 && wg_per_cu == 1;
}

static int check_bf3_cu_claim(UNet* u) {
    for (Op& op : u->prog) {
        if (!(op.inst && op.inst->bf3)) continue;
        if (int rc = op.inst->launch(op.rc(), nullptr, &op.attrs)) return rc;  // query mode: launches nothing
        const KernelAttrs& a = op.attrs;
        EDMP_REQUIRE(owns_cu(a.regs, a.block, a.lds, a.wg_per_cu),
                     "%s does not own its CU (%d VGPRs x %d threads, %d B of LDS, %d workgroups per CU): the bf16x3 containment of "
                     "profiles/r06_coresidency_fault.md is lost; build the model with EDMP_BF16X3=0",
                     op.name, a.regs, a.block, a.lds, a.wg_per_cu);
    }
    return EDMP_OK;
}

bool unet_complete(const UNet* u) { return u && u->wpack && u->tbias && !u->prog.empty(); }

void unet_destroy(UNet* u) {
    if (!u) return;
    if (u->wpack) (void)hipFree(u->wpack);
    if (u->tbias) (void)hipFree(u->tbias);
    for (float* b : u->bufs) (void)hipFree(b);
    delete u;
}

static inline int round8(int c) { return (c + 7) / 8 * 8; }

struct Packer {
    std::vector<float> host;
    bool dry = false;   // layout only: offsets and sizes are computed, nothing is written (loading a packed image)
    size_t total = 0;   // floats packed so far (== host.size() unless dry)
    // signature of the layout actually produced: every tensor's packing form and size, in order (FNV-1a).  The builder's
    // run-time switches (EDMP_NO_FUSED, EDMP_NO_RESFOLD, EDMP_NO_LEVEL, EDMP_NO_KARATSUBA, EDMP_BF16X3, EDMP_MS16, EDMP_LEVEL_MERGE, EDMP_LEVEL_SB) move
    // tensors or change their fragment order, several of them without changing the total: the signature is what makes an
    // image written under one setting unloadable under another
    uint64_t sig = 1469598103934665603ull;
    void tag(uint64_t v) {
        for (int i = 0; i < 8; ++i) {
            sig ^= (v >> (8 * i)) & 0xff;
            sig *= 1099511628211ull;
        }
    }
    size_t add_untagged(size_t n) {
        size_t o = total;
        total += ((n + 3) / 4) * 4;  // keep every tensor 16-byte aligned
        if (!dry) host.resize(total, 0.0f);
        return o;
    }
    size_t add(size_t n) {
        tag(n);
        return add_untagged(n);
    }
    int layout_id(int version) const { return (int)(((sig >> 32) ^ sig ^ (uint64_t)version * 2654435761ull) & 0x7fffffff); }
    // Conv1d weight (Cout, Cin, k) -> [tap][Cout][CinP]
    size_t conv(const float* w, int cout, int cin, int k, int cinp) {
        tag(F_CONV), tag(k), tag(cout), tag(cinp);
        size_t o = add((size_t)k * cout * cinp);
        if (dry) return o;
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < k; ++t) host[o + ((size_t)t * cout + co) * cinp + ci] = w[((size_t)co * cin + ci) * k + t];
        return o;
    }
    // ConvTranspose1d weight (Cin, Cout, k) -> [tap][Cout][Cin]
    size_t convT(const float* w, int cin, int cout, int k) {
        tag(F_CONVT), tag(k), tag(cout), tag(cin);
        size_t o = add((size_t)k * cout * cin);
        if (dry) return o;
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co)
                for (int t = 0; t < k; ++t) host[o + ((size_t)t * cout + co) * cin + ci] = w[((size_t)ci * cout + co) * k + t];
        return o;
    }
    // Conv1d k5 weight (Cout, Cin, 5) [+ the block's residual 1x1 conv (Cout, Cin, 1)] -> the B-fragment stream of
    // wide_conv_kernel: [Cout/32][CinP/8][slots][64][4], slots = the taps that can be valid at length L (+ the residual).
    // form, sw: the stream layout and the tile height the walk chose for the op (ConvChoice; sw is unused by F_FRAG_BF3)
    size_t conv_frag(const float* w, const float* wres, int cout, int cin, int cinp, int L, PackForm form, int sw) {
        const bool bf3 = form == F_FRAG_BF3;  // bf3.hip: stream of bf16 triples [Cout/16][CinP/32][slots][3][64][8 bf16] (counted in floats here)
        const int kt0 = (L == 2) ? 1 : 0, ntap = (L == 2) ? 3 : 5;
        const int nslot = (bf3 ? 5 : form == F_FRAG_K4 ? 9 : ntap) + (wres ? 1 : 0);  // (the nested L = 4 form: nine slots instead of five)
        tag(form), tag(cout), tag(cinp), tag(L), tag(wres ? 1 : 0);
        if (!bf3) tag(sw);
        const size_t o = add(bf3 ? bf3_stream_elems(cout, cinp, nslot) / 2 : (size_t)(cout / sw) * (cinp / (sw == 32 ? 8 : 16)) * nslot * 256);
        if (dry) return o;
        std::vector<float> tmp((size_t)6 * cout * cinp, 0.0f);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) {
                for (int t = 0; t < 5; ++t) tmp[((size_t)t * cout + co) * cinp + ci] = w[((size_t)co * cin + ci) * 5 + t];
                if (wres) tmp[((size_t)5 * cout + co) * cinp + ci] = wres[(size_t)co * cin + ci];
            }
        if (bf3) pack_fragments_bf3(tmp.data(), cout, cinp, 5, wres != nullptr, reinterpret_cast<unsigned short*>(&host[o]));
        else if (form == F_FRAG_K4) pack_fragments_k4(tmp.data(), cout, cinp, wres != nullptr, &host[o]);
        else if (form == F_FRAG_K2) pack_fragments_k2(tmp.data(), cout, cinp, wres != nullptr, &host[o]);
        else pack_fragments(tmp.data(), cout, cinp, kt0, ntap, wres != nullptr, &host[o], sw);
        return o;
    }
    // strided Conv1d k3 (Cout, Cin, 3) or ConvTranspose1d k4 (Cin, Cout, 4) of a wide level -> fragment stream, slot = tap
    // (form: F_FRAG_BF3 = bf3.hip's bf16-triple stream | F_FRAG with the tile height sw)
    size_t resample_frag(const float* w, int cin, int cout, int k, bool transposed, PackForm form, int sw) {
        const bool bf3 = form == F_FRAG_BF3;
        if (bf3) tag(F_FRAG_BF3);
        tag(F_RESAMPLE), tag(cout), tag(cin), tag(k), tag(transposed ? 1 : 0);
        if (!bf3) tag(sw);
        const size_t o = add(bf3 ? bf3_stream_elems(cout, cin, k) / 2 : (size_t)(cout / sw) * (cin / (sw == 32 ? 8 : 16)) * k * 256);
        if (dry) return o;
        std::vector<float> tmp((size_t)6 * cout * cin, 0.0f);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < k; ++t)
                    tmp[((size_t)t * cout + co) * cin + ci] = transposed ? w[((size_t)ci * cout + co) * k + t] : w[((size_t)co * cin + ci) * k + t];
        if (bf3) pack_fragments_bf3(tmp.data(), cout, cin, k, false, reinterpret_cast<unsigned short*>(&host[o]));
        else pack_fragments(tmp.data(), cout, cin, 0, k, false, &host[o], sw);
        return o;
    }
    size_t vec(const float* v, int n) {
        tag(F_VEC);
        size_t o = add(n);
        if (!dry) memcpy(&host[o], v, sizeof(float) * n);
        return o;
    }
};

struct BufPool {
    std::vector<int> free_ids;
    std::vector<int> pinned;  // never recycled (activation taps kept readable after a forward)
    int n = 0;
    int get() {
        if (!free_ids.empty()) {
            int i = free_ids.back();
            free_ids.pop_back();
            return i;
        }
        return n++;
    }
    void pin(int i) { pinned.push_back(i); }
    void put(int i) {
        for (int q : pinned)
            if (q == i) return;
        for (int q : free_ids)
            if (q == i) return;
        free_ids.push_back(i);
    }
};

// Build-time tensor handle
struct TH {
    int buf;
    int C, L;
};

}  // namespace edmp

using namespace edmp;

extern "C" int64_t edmp_unet_param_count(const edmp_unet_desc* desc) {
    if (!desc || desc->n_levels < 2 || desc->n_levels > EDMP_MAX_LEVELS) return -1;
    return inventory(*desc).total;
}

// Version of the packing code: bump whenever the packing of any kernel family changes.  The layout id of an image is this
// version mixed with the signature of the tensor sequence the builder actually produced (Packer::sig): a stale image, or
// one written under other builder switches, fails to load instead of feeding a kernel the wrong fragment order.
static const int kPackVersion = 301;

// ---- the ARCHITECTURE WALK: the one place that states an op ---------------------------------------------------------------------
// kernel instance an op launches, spelled as rocprofv3's kernel trace prints it (minus the edmp:: prefix): lets
// bench.py's per-kernel table be checked line by line against profiles/*_kernel_stats.csv
static void op_kernel_name(const Op& o, char* out) {
    if (o.kind == OP_RCB || o.kind == OP_WRS) {
        const ConvInst& r = *o.inst;
        snprintf(out, 64, "%s_conv_kernel<%d, %d, %d, %d, %d, %s>", r.bf3 ? "bf3" : "wide", r.kind, r.ms, r.cg, r.gs, r.L, r.res ? "true" : "false");
    } else if (o.kind == OP_LVL && o.lv_pair) {
        const Level2Inst& r = *o.lv_pair;
        snprintf(out, 64, "level2_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d>", r.ma, r.ca, r.la, r.cina, r.mb, r.cb, r.lb, r.cinb, r.sb);
    } else if (o.kind == OP_LVL) {
        const LevelInst& r = *o.lv_inst;
        snprintf(out, 64, "level_kernel<%d, %d, %d, %d, %d>", r.mode, r.C, r.L, r.sb, r.cin);
    } else if (o.kind == OP_CONV) {
        const int kc = pick_kc(o.cv().C1, o.cv().C2);
        if (o.cv().Cout % 64 == 0) snprintf(out, 64, "conv_mfma_kernel<64, 64, %d>", kc);
        else snprintf(out, 64, "conv_mfma_kernel<128, 32, %d>", kc >= 32 ? 32 : kc);
    } else {
        const int n = (o.gn().C / 8) * o.gn().L;
        snprintf(out, 64, "gn_mish_kernel<%d>", n <= 128 ? 2 : n <= 256 ? 4 : 8);
    }
}

// Where the walk's offsets and buffer ids become pointers: an offset into the packed weight image -> wpack + offset, an id of the
// buffer pool -> that activation buffer.  Unbound (the layout-only pass: neither exists yet) both are nullptr.
struct Binder {
    const float* wpack = nullptr;
    const std::vector<float*>* bufs = nullptr;
    const float* w(size_t off) const { return wpack ? wpack + off : nullptr; }
    float* buf(int id) const { return bufs ? (*bufs)[id] : nullptr; }
};

static int down_length(int L) { return (L - 1) / 2 + 1; }  // Conv1d k3 s2 p1
static int up_length(int L) {                             // ConvTranspose1d k4 s2 p1, then the crop rule of temporalunet.py:70-71
    const int Lout = 2 * L;
    return (Lout == 8 || Lout == 14 || Lout == 26) ? Lout - 1 : Lout;
}

// Walks the architecture (temporalunet.py:47-76) once: decides per layer which kernel family runs it, packs its weights into the
// device image in that family's layout (or only sizes them: Packer::dry), assigns activation buffers from a recycling pool and
// emits the layer program, FLOP counts and kernel names included.  No device work.  A model build runs it twice (unet_build).
struct Walk {
    const edmp_unet_desc* desc;
    const float* params;   // state-dict blob (never read through when pk.dry)
    RawNet inv;
    const BuildSwitches sw;
    const Binder bind;
    int N, td, nd, CP0 = 8;  // horizon, time_dim, levels, padded input channels
    std::vector<int> dm;     // input_dim, dims...
    // products
    Packer pk;
    BufPool pool;
    std::vector<Op> ops;
    std::vector<UNet::Tap> taps;
    std::vector<float> tw_all, tb_all;  // concatenated time-MLP weights of the residual blocks
    int tb_cursor = 0, rcb_idx = 0;
    int x_in_buf = -1, head_buf = -1;
    size_t max_lc;  // floats per sample of the largest activation
    size_t hw = 0, hb = 0, o_t1w = 0, o_t1b = 0, o_t3w = 0, o_t3b = 0, o_tw = 0, o_tb = 0;
    double head_flops = 0;
    // what the walk refuses once it is through (the first of each kind)
    bool identity_over_concat = false;
    int no_twin_cout = 0, no_twin_L = 0, gn_group = 0;

    // layout_only: offsets and sizes, `blob` is not looked at (the first pass of a build; both passes of loading a packed image)
    Walk(const edmp_unet_desc* d, const float* blob, bool layout_only, const BuildSwitches& s, const Binder& b) : desc(d), inv(inventory(*d)), sw(s), bind(b) {
        static const float no_params = 0.0f;  // offsets are computed from `params` but never read through
        params = layout_only ? &no_params : blob;
        N = d->horizon, td = d->time_dim, nd = d->n_levels;
        dm.push_back(d->input_dim);
        for (int i = 0; i < d->n_levels; ++i) dm.push_back(d->dims[i]);
        pk.dry = layout_only;
        max_lc = (size_t)N * CP0;
    }

    void append(std::vector<float>& v, const float* src, size_t n) {  // layout-only pass: sizes, no reads
        if (pk.dry) v.resize(v.size() + n, 0.0f);
        else v.insert(v.end(), src, src + n);
    }
    int time_bias(const RawRCB& r) {  // the block's columns of the time-bias table; returns their offset in a row
        const int off = tb_cursor;
        tb_cursor += r.cout;
        append(tw_all, params + r.tw.off, (size_t)r.cout * td);
        append(tb_all, params + r.tb.off, r.cout);
        return off;
    }
    const float* vec(const RawT& t, int n) { return bind.w(pk.vec(params + t.off, n)); }
    TH new_out(int C, int Lin, int Lout) {  // an op's output buffer
        max_lc = std::max(max_lc, (size_t)std::max(Lin, Lout) * C);
        return TH{pool.get(), C, Lout};
    }
    void tap(int which, TH x) {  // kept readable after a forward
        taps.push_back({which, bind.buf(x.buf), x.C, x.L});
        pool.pin(x.buf);
    }
    template <class P>
    void set_src(P& p, TH a, const TH* a2) {
        p.src1 = bind.buf(a.buf);
        p.src2 = a2 ? bind.buf(a2->buf) : nullptr;
        p.C1 = a.C;
        p.C2 = a2 ? a2->C : 0;
    }
    Op& push(Op o) {
        if (o.flops_direct == 0) o.flops_direct = o.flops_exec;
        if (o.inst && o.inst->bf3) o.flops_bf16 = 6.0 * o.flops_direct;  // six exact partial products per fp32 product, issued on the bf16 pipe
        if (!(o.kind == OP_RCB && !o.inst)) op_kernel_name(o, o.name);    // (a Conv1dBlock without its instance: refused below)
        ops.push_back(o);
        return ops.back();
    }

    static long valid_pairs(int Lin, int Lout, int k, int stride, int pad, bool tr) {
        long cnt = 0;
        for (int lo = 0; lo < Lout; ++lo)
            for (int t = 0; t < k; ++t) {
                if (!tr) {
                    int li = lo * stride + t - pad;
                    if (li >= 0 && li < Lin) ++cnt;
                } else {
                    int num = lo + pad - t;
                    if (num >= 0 && num % stride == 0 && num / stride < Lin) ++cnt;
                }
            }
        return cnt;
    }
    // nominal FLOPs: what torch executes: conv 2*Lout*Cout*Cin*k ; convT 2*Lin*Cin*Cout*k (uncropped).  Issued: the taps that meet data, stored channels
    static void conv_flops(Op& o, int Lin, int Lout, int cin_true, int cin_store, int Cout, int k, int stride, int pad, bool tr) {
        o.flops_nominal = tr ? 2.0 * Lin * cin_true * Cout * k : 2.0 * Lout * Cout * (double)cin_true * k;
        o.flops_exec = 2.0 * (double)valid_pairs(Lin, Lout, k, stride, pad, tr) * Cout * (double)cin_store;
    }
    TH emit_conv(TH a, const TH* a2, int cin_true, size_t w, size_t b, int Cout, int k, int stride, int pad, bool tr, int Lout) {
        ConvP c{};
        set_src(c, a, a2);
        c.Lin = a.L, c.Lout = Lout, c.ntaps = k, c.stride = stride, c.pad = pad, c.transposed = tr;
        c.W = bind.w(w), c.bias = bind.w(b), c.Cout = Cout;
        const TH out = new_out(Cout, a.L, Lout);
        c.dst = bind.buf(out.buf);
        Op o{OP_CONV, c};
        conv_flops(o, a.L, Lout, cin_true, c.C1 + c.C2, Cout, k, stride, pad, tr);
        push(o);
        return out;
    }
    TH emit_wrs(TH a, size_t w, size_t b, int Cout, const ConvInst* inst, int k, int Lout) {
        RcbP c{};
        set_src(c, a, nullptr);
        c.W = bind.w(w), c.bias = bind.w(b), c.Cout = Cout;
        const TH out = new_out(Cout, a.L, Lout);
        c.dst = bind.buf(out.buf);
        Op o{OP_WRS, c};
        o.inst = inst;
        conv_flops(o, a.L, Lout, a.C, a.C, Cout, k, 2, 1, inst->kind == WK_UP);
        push(o);
        return out;
    }
    void emit_gn(TH y, const float* gamma, const float* beta, const float* res, int tb_off) {
        GnP g{};
        g.y = bind.buf(y.buf), g.gamma = gamma, g.beta = beta, g.add_res = res, g.L = y.L, g.C = y.C;
        // the generic GroupNorm keeps a group in registers (gn_mish_kernel, at most 8 x 64 elements)
        if (!gn_group && (y.C / 8) * y.L > 512) gn_group = (y.C / 8) * y.L;
        Op o{OP_GN, g};
        o.tb1 = tb_off;
        push(o);
    }
    // the resampler of a wide level: its fragment-stream instance if a row exists, else the generic conv
    TH emit_resampler(int kind, TH a, const RawT& w, const RawT& b, int Lout) {
        const bool up = kind == WK_UP;
        const int C = a.C, k = up ? 4 : 3;
        if (const ConvChoice ch = choose_conv(sw, kind, C, a.L, C, 0); ch.row[0]) {
            const size_t wo = pk.resample_frag(params + w.off, C, C, k, up, ch.stream, ch.row[0]->ms), bo = pk.vec(params + b.off, C);
            return emit_wrs(a, wo, bo, C, ch.row[0], k, Lout);
        }
        const size_t wo = up ? pk.convT(params + w.off, C, C, k) : pk.conv(params + w.off, C, C, k, C), bo = pk.vec(params + b.off, C);
        return emit_conv(a, nullptr, C, wo, bo, C, k, 2, 1, up, Lout);
    }
    // a block's residual 1x1 conv as its own launch (no instance folds it in, or EDMP_NO_RESFOLD)
    TH emit_res_conv(const RawRCB& r, TH x, const TH* x2) {
        const size_t wr = pk.conv(params + r.rw.off, r.cout, r.cin, 1, x.C + (x2 ? x2->C : 0)), br = pk.vec(params + r.rb.off, r.cout);
        return emit_conv(x, x2, r.cin, wr, br, r.cout, 1, 1, 0, false, x.L);
    }
    struct BlockW { const float *w, *b, *gamma, *beta; };  // a packed Conv1dBlock
    // Conv1dBlock on the position-tile kernel.  res: the residual conv2 adds | tbo: the time bias conv1 adds | fold: the block's
    // residual 1x1 conv rides in this launch (its weights sit behind the taps in w); *fold receives its output
    TH emit_fused(TH a, const TH* a2, int cin_true, int cout, const ConvChoice& ch, const BlockW& w, const float* res, int tbo, const RawT* fold_bias, TH* fold) {
        RcbP c{};
        set_src(c, a, a2);
        c.W = w.w, c.bias = w.b, c.gamma = w.gamma, c.beta = w.beta, c.add_res = res, c.Cout = cout;
        const TH out = new_out(cout, a.L, a.L);
        c.dst = bind.buf(out.buf);
        const int cin_store = c.C1 + c.C2;
        Op o{OP_RCB};
        o.tb1 = tbo;
        o.inst = ch.row[fold ? 1 : 0];
        if (!o.inst && !no_twin_cout) no_twin_cout = cout, no_twin_L = a.L;  // listed without the twin that folds the residual in
        conv_flops(o, a.L, a.L, cin_true, cin_store, cout, 5, 1, 2, false);
        o.flops_direct = o.flops_exec;
        // issued MFMA work: the L = 2 Karatsuba form runs 3 matrix products where the direct form runs 4, the nested L = 4 form 9 for 14
        if (ch.form) o.flops_exec = 2.0 * (ch.form == 2 ? 3.0 : 9.0) * cout * (double)cin_store;
        if (fold) {
            *fold = TH{pool.get(), cout, a.L};
            c.res_out = bind.buf(fold->buf);
            c.res_bias = vec(*fold_bias, cout);
            o.flops_nominal += 2.0 * a.L * cout * (double)cin_true;
            o.flops_exec += 2.0 * a.L * cout * (double)cin_store;
            o.flops_direct += 2.0 * a.L * cout * (double)cin_store;
        }
        o.p = c;
        push(o);
        return out;
    }
    TH emit_rcb(TH x, const TH* x2) {
        const RawRCB& r = inv.rcbs[rcb_idx++];
        const int cin_store = x.C + (x2 ? x2->C : 0);
        // conv1 (a residual 1x1 conv folded into the wide fused kernel is packed right behind it, as tap index 5)
        const ConvChoice ch1 = choose_conv(sw, WK_K5, r.cout, x.L, x.C, x2 ? x2->C : 0), ch2 = choose_conv(sw, WK_K5, r.cout, x.L, r.cout, 0);
        const bool wide = ch1.row[0] && ch2.row[0];  // (same shape: both or neither)
        const bool fold_res = wide && r.has_res && sw.resfold;
        // the position-tile kernel reads its weights as an MFMA fragment stream (wide.hip); the generic conv as [tap][Cout][Cin]
        const size_t w1 = wide ? pk.conv_frag(params + r.cb[0].w.off, fold_res ? params + r.rw.off : nullptr, r.cout, r.cin, cin_store, x.L, ch1.stream, ch1.row[0]->ms)
                               : pk.conv(params + r.cb[0].w.off, r.cout, r.cin, 5, cin_store);
        const size_t b1 = pk.vec(params + r.cb[0].b.off, r.cout);
        const BlockW k1{bind.w(w1), bind.w(b1), vec(r.cb[0].gw, r.cout), vec(r.cb[0].gb, r.cout)};
        const size_t w2 = wide ? pk.conv_frag(params + r.cb[1].w.off, nullptr, r.cout, r.cout, r.cout, x.L, ch2.stream, ch2.row[0]->ms) : pk.conv(params + r.cb[1].w.off, r.cout, r.cout, 5, r.cout);
        const size_t b2 = pk.vec(params + r.cb[1].b.off, r.cout);
        const BlockW k2{bind.w(w2), bind.w(b2), vec(r.cb[1].gw, r.cout), vec(r.cb[1].gb, r.cout)};
        const int tb_off = time_bias(r);
        if (!r.has_res && x2) identity_over_concat = true;  // identity residual (blocks.py:151-152) over a channel concat
        TH rr{-1, r.cout, x.L};                             // the residual 1x1 conv's output, where the block has one
        if (wide) {
            const TH h = emit_fused(x, x2, r.cin, r.cout, ch1, k1, nullptr, tb_off, &r.rb, fold_res ? &rr : nullptr);
            if (r.has_res && !fold_res) rr = emit_res_conv(r, x, x2);
            const TH out = emit_fused(h, nullptr, r.cout, r.cout, ch2, k2, bind.buf(r.has_res ? rr.buf : x.buf), -1, nullptr, nullptr);
            pool.put(h.buf);
            if (rr.buf >= 0) pool.put(rr.buf);
            return out;
        }
        const TH y1 = emit_conv(x, x2, r.cin, w1, b1, r.cout, 5, 1, 2, false, x.L);
        emit_gn(y1, k1.gamma, k1.beta, nullptr, tb_off);
        const TH y2 = emit_conv(y1, nullptr, r.cout, w2, b2, r.cout, 5, 1, 2, false, x.L);
        pool.put(y1.buf);
        if (r.has_res) rr = emit_res_conv(r, x, x2);
        emit_gn(y2, k2.gamma, k2.beta, bind.buf(r.has_res ? rr.buf : x.buf), -1);
        if (rr.buf >= 0) pool.put(rr.buf);
        return y2;
    }

    // a whole level in one launch (level.hip): RCB, RCB, resampling conv (+ the final Conv1dBlock); consumes two entries
    // of inv.rcbs like two emit_rcb calls would, in the same order (so the time-bias row keeps its layout)
    TH emit_level(const LevelInst* lv, TH xin, const TH* x2, const RawT& rs_w, const RawT& rs_b, bool want_skip, TH* skip_th) {
        const RawRCB& r1 = inv.rcbs[rcb_idx++];
        const RawRCB& r2 = inv.rcbs[rcb_idx++];
        const int mode = lv->mode, Cc = r1.cout, Ll = xin.L, KX = std::max(lv->cin, 16);  // the first conv's K: stored input channels, padded to a whole K group
        const bool fin = mode == LV_UP_FINAL;
        const int cin_store = xin.C + (x2 ? x2->C : 0);
        // the level kernels read plain fragment streams with 16-sample tiles
        auto frag = [&](const RawT& w, const RawT* wres, int cin, int K, int L) {
            return bind.w(pk.conv_frag(params + w.off, wres ? params + wres->off : nullptr, Cc, cin, K, L, F_FRAG, 16));
        };
        auto v = [&](const RawT& t) { return vec(t, Cc); };
        LevelP c{};
        set_src(c, xin, x2);
        // the image holds the level's tensors in THIS order (statements run top to bottom; the packer appends)
        c.w11 = frag(r1.cb[0].w, &r1.rw, r1.cin, KX, Ll);
        c.w12 = frag(r1.cb[1].w, nullptr, Cc, Cc, Ll);
        c.w21 = frag(r2.cb[0].w, nullptr, Cc, Cc, Ll);
        c.w22 = frag(r2.cb[1].w, nullptr, Cc, Cc, Ll);
        c.wrs = bind.w(pk.resample_frag(params + rs_w.off, Cc, Cc, mode == LV_DOWN ? 3 : 4, mode != LV_DOWN, F_FRAG, 16));
        const float* none = bind.w(0);  // what the final block's arguments hold in the modes that have none: the image's base, never read
        c.wfin = fin ? frag(inv.final_cb.w, nullptr, Cc, Cc, 50) : none;
        c.b11 = v(r1.cb[0].b), c.g11 = v(r1.cb[0].gw), c.be11 = v(r1.cb[0].gb);
        c.rb1 = v(r1.rb);
        c.b12 = v(r1.cb[1].b), c.g12 = v(r1.cb[1].gw), c.be12 = v(r1.cb[1].gb);
        c.b21 = v(r2.cb[0].b), c.g21 = v(r2.cb[0].gw), c.be21 = v(r2.cb[0].gb);
        c.b22 = v(r2.cb[1].b), c.g22 = v(r2.cb[1].gw), c.be22 = v(r2.cb[1].gb);
        c.brs = v(rs_b);
        c.bfin = fin ? v(inv.final_cb.b) : none, c.gfin = fin ? v(inv.final_cb.gw) : none, c.befin = fin ? v(inv.final_cb.gb) : none;
        Op o{OP_LVL};
        o.lv_inst = lv;
        o.tb1 = time_bias(r1), o.tb2 = time_bias(r2);  // time-bias table columns, block order
        if (want_skip) {
            *skip_th = TH{pool.get(), Cc, Ll};
            c.skip_out = bind.buf(skip_th->buf);
        }
        const int Lout = mode == LV_DOWN ? down_length(Ll) : up_length(Ll);
        const TH out = new_out(Cc, Ll, Lout);
        c.out = bind.buf(out.buf);
        const double vp = (double)valid_pairs(Ll, Ll, 5, 1, 2, false);
        const int k = mode == LV_DOWN ? 3 : 4;
        o.flops_nominal = 2.0 * Ll * Cc * 5.0 * ((double)r1.cin + 3.0 * Cc) + 2.0 * Ll * Cc * (double)r1.cin +
                          (mode == LV_DOWN ? 2.0 * Lout * Cc * (double)Cc * k : 2.0 * Ll * (double)Cc * Cc * k) + (fin ? 2.0 * Lout * Cc * (double)Cc * 5 : 0.0);
        o.flops_exec = 2.0 * vp * Cc * ((double)cin_store + 3.0 * Cc) + 2.0 * Ll * Cc * (double)cin_store +
                       2.0 * (double)valid_pairs(Ll, Lout, k, 2, 1, mode != LV_DOWN) * Cc * (double)Cc +
                       (fin ? 2.0 * (double)valid_pairs(Lout, Lout, 5, 1, 2, false) * Cc * (double)Cc : 0.0);
        o.p = c;
        push(o);
        return out;
    }
    // this level and the one behind it as one launch (level2_kernel): the first one's output only ever exists in LDS - no tap
    void pair_or_tap(const LevelInst* lv, const LevelInst* next, int which, TH x) {
        if (const Level2Inst* pair = choose_pair(sw, lv, next)) {
            ops.back().lv_pair = pair;
            op_kernel_name(ops.back(), ops.back().name);
        } else {
            tap(which, x);
        }
    }

    // the walk itself: down path, middle, up path, final block + head, time-embedding tensors
    int walk() {
        TH x{pool.get(), CP0, N};
        x_in_buf = x.buf;
        pool.pin(x_in_buf);  // written by the sampler kernels between forwards: never recycled as an activation
        std::vector<TH> skips;
        bool final_fused = false;
        for (int i = 0; i < nd; ++i) {
            if (const LevelInst* lv = (i != nd - 1) ? choose_level(sw, LV_DOWN, dm[i + 1], x.L, x.C, 0) : nullptr) {
                // the skip of level 0 is never consumed (5 up-samplers for 6 skips, temporalunet.py:31-32,66-67): not even written
                TH sk{-1, dm[i + 1], x.L};
                TH xo = emit_level(lv, x, nullptr, inv.down_w[i], inv.down_b[i], i > 0, &sk);
                pool.put(x.buf);
                skips.push_back(sk);
                x = xo;
                pair_or_tap(lv, i + 1 < nd - 1 ? choose_level(sw, LV_DOWN, dm[i + 2], x.L, x.C, 0) : nullptr, i, x);
                continue;
            }
            TH a = emit_rcb(x, nullptr);
            pool.put(x.buf);  // the block input is dead once both consumers (conv1, residual) are emitted
            TH b = emit_rcb(a, nullptr);
            pool.put(a.buf);
            skips.push_back(b);
            x = (i != nd - 1) ? emit_resampler(WK_DOWN, b, inv.down_w[i], inv.down_b[i], down_length(b.L)) : b;
            tap(i, x);
        }
        {
            // middle: input is skips.back() (same buffer, must stay alive for the up path)
            TH a = emit_rcb(x, nullptr);
            TH b = emit_rcb(a, nullptr);
            pool.put(a.buf);
            x = b;
            tap(100, x);
        }
        for (int j = 0, i = nd; i > 1; --i, ++j) {
            TH sk = skips.back();
            skips.pop_back();
            EDMP_REQUIRE(sk.L == x.L && sk.C == x.C, "skip/upsample shape mismatch at up level %d (L %d vs %d)", j, sk.L, x.L);
            EDMP_REQUIRE(sk.buf >= 0, "up level %d consumes a skip tensor that the fused down level did not write", j);
            const int mode = (i == 2 && dm[1] == dm[i - 1] && 2 * x.L == N) ? LV_UP_FINAL : LV_UP;
            if (const LevelInst* lv = choose_level(sw, mode, dm[i - 1], x.L, x.C, sk.C)) {
                TH xo = emit_level(lv, x, &sk, inv.up_w[j], inv.up_b[j], false, nullptr);
                pool.put(x.buf);
                pool.put(sk.buf);
                x = xo;
                if (mode == LV_UP_FINAL) {
                    final_fused = true;  // the level kernel already applied final_conv.0
                } else {
                    const bool next_is_final = i == 3 && !skips.empty() && dm[1] == dm[i - 2] && 2 * x.L == N;
                    pair_or_tap(lv, next_is_final ? choose_level(sw, LV_UP_FINAL, dm[i - 2], x.L, x.C, skips.back().C) : nullptr, 200 + j, x);
                }
                continue;
            }
            TH a = emit_rcb(x, &sk);
            pool.put(x.buf);
            pool.put(sk.buf);
            TH b = emit_rcb(a, nullptr);
            pool.put(a.buf);
            x = emit_resampler(WK_UP, b, inv.up_w[j], inv.up_b[j], up_length(b.L));
            pool.put(b.buf);
            tap(200 + j, x);
        }
        EDMP_REQUIRE(x.L == N, "decoder output length %d != horizon %d", x.L, N);
        // final Conv1dBlock + 1x1 head
        if (!final_fused) {
            const size_t w = pk.conv(params + inv.final_cb.w.off, dm[1], dm[1], 5, dm[1]), b = pk.vec(params + inv.final_cb.b.off, dm[1]);
            const float *g = vec(inv.final_cb.gw, dm[1]), *be = vec(inv.final_cb.gb, dm[1]);
            TH y = emit_conv(x, nullptr, dm[1], w, b, dm[1], 5, 1, 2, false, N);
            emit_gn(y, g, be, nullptr, -1);
            pool.put(x.buf);
            x = y;
        }
        hw = pk.vec(params + inv.final_w.off, desc->input_dim * dm[1]);
        hb = pk.vec(params + inv.final_b.off, desc->input_dim);
        head_flops = 2.0 * N * desc->input_dim * dm[1];

        // raw time-embedding weights for the table kernel
        o_t1w = pk.vec(params + inv.t1w.off, 4 * td * td), o_t1b = pk.vec(params + inv.t1b.off, 4 * td);
        o_t3w = pk.vec(params + inv.t3w.off, 4 * td * td), o_t3b = pk.vec(params + inv.t3b.off, td);
        o_tw = pk.vec(tw_all.data(), (int)tw_all.size()), o_tb = pk.vec(tb_all.data(), (int)tb_all.size());
        head_buf = x.buf;
        EDMP_REQUIRE(!identity_over_concat, "identity residual over a channel concat is not supported");
        EDMP_REQUIRE(!no_twin_cout, "no fused conv+GroupNorm kernel for Cout=%d L=%d", no_twin_cout, no_twin_L);
        // refuse the architecture here, at load, rather than in the middle of its first forward (launch_gn keeps the same check)
        EDMP_REQUIRE(!gn_group, "GroupNorm group of %d elements exceeds the register-resident limit (512)", gn_group);
        // a merged pair is ONE launch, attributed to its first op: that op carries the pair's FLOPs (the model totals are unaffected)
        for (size_t i = 0; i < ops.size(); ++i)
            if (second_of_pair(ops, i)) {
                Op &a = ops[i - 1], &b = ops[i];
                a.flops_nominal += b.flops_nominal, a.flops_exec += b.flops_exec, a.flops_direct += b.flops_direct;
                b.flops_nominal = b.flops_exec = b.flops_direct = 0.0;
            }
        return EDMP_OK;
    }
};

static int check_desc(const edmp_unet_desc* desc) {
    EDMP_REQUIRE(desc->n_levels >= 2 && desc->n_levels <= EDMP_MAX_LEVELS, "n_levels out of range");
    EDMP_REQUIRE(desc->input_dim >= 1 && desc->input_dim <= 8, "input_dim must be in 1..8");
    EDMP_REQUIRE(desc->time_dim >= 4 && desc->time_dim % 2 == 0, "time_dim must be even");
    for (int i = 0; i < desc->n_levels; ++i) EDMP_REQUIRE(desc->dims[i] % 8 == 0 && desc->dims[i] >= 8, "dims must be multiples of 8");
    return EDMP_OK;
}

// builds the layer program + device weight image.  packed == nullptr: repack `params` (state-dict order) on the host;
// otherwise `packed` IS the device image (edmp_unet_read_packed of the same architecture): only the layout is computed.
// The walk runs twice under one BuildSwitches value: pass 1 layout-only and unbound (what to allocate, every refusal), pass 2 bound to
// the image and the buffers that then exist (the program, the taps; it packs unless `packed` is given).
static int unet_build(edmp_ctx* ctx, const edmp_unet_desc* desc, const float* params, int64_t n_params, int max_batch, const float* packed,
                      int64_t n_packed, int packed_layout) {
    ctx->epoch++;
    if (int rc = check_desc(desc)) return rc;
    EDMP_REQUIRE(max_batch >= 1, "max_batch must be positive");
    const BuildSwitches sw = BuildSwitches::read();
    // ---- pass 1: the layout
    Walk lay(desc, nullptr, true, sw, Binder{});
    EDMP_REQUIRE(packed || lay.inv.total == n_params, "parameter blob has %lld floats, architecture needs %lld", (long long)n_params, (long long)lay.inv.total);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    if (ctx->unet) {
        unet_destroy(ctx->unet);
        ctx->unet = nullptr;
    }
    // owned here until the build has succeeded: every early return below (argument checks, failed allocations / copies /
    // launches) releases the weight image and the activation buffers
    std::unique_ptr<UNet, void (*)(UNet*)> guard(new UNet(), unet_destroy);
    UNet* u = guard.get();
    u->desc = *desc;
    u->max_batch = max_batch;
    if (int rc = lay.walk()) return rc;
    u->tb_stride = lay.tb_cursor;
    u->buf_cap = lay.max_lc * (size_t)max_batch;
    u->layout = lay.pk.layout_id(kPackVersion);
    u->wpack_floats = lay.pk.total;
    if (packed && packed_layout != u->layout) {
        set_error("packed weight image has layout id %d, this library with the current builder switches packs %d: re-pack from the state dict", packed_layout, u->layout);
        return EDMP_ERR_LAYOUT;
    }
    if (packed && (int64_t)u->wpack_floats != n_packed) {
        set_error("packed weight image has %lld floats, this architecture / library layout needs %zu", (long long)n_packed, u->wpack_floats);
        return EDMP_ERR_LAYOUT;
    }
    // ---- device image, activation buffers, time-bias table
    if (hipMalloc((void**)&u->wpack, u->wpack_floats * sizeof(float)) != hipSuccess) {
        set_error("hipMalloc of %zu weight bytes failed", u->wpack_floats * sizeof(float));
        return EDMP_ERR_HIP;
    }
    for (int i = 0; i < lay.pool.n; ++i) {
        float* p = nullptr;
        if (hipMalloc((void**)&p, u->buf_cap * sizeof(float)) != hipSuccess) {
            set_error("hipMalloc of activation buffer %d (%zu bytes) failed", i, u->buf_cap * sizeof(float));
            return EDMP_ERR_HIP;
        }
        u->bufs.push_back(p);
    }
    EDMP_HIP_CHECK(hipMalloc((void**)&u->tbias, (size_t)desc->T * u->tb_stride * sizeof(float)));
    // ---- pass 2: the same walk, bound
    Walk pl(desc, params, packed != nullptr, sw, Binder{u->wpack, &u->bufs});
    if (int rc = pl.walk()) return rc;
    EDMP_REQUIRE(pl.pk.layout_id(kPackVersion) == u->layout && pl.pk.total == u->wpack_floats && pl.pool.n == lay.pool.n,
                 "the two passes of the model build disagree: layout id %d / %d, %zu / %zu floats", u->layout, pl.pk.layout_id(kPackVersion), u->wpack_floats, pl.pk.total);
    EDMP_HIP_CHECK(hipMemcpy(u->wpack, packed ? packed : pl.pk.host.data(), u->wpack_floats * sizeof(float), hipMemcpyHostToDevice));
    {
        size_t sm = (size_t)(6 * pl.td) * sizeof(float);
        hipLaunchKernelGGL(time_table_kernel, dim3(desc->T), dim3(256), sm, ctx->stream, u->wpack + pl.o_t1w, u->wpack + pl.o_t1b,
                           u->wpack + pl.o_t3w, u->wpack + pl.o_t3b, u->wpack + pl.o_tw, u->wpack + pl.o_tb, u->tbias, pl.td, u->tb_stride);
        EDMP_HIP_CHECK(hipGetLastError());
        EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    u->prog = std::move(pl.ops);
    u->taps = std::move(pl.taps);
    for (const Op& op : u->prog) {
        u->flops_nominal += op.flops_nominal;  // (zero for an OP_GN)
        u->flops_exec += op.flops_exec;
        u->flops_direct += op.flops_direct;
        u->flops_bf16 += op.flops_bf16;
        if (op.inst && op.inst->bf3) u->flops_f32_moved += op.flops_exec;
    }
    if (int rc = check_bf3_cu_claim(u)) return rc;
    u->flops_nominal += pl.head_flops;
    u->flops_exec += pl.head_flops;
    u->flops_direct += pl.head_flops;
    u->x_in = u->bufs[pl.x_in_buf];
    u->h_last = u->bufs[pl.head_buf];
    u->head_w = u->wpack + pl.hw;
    u->head_b = u->wpack + pl.hb;
    u->head_cin = pl.dm[1];
    ctx->unet = guard.release();
    return EDMP_OK;
}

extern "C" int edmp_unet_load(edmp_ctx* ctx, const edmp_unet_desc* desc, const float* params, int64_t n_params, int max_batch) {
    EDMP_REQUIRE(ctx && desc && params, "edmp_unet_load: null argument");
    return unet_build(ctx, desc, params, n_params, max_batch, nullptr, 0, 0);
}

extern "C" int edmp_unet_load_packed(edmp_ctx* ctx, const edmp_unet_desc* desc, const float* packed, int64_t n_packed, int layout, int max_batch) {
    EDMP_REQUIRE(ctx && desc && packed, "edmp_unet_load_packed: null argument");
    return unet_build(ctx, desc, nullptr, 0, max_batch, packed, n_packed, layout);
}

// host-only: pass 1 of a model build alone (the layout-only, unbound walk) under the current builder switches, no device work
extern "C" int edmp_unet_plan_describe(const edmp_unet_desc* desc, int cap, int* n_ops, char* names, int* layout, int64_t* n_packed) {
    EDMP_REQUIRE(desc && n_ops, "edmp_unet_plan_describe: null argument");
    if (int rc = check_desc(desc)) return rc;
    Walk pl(desc, nullptr, true, BuildSwitches::read(), Binder{});
    if (int rc = pl.walk()) return rc;
    const int n = (int)pl.ops.size();
    *n_ops = n;
    for (int i = 0; names && i < n && i < cap; ++i) memcpy(names + (size_t)i * 64, pl.ops[i].name, 64);
    if (layout) *layout = pl.pk.layout_id(kPackVersion);
    if (n_packed) *n_packed = (int64_t)pl.pk.total;
    return EDMP_OK;
}

extern "C" int64_t edmp_unet_packed_size(edmp_ctx* ctx, int* layout) {
    if (layout) *layout = (ctx && ctx->unet) ? ctx->unet->layout : 0;
    return (ctx && ctx->unet) ? (int64_t)ctx->unet->wpack_floats : -1;
}

extern "C" int edmp_unet_read_packed(edmp_ctx* ctx, float* out_host, int64_t capacity) {
    EDMP_REQUIRE(ctx && ctx->unet && out_host, "edmp_unet_read_packed: null argument / no model");
    EDMP_REQUIRE(capacity >= (int64_t)ctx->unet->wpack_floats, "buffer of %lld floats, image has %zu", (long long)capacity, ctx->unet->wpack_floats);
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    EDMP_HIP_CHECK(hipMemcpy(out_host, ctx->unet->wpack, ctx->unet->wpack_floats * sizeof(float), hipMemcpyDeviceToHost));
    return EDMP_OK;
}

namespace edmp {
// an event pair for a bracket: a recycled one of Prof::pool, or a new one
static int prof_events(Prof& pf, Prof::Pend& e) {
    if (!pf.pool.empty()) {
        e.a = pf.pool.back().first;
        e.b = pf.pool.back().second;
        pf.pool.pop_back();
        return EDMP_OK;
    }
    EDMP_HIP_CHECK(hipEventCreate(&e.a));
    EDMP_HIP_CHECK(hipEventCreate(&e.b));
    return EDMP_OK;
}
// shared with sampler.hip: run the forward on the context's stream
// run the layer program on u->x_in ([B][N][8], already filled); leaves the head input in u->h_last
// `tail` (device-resident loop): if the program ends with the fused final level (LV_UP_FINAL, 32 channels into the head) the
// tail of the reverse step runs inside that launch and *tail_done is set; otherwise the caller launches head_psample_kernel
int unet_run_program(edmp_ctx* ctx, int B, int t, const TailP* tail, bool* tail_done) {
    if (tail_done) *tail_done = false;
    UNet* u = ctx->unet;
    EDMP_REQUIRE(u, "edmp_unet_load has not been called");
    EDMP_REQUIRE(B >= 1 && B <= u->max_batch, "batch %d outside 1..max_batch=%d", B, u->max_batch);
    hipStream_t main_stream = ctx->stream;
    EDMP_REQUIRE(t >= 1 && t <= u->desc.T, "t=%d outside 1..T=%d", t, u->desc.T);
    const float* trow = u->tbias + (size_t)(t - 1) * u->tb_stride;
    Prof& pf = ctx->prof;
    Prof::Pend whole{nullptr, nullptr, -1};
    if (pf.on == 2) {  // one bracket around the whole program: the conv family's time with no per-launch event overhead
        if (int rc = prof_events(pf, whole)) return rc;
        EDMP_HIP_CHECK(hipEventRecord(whole.a, main_stream));
    }
    const std::vector<Op>& prog = u->prog;
    // a level's launch parameters at this batch and step
    auto level_params = [&](const Op& o) {
        LevelP p = o.lv();
        p.B = B;
        p.tail.rps = tail ? tail->rps : 0;  // a scene batch: the workgroups are dealt scene by scene (level.hip)
        p.tb1 = trow + o.tb1, p.tb2 = trow + o.tb2;
        return p;
    };
    // the tail of the reverse step runs inside the last level's launch when that level is the program's last op (LV_UP_FINAL, 32 channels)
    auto fuse_step_tail = [&](LevelP& p, const Op& o, size_t index) {
        if (tail && tail_done && o.lv_inst->mode == LV_UP_FINAL && index + 1 == prog.size() && u->head_cin == 32 && tail->N == u->desc.horizon && tail->C <= 8 && p.out == u->h_last) {
            p.tail = *tail;
            p.tail.on = 1;
            p.tail.w = u->head_w;
            p.tail.bias = u->head_b;
            *tail_done = true;
        }
    };
    for (size_t i = 0; i < prog.size(); ++i) {
        const Op& op = prog[i];
        if (second_of_pair(prog, i)) continue;  // ran inside the previous launch
        hipStream_t s = main_stream;
        Prof::Pend ev{nullptr, nullptr, (int)i};
        const bool timed = pf.on == 1 && own_launch(prog, i);
        if (timed) {
            if (int rc = prof_events(pf, ev)) return rc;
            EDMP_HIP_CHECK(hipEventRecord(ev.a, s));
        }
        int rc = EDMP_OK;
        if (op.kind == OP_RCB) {
            RcbP p = op.rc();
            p.B = B;
            p.add_tb = op.tb1 >= 0 ? trow + op.tb1 : nullptr;
            EDMP_REQUIRE(!(p.add_tb && p.add_res), "fused conv block: a launch adds the time bias (conv1) or the residual (conv2), not both");
            rc = op.inst->launch(p, s, nullptr);
        } else if (op.kind == OP_LVL && op.lv_pair) {
            const Op& nx = prog[i + 1];
            LevelP pa = level_params(op), pb = level_params(nx);
            pa.out = nullptr, pb.src1 = nullptr;  // (level B's first input half arrives in LDS)
            fuse_step_tail(pb, nx, i + 1);
            rc = op.lv_pair->launch(pa, pb, s);
        } else if (op.kind == OP_LVL) {
            LevelP p = level_params(op);
            fuse_step_tail(p, op, i);
            rc = op.lv_inst->launch(p, s);
        } else if (op.kind == OP_WRS) {
            RcbP p = op.rc();
            p.B = B;
            rc = op.inst->launch(p, s, nullptr);
        } else if (op.kind == OP_CONV) {
            ConvP p = op.cv();
            p.B = B;
            launch_conv(p, s);
        } else {
            GnP g = op.gn();
            g.B = B;
            g.add_tbias = op.tb1 >= 0 ? trow + op.tb1 : nullptr;
            rc = launch_gn(g, s);
        }
        if (rc) return rc;
        if (timed) {
            EDMP_HIP_CHECK(hipEventRecord(ev.b, s));
            pf.pending.push_back(ev);
        }
    }
    if (pf.on == 2) {
        EDMP_HIP_CHECK(hipEventRecord(whole.b, main_stream));
        pf.pending.push_back(whole);
    }
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}

int prof_fold(edmp_ctx* ctx) {
    Prof& p = ctx->prof;
    const size_t nops = ctx->unet ? ctx->unet->prog.size() : 0;
    if (p.op_ms.size() != nops) {
        p.op_ms.assign(nops, 0.0);
        p.op_calls.assign(nops, 0);
    }
    for (auto& e : p.pending) {
        float ms = 0.f;
        EDMP_HIP_CHECK(hipEventElapsedTime(&ms, e.a, e.b));
        p.conv_ms += ms;
        if (e.op < 0) {  // whole-program bracket: counts every launch of the program
            for (size_t i = 0; i < nops; ++i) p.conv_launches += own_launch(ctx->unet->prog, i) ? 1 : 0;
        } else {
            p.conv_launches += 1;
        }
        if (e.op >= 0 && (size_t)e.op < nops) {
            p.op_ms[e.op] += ms;
            p.op_calls[e.op] += 1;
        }
        p.pool.push_back({e.a, e.b});
    }
    p.pending.clear();
    return EDMP_OK;
}

int unet_forward_impl(edmp_ctx* ctx, const float* x_dev, int B, int t, float* eps_dev) {
    UNet* u = ctx->unet;
    EDMP_REQUIRE(u, "edmp_unet_load has not been called");
    EDMP_REQUIRE(B >= 1 && B <= u->max_batch, "batch %d outside 1..max_batch=%d", B, u->max_batch);
    hipStream_t s = ctx->stream;
    const int N = u->desc.horizon, C = u->desc.input_dim;
    {
        int total = B * N * 8;
        hipLaunchKernelGGL(pack_input_kernel, dim3((total + 255) / 256), dim3(256), 0, s, x_dev, u->x_in, B, C, N, 8);
    }
    int rc = unet_run_program(ctx, B, t, nullptr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(head_1x1_kernel, dim3((B * N + 255) / 256), dim3(256), 0, s, u->h_last, u->head_w, u->head_b, eps_dev, B, N,
                       u->head_cin, C);
    EDMP_HIP_CHECK(hipGetLastError());
    return EDMP_OK;
}
}  // namespace edmp

extern "C" int edmp_unet_forward_dev(edmp_ctx* ctx, const float* x_dev, int B, int t, float* eps_dev) {
    EDMP_REQUIRE(ctx && x_dev && eps_dev, "edmp_unet_forward_dev: null argument");
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    sampler_end_run(ctx);  // the input buffer carries the next segment's UNet input
    return unet_forward_impl(ctx, x_dev, B, t, eps_dev);
}

extern "C" int edmp_unet_read_activation_dev(edmp_ctx* ctx, int which, int B, float* out_dev, int64_t capacity, int* C_out, int* L_out) {
    EDMP_REQUIRE(ctx && ctx->unet, "edmp_unet_read_activation_dev: no model");
    for (auto& t : ctx->unet->taps)
        if (t.which == which) {
            if (C_out) *C_out = t.C;
            if (L_out) *L_out = t.L;
            if (!out_dev && capacity == 0) return EDMP_OK;  // shape query
            EDMP_REQUIRE(out_dev, "edmp_unet_read_activation_dev: null output");
            EDMP_REQUIRE(B >= 1 && B <= ctx->unet->max_batch, "batch %d outside 1..max_batch=%d", B, ctx->unet->max_batch);
            const int64_t total = (int64_t)B * t.C * t.L;
            EDMP_REQUIRE(capacity >= total, "buffer of %lld floats, activation tap %d holds %lld (B=%d, C=%d, L=%d)", (long long)capacity, which,
                         (long long)total, B, t.C, t.L);
            hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, t.p, out_dev, B, t.L, t.C);
            EDMP_HIP_CHECK(hipGetLastError());
            return EDMP_OK;
        }
    set_error("no activation tap %d", which);
    return EDMP_ERR_ARG;
}

extern "C" int edmp_unet_flops_direct(edmp_ctx* ctx, double* direct) {
    EDMP_REQUIRE(ctx && ctx->unet && direct, "no model loaded");
    *direct = ctx->unet->flops_direct;
    return EDMP_OK;
}

extern "C" int edmp_unet_flops(edmp_ctx* ctx, double* nominal, double* executed) {
    EDMP_REQUIRE(ctx && ctx->unet, "no model loaded");
    if (nominal) *nominal = ctx->unet->flops_nominal;
    if (executed) *executed = ctx->unet->flops_exec;
    return EDMP_OK;
}

extern "C" int edmp_unet_flops_pipes(edmp_ctx* ctx, double* f32_issued, double* bf16_issued) {
    EDMP_REQUIRE(ctx && ctx->unet, "no model loaded");
    if (f32_issued) *f32_issued = ctx->unet->flops_exec - ctx->unet->flops_f32_moved;
    if (bf16_issued) *bf16_issued = ctx->unet->flops_bf16;
    return EDMP_OK;
}

extern "C" int edmp_prof_ops_bf16(edmp_ctx* ctx, int cap, int* n_ops, double* flops_bf16) {
    EDMP_REQUIRE(ctx && ctx->unet && n_ops, "edmp_prof_ops_bf16: null argument / no model");
    const int n = (int)ctx->unet->prog.size();
    *n_ops = n;
    for (int i = 0; i < n && i < cap; ++i)
        if (flops_bf16) flops_bf16[i] = ctx->unet->prog[i].flops_bf16;
    return EDMP_OK;
}

extern "C" int edmp_prof_ops(edmp_ctx* ctx, int cap, int* n_ops, double* ms, int64_t* calls, double* flops_exec, char* names) {
    EDMP_REQUIRE(ctx && ctx->unet && n_ops, "edmp_prof_ops: null argument / no model");
    EDMP_HIP_CHECK(hipSetDevice(ctx->device));
    EDMP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (int rc = prof_fold(ctx)) return rc;
    const int n = (int)ctx->unet->prog.size();
    *n_ops = n;
    for (int i = 0; i < n && i < cap; ++i) {
        const Op& op = ctx->unet->prog[i];
        if (ms) ms[i] = ctx->prof.op_ms[i];
        if (calls) calls[i] = ctx->prof.op_calls[i];
        if (flops_exec) flops_exec[i] = op.flops_exec;
        if (names) {
            strncpy(names + (size_t)i * 64, op.name, 63);
            names[(size_t)i * 64 + 63] = 0;
        }
    }
    return EDMP_OK;
}

extern "C" int edmp_cu_claim(int regs, int block, int lds_bytes, int wg_per_cu) { return owns_cu(regs, block, lds_bytes, wg_per_cu) ? 1 : 0; }

extern "C" int edmp_unet_op_attrs(edmp_ctx* ctx, int cap, int* n_ops, char* names, int* regs, int* block, int* lds_bytes, int* wg_per_cu) {
    EDMP_REQUIRE(ctx && ctx->unet && n_ops, "edmp_unet_op_attrs: null argument / no model");
    const int n = (int)ctx->unet->prog.size();
    *n_ops = n;
    for (int i = 0; i < n && i < cap; ++i) {
        const Op& op = ctx->unet->prog[i];
        if (names) {
            strncpy(names + (size_t)i * 64, op.name, 63);
            names[(size_t)i * 64 + 63] = 0;
        }
        if (regs) regs[i] = op.attrs.regs;
        if (block) block[i] = op.attrs.block;
        if (lds_bytes) lds_bytes[i] = op.attrs.lds;
        if (wg_per_cu) wg_per_cu[i] = op.attrs.wg_per_cu;
    }
    return EDMP_OK;
}

#ifdef EDMP_STAMPS
extern "C" int edmp_debug_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(edmp::g_stamps), sizeof(unsigned long long) * 8 * 16);
}
#endif
