// Internal declarations shared by the GEMM translation units of libpa2d (pa2d_gemm.hip = engine selection, plan_kc + launch_kc
// (KCParams -> KCChoice -> launch) + C ABI of the linears, pa2d_conv.hip = C ABI of the conv stages (host code only),
// pa2d_gemm_kc.hip = exact fp32 engine, pa2d_gemm_split.hip = bf16 split / bf16 compute engines, pa2d_gemm_mc.hip =
// weight-gradient dispatch (plan_wgrad, launch_wgrad), its gather kernel and the deterministic reductions,
// pa2d_gemm_mc_planes.hip = the weight-gradient kernels on plane images), launch_lds (the one launch of a kernel with more
// than 64 KB of LDS) and the leaf code the weight-gradient kernels share.  Split only so that the translation units compile
// in parallel; nothing here is part of the C ABI.
#pragma once
#include "pa2d_internal.h"
#include "pa2d_bf16_split.h"      // bf16x8 / bf16x4, split3
#include <stdlib.h>

#define EPI_ACT 1        // out = act(acc + bias)
#define EPI_STORE_PRE 2  // aux = acc + bias   (pre-activation, saved for backward)
#define EPI_MUL_DACT 4   // out = acc * act'(aux)

struct KCParams {
    const float* A; long long lda;
    const float* B; long long ldb;
    float* C; long long ldc;
    const float* bias;
    const float* bias2; int bias_split;   // columns >= bias_split take bias2[col - bias_split] (two stacked projections)
    int depth;   // taps == 27: the image's third extent (fastest spatial axis: point n = (h*W + w)*depth + d)
                 // (depth and taps sit in alignment holes: the kernel-argument layout of the other kernels is unchanged)
    const float* res; long long ldres;
    float* aux; long long ldaux;
    int M, N, K;
    int act, epi;
    int H, W, Cin;   // im2col view: A = image [B,H,W,Cin] with pixel pitch lda, K = 9*Cin
    unsigned a_bytes, b_bytes;   // extents of A and B for the buffer descriptors (filled by launch_kc)
    unsigned c_bytes, res_bytes, aux_bytes;
    int apre;   // split engine: A already holds the NT bf16 planes of every 32-channel chunk (split_planes_kernel)
    int engine; // PA2D_ENGINE_* of this call (explicit per call: the library keeps no engine state)
    int aux_deriv; // PA2D_ACT_SAVE_DERIVATIVE: aux receives / holds act'(pre-activation) instead of the pre-activation
    void* wimg;  // scratch for the weight plane image of the row-stationary linear kernel (KCChoice::wimg_bytes), or NULL
    const float* wsrc; long long wsn, wsk;   // the image's source: B[n][k] = wsrc[n * wsn + k * wsk]
    int io_bf16; // bf16-storage entry points: A (row-major [M][K] or the NHWC image), C, res and aux hold bf16; lda / ldc /
                 // ldres / ldaux stay in ELEMENTS; a bf16 A is read as pre-made 1-plane "planes" (apre = 1)
    int taps;    // im2col view: 27 = 3x3x3 conv on an image [B,H,W,depth,Cin] (K = 27*Cin; the pa2d_conv3x3x3x2_* entry
                 // points select the 27-tap kernels with it); anything else (the conv ABI passes 9) = 3x3, K = 9*Cin
};

// 27-tap geometry of the 3x3x3 implicit GEMMs: tap t = kh*9 + kw*3 + kd has offset (kh-1, kw-1, kd-1) on (H, W, depth);
// point n = (h*W + w)*depth + d, so the neighbour at that offset is row n + ((kh-1)*W + (kw-1))*depth + (kd-1).
__device__ __forceinline__ void conv3d_point(int n, int W, int depth, int& y, int& x, int& z) {
    const int t = n / depth;
    z = n - t * depth;
    y = t / W;
    x = t - y * W;
}
__device__ __forceinline__ void conv3d_tap(int tap, int& dy, int& dx, int& dz) {
    dy = tap / 9 - 1;
    dx = (tap / 3) % 3 - 1;
    dz = tap % 3 - 1;
}

__device__ __forceinline__ float gelu_f(float x) { return gelu_exact(x); }
__device__ __forceinline__ float dgelu_f(float x) { return dgelu_exact(x); }

// Branch-free epilogue of one 32x32 accumulator tile.  Ragged rows / columns are masked by the buffer
// range check (masked lanes get offset OOB_OFF: loads return 0, stores are dropped); all residual /
// pre-activation loads of the tile are issued before the first use.  ACT_ID < 0: runtime p.act.
template <bool HAS_RES, bool STORE_PRE, bool ACT, bool DACT, int ACT_ID, typename TO = float>
__device__ __forceinline__ void kc_epilogue_tile(const KCParams& p, const f32x16& acc, int row_base, int col,
                                                 __amdgpu_buffer_rsrc_t rc, __amdgpu_buffer_rsrc_t rres,
                                                 __amdgpu_buffer_rsrc_t raux) {
    constexpr unsigned ES = Act<TO>::ES;
    const bool col_ok = col < p.N;
    const float bv = (p.bias && col_ok) ? (col < p.bias_split ? p.bias[col] : p.bias2[col - p.bias_split]) : 0.f;
    unsigned offc[16];
    float rv[16], av[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row_base + (r & 3) + 8 * (r >> 2);
        const bool ok = col_ok && row < p.M;
        offc[r] = ok ? ((unsigned)row * (unsigned)p.ldc + (unsigned)col) * ES : OOB_OFF;
        if (HAS_RES) rv[r] = Act<TO>::bld1(rres, ok ? ((unsigned)row * (unsigned)p.ldres + (unsigned)col) * ES : OOB_OFF);
        if (DACT) av[r] = Act<TO>::bld1(raux, ok ? ((unsigned)row * (unsigned)p.ldaux + (unsigned)col) * ES : OOB_OFF);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row_base + (r & 3) + 8 * (r >> 2);
        float v = acc[r] + bv;
        if (STORE_PRE)
            Act<TO>::bst1(raux, offc[r] != OOB_OFF ? ((unsigned)row * (unsigned)p.ldaux + (unsigned)col) * ES : OOB_OFF,
                          p.aux_deriv ? (ACT_ID == ACT_GELU ? dgelu_f(v) : act_bwd(p.act, v)) : v);
        if (ACT) v = ACT_ID == ACT_GELU ? gelu_f(v) : act_fwd(p.act, v);
        if (DACT) v *= p.aux_deriv ? av[r] : (ACT_ID == ACT_GELU ? dgelu_f(av[r]) : act_bwd(p.act, av[r]));
        if (HAS_RES) v += rv[r];
        Act<TO>::bst1(rc, offc[r], v);
    }
}

// BIAS_ONLY: the conv implicit GEMMs only ever store acc (+ bias): one variant instead of nine (compile time)
template <int TM, int TN, bool BIAS_ONLY = false, typename TO = float>
__device__ __forceinline__ void kc_epilogue(const KCParams& p, f32x16 (&acc)[TM][TN], int row0, int col0) {
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(p.C, p.c_bytes);
    const __amdgpu_buffer_rsrc_t rres = make_rsrc(p.res ? p.res : p.C, p.res ? p.res_bytes : 0u);
    const __amdgpu_buffer_rsrc_t raux = make_rsrc(p.aux ? p.aux : p.C, p.aux ? p.aux_bytes : 0u);
    const bool has_res = p.res != nullptr;
    const bool gelu = p.act == ACT_GELU;
#define KC_EPI(HR, SP, AC, DA, ID)                                                                     \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) _Pragma("unroll") for (int i = 0; i < TM; ++i)      \
        kc_epilogue_tile<HR, SP, AC, DA, ID, TO>(p, acc[i][j], row0 + i * 32, col0 + j * 32, rc, rres, raux);
    if constexpr (BIAS_ONLY) {
        KC_EPI(false, false, false, false, 0)
    } else if (p.epi == 0) {
        if (has_res) { KC_EPI(true, false, false, false, 0) } else { KC_EPI(false, false, false, false, 0) }
    } else if (p.epi == (EPI_ACT | EPI_STORE_PRE) && gelu && !has_res) {
        KC_EPI(false, true, true, false, ACT_GELU)
    } else if (p.epi == EPI_ACT && gelu && !has_res) {          // inference: no pre-activation saved
        KC_EPI(false, false, true, false, ACT_GELU)
    } else if (p.epi == EPI_MUL_DACT && gelu && !has_res) {
        KC_EPI(false, false, false, true, ACT_GELU)
    } else {   // generic: any flag combination / activation (off the hot path)
        const bool sp = p.epi & EPI_STORE_PRE, ac = p.epi & EPI_ACT, da = p.epi & EPI_MUL_DACT;
        if (da) { if (has_res) { KC_EPI(true, false, false, true, -1) } else { KC_EPI(false, false, false, true, -1) } }
        else if (sp && ac) { if (has_res) { KC_EPI(true, true, true, false, -1) } else { KC_EPI(false, true, true, false, -1) } }
        else if (ac) { if (has_res) { KC_EPI(true, false, true, false, -1) } else { KC_EPI(false, false, true, false, -1) } }
        else { if (has_res) { KC_EPI(true, true, false, false, -1) } else { KC_EPI(false, true, false, false, -1) } }
    }
#undef KC_EPI
}

struct MCParams {
    const float* A; long long lda; int Mi;
    int depth;       // 27-tap kernels (TAPS = 27): image [B,H,W,depth,Cin], j = tap*Cin + ci with tap < 27 (an alignment
                     // hole: the kernel-argument layout of the other kernels is unchanged)
    const float* B; long long ldb; int Nj;
    float* slab;
    int Mk, chunks_per_split, splits;
    int H, W, Cin;   // im2col view of B: image [B,H,W,Cin] with pixel pitch ldb, j = tap*Cin + ci
    unsigned a_bytes, b_bytes;
    float* colsum;   // optional [splits][Mi]: per-split column sums of A (= the bias gradient of a linear layer), produced
                     // by the workgroups of column tile 0 from the A tiles they stage anyway; NULL = off
};
struct MCPlan { int big; int splits; int chunks_per_split; size_t slab_floats; };
struct KCTile { int bm, bn, bk; };

// ---- leaf code of the weight-gradient kernels (pa2d_gemm_mc.hip, pa2d_gemm_mc_planes.hip), written once; the kernels keep
// their own staging and pipelines.  Three of the four are macros because the kernels' code objects are pinned: the same
// text as an inline function (arguments by reference or by value) changes the register allocation of some instantiation.
// Workgroup -> (split, row tile, column tile) of the 64 x 64 / 128 x 128-tile kernels.  XCD-aware map (speed only): when
// the split count is a multiple of 8, blocks b, b+8, ... (one XCD under round-robin dispatch) own a contiguous range of
// splits = a contiguous range of rows m, so each XCD's L2 streams 1/8 of the operands instead of all of them.
#define MC_DECODE(splits_, tiles_i_, tiles_j_, split_, ti_, tj_)                                          \
    {                                                                                                     \
        const int tiles = (tiles_i_) * (tiles_j_);                                                        \
        if (((splits_) & 7) == 0) {                                                                       \
            const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, q = (splits_) >> 3;                   \
            split_ = xcd * q + slot / tiles;                                                              \
            const int t = slot % tiles;                                                                   \
            tj_ = t % (tiles_j_);                                                                         \
            ti_ = t / (tiles_j_);                                                                         \
        } else {                                                                                          \
            tj_ = blockIdx.x % (tiles_j_);                                                                \
            ti_ = (blockIdx.x / (tiles_j_)) % (tiles_i_);                                                 \
            split_ = blockIdx.x / tiles;                                                                  \
        }                                                                                                 \
    }
// 8 consecutive fp32 values of one operand row (two 16-byte loads u0_, u1_) -> their NT_ bf16 planes pk_[NT_]; add_cs_: also
// added to the thread's eight column sums cs_ (the bias gradient rides on the dY tiles of column tile 0)
#define MC_SPLIT_ROW8(NT_, u0_, u1_, add_cs_, cs_, pk_)                                                   \
    {                                                                                                     \
        const float4 v0_ = make_float4(__uint_as_float((u0_).x), __uint_as_float((u0_).y), __uint_as_float((u0_).z), __uint_as_float((u0_).w)); \
        const float4 v1_ = make_float4(__uint_as_float((u1_).x), __uint_as_float((u1_).y), __uint_as_float((u1_).z), __uint_as_float((u1_).w)); \
        if (add_cs_) {                                                                                    \
            cs_[0] += v0_.x; cs_[1] += v0_.y; cs_[2] += v0_.z; cs_[3] += v0_.w;                           \
            cs_[4] += v1_.x; cs_[5] += v1_.y; cs_[6] += v1_.z; cs_[7] += v1_.w;                           \
        }                                                                                                 \
        bf16x4 h0_, m0_, l0_, h1_, m1_, l1_;                                                              \
        split3(v0_, h0_, m0_, l0_);                                                                       \
        split3(v1_, h1_, m1_, l1_);                                                                       \
        pk_[0] = __builtin_shufflevector(h0_, h1_, 0, 1, 2, 3, 4, 5, 6, 7);                               \
        if constexpr ((NT_) == 3) {                                                                       \
            pk_[1] = __builtin_shufflevector(m0_, m1_, 0, 1, 2, 3, 4, 5, 6, 7);                           \
            pk_[2] = __builtin_shufflevector(l0_, l1_, 0, 1, 2, 3, 4, 5, 6, 7);                           \
        }                                                                                                 \
    }
// Column-sum epilogue: the RPP threads that staged the same column left their sums in sm[RPP][BM] (LDS is free after the
// last barrier of the K loop); thread c < BM adds them in row order and stores colsum[split][ti*BM + c].
template <int BM, int RPP>
__device__ __forceinline__ void mc_colsum_reduce(const float* sm, int tid, int ti, int split, int Mi, float* colsum) {
    static_assert(BM <= 256, "one column per thread");
    __syncthreads();
    if (tid < BM) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < RPP; ++r) t += sm[r * BM + tid];
        if (ti * BM + tid < Mi) colsum[(size_t)split * Mi + ti * BM + tid] = t;
    }
}
// Slab epilogue of the TM_ x TN_ 32x32x16 accumulators acc[i][j] of a wave into `out` (the split's slab), ragged edges
// guarded: register r of lane l is row row0 + i*32 + (r&3) + 8*(r>>2) (row0 includes 4*(l>>5)), column col0 + j*32 (col0
// includes l & 31).  Uses out, row0, col0, acc and p.Mi / p.Nj of the kernel.  One tile goes to the helper BY VALUE.
__device__ __forceinline__ void mc_store_tile(float* out, int Mi, int Nj, int row0, int col, const f32x16 acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        if (row < Mi) out[(size_t)row * Nj + col] = acc[r];
    }
}
#define MC_STORE_TILES(TM_, TN_)                                                                          \
    _Pragma("unroll") for (int j = 0; j < (TN_); ++j) {                                                   \
        const int col = col0 + j * 32;                                                                    \
        if (col >= p.Nj) continue;                                                                        \
        _Pragma("unroll") for (int i = 0; i < (TM_); ++i) mc_store_tile(out, p.Mi, p.Nj, row0 + i * 32, col, acc[i][j]); \
    }

// dynamic LDS above the 64 KB default: the attribute is set on every launch (it is per device and the call is cheap)
template <typename K, typename... Args>
static inline int launch_lds(K kernel, dim3 grid, dim3 block, int smem, hipStream_t st, Args... args) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
    return (int)hipGetLastError();
}

static inline bool engine_ok(int e) { return e >= 0 && e <= 2; }
// ---- forward / data-gradient GEMMs (pa2d_gemm.hip): one description (KCParams), one planner, one launch for every caller.
enum KCFamily {
    KC_EXACT,          // gemm_kc_kernel: exact fp32 MFMA tiles
    KC_SPLIT_SMALL,    // gemm_kc_split_kernel<64, 64>: small plain GEMMs of the split engine, operands split while staged
    KC_SPLIT,          // gemm_kc_split_kernel: per-tile kernel of the bf16 engines (conv on planes; plain GEMMs of engine 2)
    KC_HALO,           // conv_halo_kernel: 3x3 conv with the halo tile resident in LDS
    KC_PANEL,          // gemm_panel_kernel: persistent row-panel kernel on the whole 256-row blocks
    KC_ROWPANEL        // gemm_rowpanel_kernel: row-stationary kernel on the whole 128-row rounds (needs the weight image)
};
enum KCPack { KC_PACK_NONE, KC_PACK_F32_16, KC_PACK_F32_32, KC_PACK_PLANES };      // conv weight pack the kernel stages
struct KCChoice {
    int rc;                   // PA2D_OK, or what launch_kc answers: no kernel of the chosen family takes this request
    KCFamily family;
    int bm, bn, bk;           // workgroup tile and K-step (row-stationary: 128 rows x 64-column pairs, 64-k stages)
    int nt;                   // bf16 planes per operand: 3 = exact split, 1 = bf16 compute, 0 = fp32 MFMAs
    int mfma16, ahead;        // KC_HALO: 16x16x32 consumers, and their hand-placed fragment reads (else the reference loop)
    int out_bf16;             // C / res / aux hold bf16
    int mode;                 // KC_PANEL / KC_ROWPANEL: epilogue variant (0 bias + residual, 1 GELU (+ pre), 2 * GELU'(aux))
    int head_rows;            // KC_PANEL / KC_ROWPANEL: the rows they take; the other M - head_rows (< bm) go to the kernel that
    int tail_family, tail_bm, tail_bn;      // plan_kc picks for a GEMM of that many rows (-1: no tail)
    bool a_planes;            // A is read as bf16 planes ([row][32-channel chunk][nt][32]; bf16 storage: the tensor itself)
    KCPack pack;              // conv: the weight pack B must be (KC_PACK_PLANES: x nt)
    bool reads_b;             // some row goes to a kernel that reads p.B (false: the weight image serves every row)
    size_t wimg_bytes;        // plain GEMM: bytes of the weight image with which the row-stationary kernel can run (0: never)
};
#define PA2D_ROUTE_FIELDS 18      // ints in which pa2d_gemm_route reports a KCChoice (include/pa2d.h)
// Which kernel runs this GEMM.  Shapes, flags, null-ness of pointers and pa2d_env() only: nothing is dereferenced or allocated.
// Callers that only have a shape fill the shape fields and apre = 1 ("planes on offer") and read the answer.
KCChoice plan_kc(const KCParams& p, bool im2col);
// the one dispatch of every forward / data-gradient GEMM: checks, every buffer extent, plan_kc, one switch; ev0 / ev1 go round it
int launch_kc(const KCParams& p_in, bool im2col, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// shape fields of the conv implicit GEMM [M, taps*Cin] x [taps*Cin, N] on the image [., H, W, depth, Cin]; planes on offer
static inline KCParams kc_conv_shape(int engine, bool io_bf16, int M, int N, int Cin, int taps, int H, int W, int depth) {
    KCParams p = {};
    p.engine = engine; p.io_bf16 = io_bf16 ? 1 : 0; p.apre = 1;
    p.lda = Cin; p.ldb = (long long)taps * Cin; p.ldc = N;
    p.M = M; p.N = N; p.K = taps * Cin; p.H = H; p.W = W; p.Cin = Cin; p.taps = taps; p.depth = depth;
    return p;
}
// fp32 weight re-layouts: mode 0 = transpose, 1 / 2 = conv forward / data-gradient pack (w1 = NULL: one kernel in it)
int launch_repack(const float* w0, const float* w1, float* dst, int mode, int N, int K, int C, int Cin, hipStream_t st,
                  int taps = 9);
// ---- the kernels behind launch_kc: plain launchers of the variant `c` names, on a KCParams whose extents are filled in
// exact fp32 engine (pa2d_gemm_kc.hip)
int launch_kc_f32(const KCParams& p, bool im2col, const KCTile& t, hipStream_t st);
// bf16 engines (pa2d_gemm_split.hip): KC_SPLIT and KC_SPLIT_SMALL
int launch_kc_split(const KCParams& p, bool im2col, const KCChoice& c, hipStream_t st);
size_t planes_bytes(long long rows, int C, int NT);
int launch_split_planes(const float* src, long long ld, void* dst, long long rows, int C, int NT, hipStream_t st);
// taps = 27: pack of the two [C, Cin, 3, 3, 3] kernels of the 3x3x3 conv (same row image, K-step kc = cic*27 + tap)
int launch_repack_split(const float* w0, const float* w1, void* dst, int bwd, int NT, int C, int Cin, hipStream_t st,
                        int taps = 9);
// persistent row-panel kernel for large-M plain GEMMs of the bf16 engines (pa2d_gemm_panel.hip); p.M % 256 == 0
int launch_kc_panel(const KCParams& p, const KCChoice& c, hipStream_t st);
// row-stationary split-engine linears (pa2d_gemm_rowpanel.hip) on the weight plane image p.wimg; p.M % 128 == 0
int launch_pack_weight_image(const float* w, long long sn, long long sk, void* img, int N, int K, hipStream_t st);
int launch_kc_rowpanel(const KCParams& p, const KCChoice& c, hipStream_t st);
// conv with the halo tile resident in LDS (pa2d_conv_halo.hip); KC_HALO_TH x KC_HALO_TW pixels x 128 channels per workgroup
constexpr int KC_HALO_TH = 8, KC_HALO_TW = 32;
int launch_conv_halo(const KCParams& p, const KCChoice& c, hipStream_t st);
// ---- weight gradients (pa2d_gemm_mc.hip): dW[Mi][Nj] = sum_m A[m][Mi]^T . B[m (shifted by tap)][Cin], written as per-split
// slabs [splits][Mi][Nj] that launch_reduce adds up.  One description, one planner, one launch for every caller: the
// counterpart of KCParams / plan_kc / launch_kc.
enum MCSrc {
    MC_SRC_F32,       // A, B: fp32 matrices with row pitches lda, ldb (elements)
    MC_SRC_PLANES,    // plane images of the split engines ([row][32-channel chunk][plane][32] bf16), contiguous
    MC_SRC_BF16       // bf16 storage: contiguous bf16 tensors = 1-plane images (engine 2)
};
enum MCKernel { MC_K_GATHER, MC_K_F32SRC, MC_K_PLANES128, MC_K_PLANES256 };      // see plan_wgrad
struct MCDesc {
    const void* A; long long lda;      // dY / dOut [Mk][Mi]
    const void* B; long long ldb;      // X [Mk][Cin]
    int Mi, Nj, Mk;                    // Nj = taps * Cin
    int taps;                          // 1: plain dW of a linear layer; 9: 3x3 view of the image B [.,H,W,Cin]; 27: 3x3x3 view of
    int H, W, depth, Cin;              // [.,H,W,depth,Cin] (taps 1: H = W = depth = 1, Cin = Nj)
    MCSrc src;
    int engine;                        // PA2D_ENGINE_*
    float* colsum;                     // optional, MC_SRC_F32 with taps = 1: [splits][Mi] per-split column sums of A
};
struct MCChoice {
    MCKernel kernel;
    MCPlan pl;                         // the split plan; pl.splits slabs
    size_t slab_bytes;
    bool planes;                       // the kernel reads plane images: an MC_SRC_F32 caller splits BOTH operands first
                                       // (launch_split_planes) and launches with src = MC_SRC_PLANES
};
MCChoice plan_wgrad(const MCDesc& d);
int launch_wgrad(const MCDesc& d, const MCChoice& c, float* slab, hipStream_t st);
// the planes kernels behind launch_wgrad (pa2d_gemm_mc_planes.hip)
int launch_wgrad_planes(const MCDesc& d, const MCChoice& c, unsigned a_bytes, unsigned b_bytes, float* slab, hipStream_t st);
// accumulate != 0: out += sum of slabs (gradient accumulation straight into the caller's buffer); mode 1 with taps = 27
// un-packs [2C][27][Cin] into two [C][Cin][3][3][3] gradients
int launch_reduce(const float* slab, int nslab, long long count, float* out, float* out2, int mode, int C, int Cin,
                  hipStream_t st, int accumulate = 0, int taps = 9);
int pa2d_launch_reduce(const float* slab, int nslab, long long count, float* out, hipStream_t st);
int colsum_blocks(int M);
int launch_colsum_bf16(const void* X, long long ld, int M, int N, float* out, float* partial, hipStream_t st,
                       float* out2 = nullptr, int split = 0, int accumulate = 0);
int launch_colsum(const float* X, long long ld, int M, int N, float* out, float* partial, hipStream_t st,
                  float* out2 = nullptr, int split = 0, int accumulate = 0);
