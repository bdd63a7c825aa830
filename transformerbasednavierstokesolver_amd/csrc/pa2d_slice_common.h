// What the three slice translation units share: pa2d_slice.hip (exact-fp32 kernels of engine f32 + the C ABI of every
// slice stage), pa2d_slice3.hip (v3 scatter / de-slice on the bf16 matrix cores) and pa2d_slice3_bwd.hip (v3 backward).
// Lane reductions, the kernel parameter blocks, the (D, MT) dispatch ladder, the chunking rule and the prototypes of the
// v3 launchers.  Nothing here is part of the C ABI.
#pragma once
#include "pa2d_internal.h"

#define NEG_BIG (-1e30f)
#define LOG2E 1.44269504088896340736f

__device__ __forceinline__ float clamp_tau(float t) { return fminf(fmaxf(t, 0.1f), 5.0f); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// Reductions across the 16 lanes of a DPP row (lanes 16g..16g+15) with VALU-DPP operands instead of ds_bpermute:
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror.  After the four steps every lane of the row holds
// the row result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}
// The same on four independent values at a time as DPP-fused v_max / v_add (4 instructions per row; hipcc emits mov_dpp +
// 2 x canonicalise + op for the forms above).  The interleave covers the two wait states a DPP read needs after a VALU
// write of the same register; the leading s_nop covers the producers of the inputs, which the compiler's hazard
// recogniser does not see through the asm.
#define ROW16_OP4(OP)                                                                                        \
    asm volatile("s_nop 1\n\t"                                                                               \
                 OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %3, %3, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"                         \
                 OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                             \
                 OP " %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                             \
                 OP " %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                             \
                 OP " %3, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                             \
                 OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"                                  \
                 OP " %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"                                  \
                 OP " %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n\t"                                  \
                 OP " %3, %3, %3 row_mirror row_mask:0xf bank_mask:0xf\n\t"                                  \
                 "s_nop 1"                                                                                   \
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
__device__ __forceinline__ void row16_max4(float& a, float& b, float& c, float& d) { ROW16_OP4("v_max_f32_dpp"); }
__device__ __forceinline__ void row16_sum4(float& a, float& b, float& c, float& d) { ROW16_OP4("v_add_f32_dpp"); }

// Reductions over the four lane groups l, l ^ 16, l ^ 32, l ^ 48 (the kq index), two families that are different
// instruction sequences.  *_shfl: __shfl_xor (ds_bpermute), the exact-fp32 kernels.  *_swap: the gfx950 row swaps, the v3
// kernels — v_permlane16_swap exchanges the odd rows of its first operand with the even rows of the second,
// v_permlane32_swap the upper half of the first with the lower half of the second.
__device__ __forceinline__ float kq_max_shfl(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
__device__ __forceinline__ float kq_sum_shfl(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
#define KQ_OP(OP)                                                                                            \
    float t;                                                                                                 \
    asm volatile("v_mov_b32 %1, %0\n\t"                                                                      \
                 "s_nop 1\n\t"                                                                               \
                 "v_permlane16_swap_b32 %0, %1\n\t"                                                          \
                 OP " %0, %0, %1\n\t"                                                                        \
                 "v_mov_b32 %1, %0\n\t"                                                                      \
                 "s_nop 1\n\t"                                                                               \
                 "v_permlane32_swap_b32 %0, %1\n\t"                                                          \
                 OP " %0, %0, %1\n\t"                                                                        \
                 "s_nop 0"                                                                                   \
                 : "+v"(v), "=&v"(t));                                                                       \
    return v
__device__ __forceinline__ float kq_max_swap(float v) { KQ_OP("v_max_f32"); }
__device__ __forceinline__ float kq_sum_swap(float v) { KQ_OP("v_add_f32"); }

// ---- kernel parameter blocks, one per stage, read by the exact-fp32 and the v3 kernels alike (the exact-fp32 backward
// kernel alone takes a re-ordered copy, SliceBwdF32Params in pa2d_slice.hip)
struct SliceParams {
    const void* xm; long long ldx;      // x_mid rows: xm[(b*N+n)*ldx + h*D + d]   (float or bf16 storage)
    const void* v; long long ldv;       // values scattered (fx_mid forward, dY in backward phase A)
    const float* ws; const float* bs; const float* temperature;   // [M,D], [M], [heads]
    float* spart; float* npart;         // [B,heads,nchunk,M,D], [B,heads,nchunk,M] (npart may be null)
    int B, N, heads, M, nchunk, ppc;    // ppc = points per chunk (multiple of 16)
    unsigned x_bytes, v_bytes;          // extents for the buffer descriptors
    int clamp;                          // 1: clamp(temperature, .1, 5) (structured mesh); 0: raw (irregular mesh)
    int xcd_map;                        // workgroup numbering of the exact-fp32 kernels, see slice_decode
};
static_assert(sizeof(SliceParams) == 112, "kernel-argument layout");

struct DesliceParams {
    const void* xm; long long ldx;
    const float* o;                     // [B,heads,M,D]
    const float* ws; const float* bs; const float* temperature;
    void* y; long long ldy;             // y[(b*N+n)*ldy + h*D + d]
    int B, N, heads, M, nchunk, ppc;
    unsigned x_bytes, y_bytes;
    int clamp, xcd_map;
};
static_assert(sizeof(DesliceParams) == 104, "kernel-argument layout");

struct SliceBwdParams {
    const void* xm; long long ldx;      // x_mid
    const void* fm; long long ldf;      // fx_mid
    const void* dy; long long lddy;     // gradient w.r.t. de-sliced y
    const float* ws; const float* bs; const float* temperature;
    const float* o; const float* ds; const float* dn;   // [B,heads,M,D] x2, [B,heads,M]
    const float* nrm;                   // [B,heads,M] slice norms: v3 plane-writing kernels only (conv bias gradient)
    void* dxm; long long lddx;          // outputs
    void* dfm; long long lddf;
    void* planes; unsigned planes_bytes;   // plane-writing kernels (template argument PL > 0): [dX | dF] is written ONLY
                                        // as the bf16 plane image [row][2C/32][PL][32] the conv GEMMs stage (no fp32 dxm /
                                        // dfm), and the column sums of dX / dF (= the conv bias gradients) go to the record
    int stride;                         // floats per block record: M*D (dWs) + M (dbs) + 1 (dtau) + 2*D (dbx | dbf)
    float* part;                        // per block: [M*D (dWs) | M (dbs) | 1 (dtau) | 2*D]
    int B, N, heads, M, nchunk, ppc;
    unsigned x_bytes, f_bytes, dy_bytes, dx_bytes, df_bytes;
    int clamp, xcd_map;
};
static_assert(sizeof(SliceBwdParams) == 216, "kernel-argument layout");

// ---- host side
// The kernels are instantiated for D in {8, 16, 32, 64} and MT = ceil(M / 16) in {1, 2, 4, 8}.  The ladder returns
// CALL(D, MT) for such a shape (runtime `D`, `mt`) and falls through for every other.
#define SLICE_DISPATCH_MT(D_, CALL)                              \
    switch (mt) {                                                \
        case 1: return CALL(D_, 1);                              \
        case 2: return CALL(D_, 2);                              \
        case 4: return CALL(D_, 4);                              \
        case 8: return CALL(D_, 8);                              \
        default: break;                                          \
    }                                                            \
    break;
#define SLICE_DISPATCH_D(CALL)                                   \
    switch (D) {                                                 \
        case 8: SLICE_DISPATCH_MT(8, CALL)                       \
        case 16: SLICE_DISPATCH_MT(16, CALL)                     \
        case 32: SLICE_DISPATCH_MT(32, CALL)                     \
        case 64: SLICE_DISPATCH_MT(64, CALL)                     \
        default: break;                                          \
    }

static inline int mt_for(int M) {
    if (M <= 16) return 1;
    if (M <= 32) return 2;
    if (M <= 64) return 4;
    if (M <= 128) return 8;
    return 0;
}
// point chunks per (batch, head): about `units` (batch, head, chunk) units in all, at least 128 points (4 groups of 32) per
// unit; and the points per chunk that go with a chunk count
static inline int ppc_for(int N, int nchunk) { return ceil_div(ceil_div(N, nchunk), 32) * 32; }
static inline int slice_nchunk_for(int B, int N, int heads, int units) {
    const int bh = B * heads > 0 ? B * heads : 1;
    if (N < 1) return 1;
    int nchunk = ceil_div(units, bh);
    const int maxc = ceil_div(N, 128);
    if (nchunk > maxc) nchunk = maxc;
    if (nchunk < 1) nchunk = 1;
    return ceil_div(N, ppc_for(N, nchunk));
}
// byte extent of `rows` rows of pitch `ld` and width `w` (elements of `es` bytes) for a buffer descriptor; it has to fit
// 32 bits
static inline int slice_extent(unsigned long long rows, long long ld, unsigned long long w, unsigned long long es,
                               unsigned& bytes) {
    const unsigned long long e = ((rows - 1) * ld + w) * es;
    if (e >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    bytes = (unsigned)e;
    return PA2D_OK;
}

// v3 launchers (pa2d_slice3.hip, pa2d_slice3_bwd.hip): bf = activations stored as bf16; PA2D_ERR_UNSUPPORTED for a shape
// outside the ladder.  The backward is not built for every shape of the ladder: ask slice_bwd3_built first.
int launch_scatter3(const SliceParams& p, int D, int mt, bool bf, hipStream_t st);
int launch_deslice3(const DesliceParams& p, int D, int mt, bool bf, hipStream_t st);
bool slice_bwd3_built(int D, int mt);
int launch_slice_bwd3(const SliceBwdParams& p, int D, int mt, int planes_nt, bool bf, hipStream_t st);
