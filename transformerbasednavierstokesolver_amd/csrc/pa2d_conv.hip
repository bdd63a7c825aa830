// C ABI of the conv stages (pa2d_conv3x3*; declared in include/pa2d.h).  Host code only: the kernels live in
// pa2d_gemm_kc.hip / pa2d_gemm_split.hip / pa2d_conv_halo.hip (implicit GEMMs), pa2d_gemm_mc.hip / pa2d_gemm_mc_planes.hip
// (weight gradients) and pa2d_gemm.hip (fp32 weight packs, plan_kc, launch_kc).  Every entry point does its own family's checks
// and then runs ONE forward / ONE backward on a ConvDesc; which kernel a GEMM gets, hence its operand layout and weight pack,
// is asked of plan_kc, never predicted here.
#include "pa2d_gemm_common.h"

// ---------------------------------------------------------------------------------------------
// What the conv families differ in.  nk = kernels stacked along the output: 2 = the pair [Wx | Wf] (N = 2C forward,
// Cin = 2C for the data gradient), 1 = the single conv of the slice predictors (nothing of a second kernel is computed
// or staged).  taps = 9: 3x3 on [B,H,W,C]; 27: 3x3x3 on [B,H,W,depth,C] (point n = (h*W + w)*depth + d, weights
// [C_out, C_in, 3, 3, 3], tap t = kh*9 + kw*3 + kd; never the halo-in-LDS conv or the planes weight gradient).
enum ConvSrc {
    SRC_F32,       // fp32 tensors, split into bf16 planes here where the engine selected for a GEMM wants planes
    SRC_PLANES,    // plane images made by the producers of the operands (pa2d_layernorm_fwd_planes, pa2d_slice_bwd_points_planes)
    SRC_BF16       // bf16 storage: the tensor itself is the 1-plane image; always the bf16 kernels (engine 2), bf16 outputs
};
struct ConvDesc {
    int B, M;      // batch as passed (<= 0: empty) and the rows of the GEMMs, B*H*W*depth
    int H, W, depth, taps, C, nk, engine;
    ConvSrc src;
};
static ConvDesc conv2d(int B, int H, int W, int C, int nk, int engine, ConvSrc src) {
    return {B, B * H * W, H, W, 1, 9, C, nk, engine, src};
}
static int conv_nt(const ConvDesc& d) { return d.engine == 2 ? 1 : 3; }      // bf16 planes per operand

// The kernel plan_kc picks for the implicit GEMM [M, taps*Cin] x [taps*Cin, N]: direction 0 = forward (N = nk*C, Cin = C),
// 1 = data gradient (N = C, Cin = nk*C), asked with planes on offer.  What follows from it here: whether A is read as
// planes (c.a_planes), and the weight pack (c.pack, c.nt).
static KCParams conv_kc_shape(const ConvDesc& d, int direction) {
    const int N = direction ? d.C : d.nk * d.C, Cin = direction ? d.nk * d.C : d.C;
    return kc_conv_shape(d.engine, d.src == SRC_BF16, d.M, N, Cin, d.taps, d.H, d.W, d.depth);
}
static KCChoice conv_plan(const ConvDesc& d, int direction) { return plan_kc(conv_kc_shape(d, direction), true); }

// bf16 engines: bytes of the pre-split activation planes of the A operand [M, Cin] of that GEMM (0 when its kernel reads
// fp32 operands)
static size_t conv_planes_bytes(const ConvDesc& d, int direction) {
    const KCChoice c = conv_plan(d, direction);
    if (!c.a_planes) return 0;
    return (planes_bytes(d.M, direction ? d.nk * d.C : d.C, c.nt) + 255) & ~(size_t)255;
}

// The weight gradient dW[nk*C][taps*C] = dOut^T . im2col(X) as the dispatch sees it; planes: dout / x are plane images made here
static MCDesc conv_wgrad(const ConvDesc& d, const void* dout, const void* x, bool planes) {
    MCDesc w = {};
    w.A = dout; w.lda = d.nk * d.C; w.B = x; w.ldb = d.C; w.Mi = d.nk * d.C; w.Nj = d.taps * d.C; w.Mk = d.M;
    w.taps = d.taps; w.H = d.H; w.W = d.W; w.depth = d.depth; w.Cin = d.C; w.engine = d.engine;
    w.src = d.src == SRC_BF16 ? MC_SRC_BF16 : (d.src == SRC_PLANES || planes) ? MC_SRC_PLANES : MC_SRC_F32;
    return w;
}

// weight pack: fp32 pack (nk*C * taps*C floats) or 3 bf16 planes (1.5x)
static size_t conv_pack_bytes(int C, int taps, int nk) {
    const size_t pair = (size_t)3 * C * taps * C;
    return (nk == 2 ? pair : (pair + 1) / 2) * sizeof(float);
}

// Workspace of a forward [weight pack (unused if prepacked) | X planes] or a backward
// [weight pack | slabs or column-sum partials | dOut planes | X planes]; the planes (SRC_F32 on the bf16 engines only) sit
// at the END of the workspace.  All sizes in bytes.
struct ConvLayout {
    size_t pack, scratch, apl, xpl, total;
    MCChoice wg;   // kernel and split plan of the weight gradient (backward)
};
static ConvLayout conv_layout(const ConvDesc& d, bool bwd) {
    ConvLayout L = {};
    L.pack = conv_pack_bytes(d.C, d.taps, d.nk);
    if (!bwd) {
        if (d.src == SRC_F32) L.apl = conv_planes_bytes(d, 0);
        L.total = L.pack + L.apl;
        return L;
    }
    L.wg = plan_wgrad(conv_wgrad(d, nullptr, nullptr, false));
    const size_t sl = L.wg.pl.slab_floats, cs = (size_t)colsum_blocks(d.M) * d.nk * d.C;
    L.scratch = (d.src != SRC_PLANES && cs > sl ? cs : sl) * sizeof(float);      // SRC_PLANES: no bias gradient here
    if (d.src == SRC_F32) {
        L.apl = conv_planes_bytes(d, 1);
        if (L.wg.planes) L.xpl = (planes_bytes(d.M, d.C, conv_nt(d)) + 255) & ~(size_t)255;
    }
    L.total = L.pack + L.scratch + L.apl + L.xpl;
    return L;
}

// Packed conv weights in the layout the kernel planned for these dims stages (KCChoice::pack: fp32 with the channel chunk =
// K-step of the tile, or bf16 planes; bf16 storage: ALWAYS the 1-plane image, also at the narrow shapes the fp32-I/O
// engines hand to the exact kernel).  direction 0: forward pack ([nk*C][taps*C]); 1: data-gradient pack ([C][taps*nk*C], taps
// flipped).  w1 = NULL for nk = 1.  A pack stays valid while the weights, the dims and the GEMM mode do not change.
static int conv_pack(const ConvDesc& d, const float* w0, const float* w1, void* pack, int direction, hipStream_t st) {
    const KCChoice c = conv_plan(d, direction);
    if (c.pack == KC_PACK_PLANES) return launch_repack_split(w0, w1, pack, direction, c.nt, d.C, d.C, st, d.taps);
    return launch_repack(w0, w1, (float*)pack, direction ? 2 : 1, 0, c.pack == KC_PACK_F32_32 ? 32 : 16, d.C, d.C, st, d.taps);
}

// The implicit GEMM [M, taps*Cin] x [taps*Cin, N]: direction 0 = forward (N = nk*C, Cin = C, biases b0 | b1 split at C),
// 1 = data gradient (N = C, Cin = nk*C).  A: the operand as the planned kernel reads it (bf16 planes where it says so).
static KCParams conv_kc_params(const ConvDesc& d, int direction, const void* A, const void* pack, void* out,
                               const float* b0, const float* b1) {
    KCParams p = conv_kc_shape(d, direction);
    p.apre = plan_kc(p, true).a_planes ? 1 : 0;
    p.A = (const float*)A; p.B = (const float*)pack; p.C = (float*)out;
    p.bias = b0; p.bias2 = b1; p.bias_split = d.C;
    return p;
}

// out[M, nk*C] = [conv(x, w0) + b0 | conv(x, w1) + b1]   (zero padding 1, channels last).  prepacked: NULL (the weights are
// packed into ws by this call) or a direction-0 pack for the same dims.  ev_start / ev_stop go round the GEMM.
static int conv_forward(const ConvDesc& d, const void* x, const float* w0, const float* w1, const float* b0,
                        const float* b1, void* out, const void* prepacked, void* ws, size_t ws_bytes, hipStream_t st,
                        hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (!engine_ok(d.engine)) return PA2D_ERR_ARG;
    if (d.B <= 0) return PA2D_OK;
    const ConvLayout L = conv_layout(d, false);
    if (ws_bytes < L.total) return PA2D_ERR_WORKSPACE;
    if (!prepacked) {
        const int rc = conv_pack(d, w0, w1, ws, 0, st);
        if (rc) return rc;
        prepacked = ws;
    }
    if (L.apl) {
        void* const planes = (char*)ws + L.pack;
        const int rc = launch_split_planes((const float*)x, d.C, planes, (long long)d.M, d.C, conv_nt(d), st);
        if (rc) return rc;
        x = planes;
    }
    return launch_kc(conv_kc_params(d, 0, x, prepacked, out, b0, b1), true, st, ev_start, ev_stop);
}

// accumulate == 0 on an empty batch: the gradients are zero (NULL pointers are skipped)
static int conv_zero_grads(const ConvDesc& d, float* dw0, float* dw1, float* db0, float* db1, hipStream_t st) {
    const size_t wb = sizeof(float) * (size_t)d.C * d.C * d.taps, bb = sizeof(float) * d.C;
    int rz = pa2d_zero(dw0, wb, st);
    if (!rz) rz = pa2d_zero(dw1, wb, st);
    if (!rz) rz = pa2d_zero(db0, bb, st);
    return rz ? rz : pa2d_zero(db1, bb, st);
}

// dx[M, C] (plain store, may be NULL: then no event is recorded either), dw0 / dw1 [C, C, taps], db0 / db1 [C]
// ((+)= per `accumulate`; db: NULL for SRC_PLANES, whose bias gradients come from pa2d_slice_bwd_points_planes) from
// dout[M, nk*C] and x[M, C].  The order of the launches is fixed: the column-sum partials reuse the slabs' scratch.
static int conv_backward(const ConvDesc& d, const void* dout, const void* x, const float* w0, const float* w1, void* dx,
                         float* dw0, float* db0, float* dw1, float* db1, const void* prepacked, void* ws, size_t ws_bytes,
                         int accumulate, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (!engine_ok(d.engine)) return PA2D_ERR_ARG;
    if (d.B <= 0) return accumulate ? PA2D_OK : conv_zero_grads(d, dw0, dw1, db0, db1, st);
    const ConvLayout L = conv_layout(d, true);
    if (ws_bytes < L.total) return PA2D_ERR_WORKSPACE;
    const int C = d.C, M = d.M, NC = d.nk * C, NT = conv_nt(d);
    float* const scratch = (float*)((char*)ws + L.pack);
    void* const planes = (char*)ws + L.total - L.apl - L.xpl;      // dOut planes
    void* const xplanes = (char*)planes + L.apl;                   // X planes
    const void* a = dout;                                          // dOut / X as the GEMMs read them
    const void* b = x;
    int rc;
    if (L.apl && (dx || L.wg.planes)) {      // someone reads the planes of dOut
        rc = launch_split_planes((const float*)dout, NC, planes, M, NC, NT, st);
        if (rc) return rc;
        a = planes;
    }
    if (dx) {
        if (!prepacked) {
            rc = conv_pack(d, w0, w1, ws, 1, st);
            if (rc) return rc;
            prepacked = ws;
        }
        rc = launch_kc(conv_kc_params(d, 1, a, prepacked, dx, nullptr, nullptr), true, st, ev_start, ev_stop);
        if (rc) return rc;
    }
    if (L.xpl) {      // the weight gradient reads both operands as planes
        rc = launch_split_planes((const float*)x, C, xplanes, M, C, NT, st);
        if (rc) return rc;
        b = xplanes;
    }
    rc = L.wg.planes ? launch_wgrad(conv_wgrad(d, a, b, true), L.wg, scratch, st)
                     : launch_wgrad(conv_wgrad(d, dout, x, false), L.wg, scratch, st);
    if (rc) return rc;
    // slab rows [nk*C][taps][Cin] -> dw0 / dw1 [C][Cin][taps] (nk = 1: every row in the first half)
    rc = launch_reduce(scratch, L.wg.pl.splits, (long long)NC * d.taps * C, dw0, dw1, 1, C, C, st, accumulate, d.taps);
    if (rc || d.src == SRC_PLANES) return rc;
    const int split = d.nk == 2 ? C : 0;      // columns >= split are db1's
    return d.src == SRC_BF16 ? launch_colsum_bf16(dout, NC, M, NC, db0, scratch, st, db1, split, accumulate)
                             : launch_colsum((const float*)dout, NC, M, NC, db0, scratch, st, db1, split, accumulate);
}

// =============================================================================================
extern "C" {

// ---- the fused pair of 3x3 convs (Physics_Attention.py:94,96 — both projections read the same input, so they run as
// ONE implicit GEMM [B*N, 9C] x [9C, 2C]):  out[B*H*W, 2C] = [conv3x3(xn, wx) + bx | conv3x3(xn, wf) + bf]  (NHWC)
size_t pa2d_conv3x3x2_workspace(int B, int H, int W, int C, int engine) {
    return conv_layout(conv2d(B, H, W, C, 2, engine, SRC_F32), true).total;
}
size_t pa2d_conv3x3x2_fwd_workspace(int B, int H, int W, int C, int engine) {
    return conv_layout(conv2d(B, H, W, C, 2, engine, SRC_F32), false).total;
}
size_t pa2d_conv3x3x2_pack_bytes(int C) { return conv_pack_bytes(C, 9, 2); }

int pa2d_conv3x3x2_pack(const float* wx, const float* wf, void* pack, size_t pack_bytes, int B, int H, int W, int C,
                        int direction, int engine, hipStream_t st) {
    if (!engine_ok(engine)) return PA2D_ERR_ARG;
    if (pack_bytes < pa2d_conv3x3x2_pack_bytes(C)) return PA2D_ERR_WORKSPACE;
    return conv_pack(conv2d(B, H, W, C, 2, engine, SRC_F32), wx, wf, pack, direction ? 1 : 0, st);
}

int pa2d_conv3x3x2_fwd(const float* xn, const float* wx, const float* bx, const float* wf, const float* bf,
                       float* out, const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                       int engine, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    return conv_forward(conv2d(B, H, W, C, 2, engine, SRC_F32), xn, wx, wf, bx, bf, out, prepacked, ws, ws_bytes, st,
                        ev_start, ev_stop);
}

// dxn[B*N, C] (plain store), dwx/dwf [C,C,3,3], dbx/dbf [C] (accumulate != 0: added to) from dout[B*N, 2C]
int pa2d_conv3x3x2_bwd(const float* dout, const float* xn, const float* wx, const float* wf, float* dxn, float* dwx,
                       float* dbx, float* dwf, float* dbf, const void* prepacked, void* ws, size_t ws_bytes, int B,
                       int H, int W, int C, int accumulate, int engine, hipStream_t st, hipEvent_t ev_start,
                       hipEvent_t ev_stop) {
    return conv_backward(conv2d(B, H, W, C, 2, engine, SRC_F32), dout, xn, wx, wf, dxn, dwx, dbx, dwf, dbf, prepacked, ws,
                         ws_bytes, accumulate, st, ev_start, ev_stop);
}

// ---- single 3x3 conv (SliceLearner.py: in_project_x alone): ONE Conv2d(C, C, 3, 1, 1) as the implicit GEMM
// [B*N, 9C] x [9C, C]: the pair's kernels and engine choice with one kernel in the packs and the weight gradient of one half
static int conv1_check(int B, int H, int W, int C, int engine) {
    if (!engine_ok(engine)) return PA2D_ERR_ARG;
    if (C <= 0 || (C & 15)) return PA2D_ERR_UNSUPPORTED;
    if (B <= 0) return PA2D_OK;
    if (H <= 0 || W <= 0) return PA2D_ERR_ARG;
    // an operand past 4 GiB (32-bit buffer descriptors; the rows must also fit an int)
    if ((unsigned long long)B * H * W * C * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}
static ConvDesc conv1(int B, int H, int W, int C, int engine) {      // after conv1_check
    return {B, B <= 0 ? 0 : B * H * W, H, W, 1, 9, C, 1, engine, SRC_F32};
}

size_t pa2d_conv3x3_workspace(int B, int H, int W, int C, int engine) {
    return conv1_check(B, H, W, C, engine) ? 0 : conv_layout(conv1(B, H, W, C, engine), true).total;
}
size_t pa2d_conv3x3_fwd_workspace(int B, int H, int W, int C, int engine) {
    return conv1_check(B, H, W, C, engine) ? 0 : conv_layout(conv1(B, H, W, C, engine), false).total;
}
size_t pa2d_conv3x3_pack_bytes(int C) { return conv_pack_bytes(C, 9, 1); }

int pa2d_conv3x3_pack(const float* w, void* pack, size_t pack_bytes, int B, int H, int W, int C, int direction, int engine,
                      hipStream_t st) {
    const int rc = conv1_check(B, H, W, C, engine);
    if (rc) return rc;
    if (pack_bytes < pa2d_conv3x3_pack_bytes(C)) return PA2D_ERR_WORKSPACE;
    return conv_pack(conv1(B, H, W, C, engine), w, nullptr, pack, direction ? 1 : 0, st);
}

// out[B*H*W, C] = conv3x3(xn, w) + b   (zero padding 1, NHWC); prepacked: NULL or pa2d_conv3x3_pack(direction 0)
int pa2d_conv3x3_fwd(const float* xn, const float* w, const float* b, float* out, const void* prepacked, void* ws,
                     size_t ws_bytes, int B, int H, int W, int C, int engine, hipStream_t st, hipEvent_t ev_start,
                     hipEvent_t ev_stop) {
    const int rc = conv1_check(B, H, W, C, engine);
    if (rc) return rc;
    if (B > 0 && !ws) return PA2D_ERR_WORKSPACE;
    return conv_forward(conv1(B, H, W, C, engine), xn, w, nullptr, b, nullptr, out, prepacked, ws, ws_bytes, st, ev_start,
                        ev_stop);
}

// dxn[B*N, C] (plain store; may be NULL), dw [C,C,3,3], db [C] ((+)= per `accumulate`) from dout[B*N, C]
int pa2d_conv3x3_bwd(const float* dout, const float* xn, const float* w, float* dxn, float* dw, float* db,
                     const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C, int accumulate, int engine,
                     hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int rc = conv1_check(B, H, W, C, engine);
    if (rc) return rc;
    if (B > 0 && !ws) return PA2D_ERR_WORKSPACE;
    return conv_backward(conv1(B, H, W, C, engine), dout, xn, w, nullptr, dxn, dw, db, nullptr, nullptr, prepacked, ws,
                         ws_bytes, accumulate, st, ev_start, ev_stop);
}

// ---- 3x3x3 conv (Physics_Attention_Structured_Mesh_3D: two Conv3d(C, C, 3, 1, 1) on [B, H, W, D, C]).
// Rows of the GEMMs (B*H*W*D) must fit an int: larger problems return PA2D_ERR_UNSUPPORTED.
static long long conv3d_rows(int B, int H, int W, int D) {
    if (B <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
    return (long long)B * H * W * D;
}
static int conv3d_check(int B, int H, int W, int D, int C, int engine) {
    if (!engine_ok(engine)) return PA2D_ERR_ARG;
    if (C <= 0 || (C & 15)) return PA2D_ERR_UNSUPPORTED;
    if (B <= 0) return PA2D_OK;
    if (H <= 0 || W <= 0 || D <= 0) return PA2D_ERR_ARG;
    return conv3d_rows(B, H, W, D) > 0x7fffffffLL ? PA2D_ERR_UNSUPPORTED : PA2D_OK;
}
static ConvDesc conv3d(int B, int H, int W, int D, int C, int engine) {
    const long long r = conv3d_rows(B, H, W, D);
    return {B, r > 0x7fffffffLL ? 0 : (int)r, H, W, D, 27, C, 2, engine, SRC_F32};      // oversized: the call itself refuses
}

size_t pa2d_conv3x3x3x2_workspace(int B, int H, int W, int D, int C, int engine) {
    return conv_layout(conv3d(B, H, W, D, C, engine), true).total;
}
size_t pa2d_conv3x3x3x2_fwd_workspace(int B, int H, int W, int D, int C, int engine) {
    return conv_layout(conv3d(B, H, W, D, C, engine), false).total;
}
size_t pa2d_conv3x3x3x2_pack_bytes(int C) { return conv_pack_bytes(C, 27, 2); }

int pa2d_conv3x3x3x2_pack(const float* wx, const float* wf, void* pack, size_t pack_bytes, int B, int H, int W, int D,
                          int C, int direction, int engine, hipStream_t st) {
    const int rc = conv3d_check(B, H, W, D, C, engine);
    if (rc) return rc;
    if (pack_bytes < pa2d_conv3x3x3x2_pack_bytes(C)) return PA2D_ERR_WORKSPACE;
    return conv_pack(conv3d(B, H, W, D, C, engine), wx, wf, pack, direction ? 1 : 0, st);
}

int pa2d_conv3x3x3x2_fwd(const float* xn, const float* wx, const float* bx, const float* wf, const float* bf, float* out,
                         const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int D, int C, int engine,
                         hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int rc = conv3d_check(B, H, W, D, C, engine);
    if (rc) return rc;
    return conv_forward(conv3d(B, H, W, D, C, engine), xn, wx, wf, bx, bf, out, prepacked, ws, ws_bytes, st, ev_start,
                        ev_stop);
}

int pa2d_conv3x3x3x2_bwd(const float* dout, const float* xn, const float* wx, const float* wf, float* dxn, float* dwx,
                         float* dbx, float* dwf, float* dbf, const void* prepacked, void* ws, size_t ws_bytes, int B, int H,
                         int W, int D, int C, int accumulate, int engine, hipStream_t st, hipEvent_t ev_start,
                         hipEvent_t ev_stop) {
    const int rc = conv3d_check(B, H, W, D, C, engine);
    if (rc) return rc;
    return conv_backward(conv3d(B, H, W, D, C, engine), dout, xn, wx, wf, dxn, dwx, dbx, dwf, dbf, prepacked, ws, ws_bytes,
                         accumulate, st, ev_start, ev_stop);
}

// ---- operand-planes interface of the bf16 engines (fp32 storage): the producers of the conv operands (LayerNorm forward,
// slice backward) emit the bf16 plane image directly; these entry points consume it, so no fp32 copy of the operand and no
// split pre-pass exists.

// bytes of the plane image of a [rows, C] tensor under `engine` (0 for PA2D_ENGINE_F32)
size_t pa2d_planes_bytes(long long rows, int C, int engine) {
    if (engine != 1 && engine != 2) return 0;
    return planes_bytes(rows, C, engine == 2 ? 1 : 3);
}

// which conv operands `engine` consumes as planes at this shape: bit 0 = X in the forward GEMM, bit 1 = X in the weight
// gradient, bit 2 = dOut in the data AND weight gradient.  The *_planes entry points need all three (mask == 7).
int pa2d_conv3x3x2_planes_mask(int B, int H, int W, int C, int engine) {
    if (!engine_ok(engine) || B <= 0) return 0;
    const ConvDesc d = conv2d(B, H, W, C, 2, engine, SRC_F32);
    int m = 0;
    if (conv_planes_bytes(d, 0)) m |= 1;
    const bool wg_planes = plan_wgrad(conv_wgrad(d, nullptr, nullptr, false)).planes;
    if (wg_planes) m |= 2;
    if (conv_planes_bytes(d, 1) && wg_planes) m |= 4;
    return m;
}

int pa2d_conv3x3x2_fwd_planes(const void* xn_planes, const float* wx, const float* bx, const float* wf, const float* bf,
                              float* out, const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                              int engine, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (B <= 0) return PA2D_OK;
    if ((pa2d_conv3x3x2_planes_mask(B, H, W, C, engine) & 1) == 0) return PA2D_ERR_UNSUPPORTED;
    return conv_forward(conv2d(B, H, W, C, 2, engine, SRC_PLANES), xn_planes, wx, wf, bx, bf, out, prepacked, ws, ws_bytes,
                        st, ev_start, ev_stop);
}

size_t pa2d_conv3x3x2_workspace_planes(int B, int H, int W, int C, int engine) {
    return conv_layout(conv2d(B, H, W, C, 2, engine, SRC_PLANES), true).total;
}

// dxn (may be NULL), dwx / dwf ((+)= per accumulate) from the plane images of dOut [B*H*W, 2C] and X [B*H*W, C]
int pa2d_conv3x3x2_bwd_planes(const void* dout_planes, const void* xn_planes, const float* wx, const float* wf, float* dxn,
                              float* dwx, float* dwf, const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W,
                              int C, int accumulate, int engine, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const ConvDesc d = conv2d(B, H, W, C, 2, engine, SRC_PLANES);
    if (B <= 0) return accumulate ? PA2D_OK : conv_zero_grads(d, dwx, dwf, nullptr, nullptr, st);
    if (pa2d_conv3x3x2_planes_mask(B, H, W, C, engine) != 7) return PA2D_ERR_UNSUPPORTED;
    return conv_backward(d, dout_planes, xn_planes, wx, wf, dxn, dwx, nullptr, dwf, nullptr, prepacked, ws, ws_bytes,
                         accumulate, st, ev_start, ev_stop);
}

// ---- bf16 storage: activations, saved tensors and inter-kernel gradients are bf16 in HBM; weights, biases and every
// parameter gradient stay fp32.  Requires C % 32 == 0 (PA2D_ERR_UNSUPPORTED otherwise, never a silent fallback).
static ConvDesc conv_bf16(int B, int H, int W, int C) { return conv2d(B, H, W, C, 2, 2, SRC_BF16); }

int pa2d_conv3x3x2_pack_bf16(const float* wx, const float* wf, void* pack, size_t pack_bytes, int C, int direction,
                             hipStream_t st) {
    if (C & 31) return PA2D_ERR_UNSUPPORTED;
    if (pack_bytes < pa2d_conv3x3x2_pack_bytes(C)) return PA2D_ERR_WORKSPACE;
    return conv_pack(conv_bf16(0, 0, 0, C), wx, wf, pack, direction ? 1 : 0, st);
}

size_t pa2d_conv3x3x2_fwd_workspace_bf16(int B, int H, int W, int C) {
    return conv_layout(conv_bf16(B, H, W, C), false).total;
}
size_t pa2d_conv3x3x2_workspace_bf16(int B, int H, int W, int C) { return conv_layout(conv_bf16(B, H, W, C), true).total; }

// xn [B*H*W, C] bf16 -> out [B*H*W, 2C] bf16; weights / biases fp32 (prepacked: pa2d_conv3x3x2_pack_bf16)
int pa2d_conv3x3x2_fwd_bf16(const void* xn, const float* wx, const float* bx, const float* wf, const float* bf, void* out,
                            const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C, hipStream_t st,
                            hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (C & 31) return PA2D_ERR_UNSUPPORTED;
    return conv_forward(conv_bf16(B, H, W, C), xn, wx, wf, bx, bf, out, prepacked, ws, ws_bytes, st, ev_start, ev_stop);
}

// dout [B*H*W, 2C] bf16, xn bf16 -> dxn bf16 (may be NULL); dwx/dwf/dbx/dbf fp32 ((+)= per accumulate)
int pa2d_conv3x3x2_bwd_bf16(const void* dout, const void* xn, const float* wx, const float* wf, void* dxn, float* dwx,
                            float* dbx, float* dwf, float* dbf, const void* prepacked, void* ws, size_t ws_bytes, int B,
                            int H, int W, int C, int accumulate, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (C & 31) return PA2D_ERR_UNSUPPORTED;
    return conv_backward(conv_bf16(B, H, W, C), dout, xn, wx, wf, dxn, dwx, dbx, dwf, dbf, prepacked, ws, ws_bytes,
                         accumulate, st, ev_start, ev_stop);
}

}  // extern "C"
