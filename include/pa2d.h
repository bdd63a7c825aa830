/* libpa2d — C ABI of the MI355X-native Transolver Physics-Attention hot path.
 *
 * Drop-in boundary.  The reference has NO native layer: every stage below is what
 * stock PyTorch dispatches from the Python lines cited per function (paths relative to the
 * reference repo OnurBasci/TransformerBasedNavierStokeSolver).  A maintainer binds these symbols
 * with ctypes from a replacement of model/Physics_Attention.py /
 * model/Transolver_Structured_Mesh_2D.py; the shipped binding is
 * transformerbasednavierstokesolver_amd/_lib.py.
 *
 * Conventions
 *   - all tensors fp32, row-major, device pointers; "ld*" = row pitch in floats; an operand may not extend
 *     past 4 GiB (32-bit buffer descriptors): larger problems return PA2D_ERR_UNSUPPORTED before any launch;
 *   - empty problems (batch 0) are valid: maps are no-ops, reductions are zero-filled;
 *   - the caller owns every buffer (outputs and workspaces); nothing here allocates, frees or
 *     synchronises, and the library keeps NO mutable state (the GEMM engine is an explicit argument of every
 *     dense entry point) -> re-entrant, safe under hipGraph capture and on any stream;
 *   - gradient outputs of parameters take an `accumulate` flag: 0 = overwrite, 1 = add to what the buffer holds
 *     (done inside the deterministic partial-sum reduce pass, so gradient accumulation over the T/step model
 *     calls of an iteration, exp_ns.py:198-211, costs no extra launch or copy);
 *   - hipStream_t is passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return value: 0 = ok, otherwise a hipError_t or PA2D_ERR_* (never a silent fallback);
 *   - activation ids follow the reference's ACTIVATION table (…_2D.py:9-10).
 */
#ifndef PA2D_H
#define PA2D_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* pa2d_stream_t;

#define PA2D_OK 0
#define PA2D_ERR_ARG 1001          /* alignment / shape contract violated */
#define PA2D_ERR_UNSUPPORTED 1002  /* size outside the compiled kernel grid */
#define PA2D_ERR_WORKSPACE 1003    /* caller workspace too small */

/* OR-ed into the `act` argument of the dense-layer entry points: `pre` receives (forward) / holds (data gradient)
 * act'(pre-activation) instead of the pre-activation itself — what the backward of `act(x.w^T + b)` needs; for GELU
 * the derivative shares every term with the activation, so saving it costs nothing and the data-gradient epilogue
 * becomes one multiplication. */
#define PA2D_ACT_SAVE_DERIVATIVE 0x100
enum pa2d_act { PA2D_ACT_NONE = 0, PA2D_ACT_GELU = 1, PA2D_ACT_TANH = 2, PA2D_ACT_SIGMOID = 3,
                PA2D_ACT_RELU = 4, PA2D_ACT_SOFTPLUS = 5, PA2D_ACT_ELU = 6, PA2D_ACT_SILU = 7 };

const char* pa2d_version(void);

/* GEMM engines (the `engine` argument of the dense entry points):
 * PA2D_ENGINE_F32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
 * PA2D_ENGINE_SPLIT fp32-accurate split: operands split exactly into 3 bf16 terms, 6 bf16 MFMA terms per product, fp32
 *                   accumulate — same parity tolerances as the exact engine.  Used by the conv GEMMs
 *                   (forward, data and weight gradients) and by the large-M plain GEMMs (K % 32 == 0, >= 256 tiles of
 *                   256 x 128 rows x columns: forward / data gradient; weight gradient from 2048 rows); small GEMMs
 *                   stay on the exact kernels;
 * PA2D_ENGINE_BF16  bf16 compute: every GEMM rounds its operands to bf16 and uses ONE bf16 MFMA term with fp32
 *                   accumulation; tensors stay fp32 in HBM (autocast-style numerics, tolerance rel-L2 <= 3e-2).
 * Workspace sizes and weight-pack layouts depend on the engine: query them, and make packs, with the engine used.
 * pa2d_default_engine(): what a caller without a preference should pass — env PA2D_GEMM=f32|split|bf16, else
 * PA2D_ENGINE_SPLIT.  It only reads the environment; no entry point consults it implicitly. */
enum pa2d_engine { PA2D_ENGINE_F32 = 0, PA2D_ENGINE_SPLIT = 1, PA2D_ENGINE_BF16 = 2 };
int pa2d_default_engine(void);
/* Kernel-selection overrides (PA2D_CONV_HALO, PA2D_MC_BIG, PA2D_LIN_PANEL, ...: A/B timing and the parity tests that
 * force one of two equivalent kernels) and PA2D_GEMM are read from the environment ONCE, when the library is loaded;
 * pa2d_reload_env() reads them again (tests).  They never change the numerics contract of an entry point.
 * PA2D_CONV_AHEAD=0: the split engine's halo conv (16x16x32 MFMA consumers) runs the reference consumer loop instead of
 * the one that reads its LDS fragments ahead of use; the two are bit-equal. */
void pa2d_reload_env(void);

/* ---- LayerNorm: nn.LayerNorm(C) of Transolver_block, model/Transolver_Structured_Mesh_2D.py:58,62,65,70-73 */
int pa2d_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                       float* rstd, int rows, int C, float eps, pa2d_stream_t stream);
size_t pa2d_layernorm_bwd_workspace(int rows, int C);
/* dx = LN'(dy) (+ dres: gradient of the residual branch `+ fx`, …_2D.py:70-71); dgamma/dbeta reduced ((+)= per
 * `accumulate`) */
int pa2d_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                       const float* gamma, const float* dres, float* dx, float* dgamma, float* dbeta,
                       void* ws, size_t ws_bytes, int rows, int C, int accumulate, pa2d_stream_t stream);

/* ---- dense layers: nn.Linear of MLP (…_2D.py:26-38), to_out (Physics_Attention.py:81-84,119)
 * y[M,N] = act(x[M,K] . w[N,K]^T + bias) (+ res);  pre (optional) receives the pre-activation.
 * Requires K % 4 == 0 and ldx, ldw % 4 == 0.
 * ws / ws_bytes: optional scratch (NULL / 0 allowed).  With pa2d_gemm_fwd_workspace(N, K, engine) bytes the split
 * engine's large-M layers (K in {128, 256}, N % 64 == 0, M >= 32768) run on the row-stationary kernel, which reads
 * the weight as a bf16 plane image made in ws by this call; results do not depend on which kernel ran beyond fp32
 * summation order. */
size_t pa2d_gemm_fwd_workspace(int N, int K, int engine);
/* The image on its own, for callers that know the weights stand still over several calls (the model calls and the
 * backward pass of one training iteration; a rollout): made once, passed as `wimg` (then ws may be NULL).
 * transposed = 0: image of w[N, K] for the layer's forward; 1: image of w^T for its data gradient (N = the layer's input
 * width, K = its output width, w stored [K, N]).  PA2D_ERR_UNSUPPORTED where pa2d_gemm_fwd_workspace(N, K, engine) is 0. */
int pa2d_gemm_weight_image(const float* w, long long ldw, int transposed, void* img, size_t img_bytes, int N, int K,
                           int engine, pa2d_stream_t stream);
int pa2d_gemm_bias_act_fwd(const float* x, long long ldx, const float* w, long long ldw, const float* bias,
                           const float* res, long long ldres, float* y, long long ldy, float* pre,
                           long long ldpre, const void* wimg, void* ws, size_t ws_bytes, int M, int N, int K, int act,
                           int engine, pa2d_stream_t stream);
/* dx[M,K] = (dy[M,N] . w[N,K]) * act'(pre[M,K])  (pre NULL -> no activation factor);
 * ws: at least K*N floats (transposed weight; PA2D_ERR_WORKSPACE below that); pa2d_gemm_bwd_data_workspace(N, K,
 * engine) bytes also hold the weight plane image of the row-stationary kernel (as for the forward); wimg (may be NULL):
 * a ready-made image of w^T, pa2d_gemm_weight_image(w, K, 1, img, bytes, K, N, engine). */
size_t pa2d_gemm_bwd_data_workspace(int N, int K, int engine);
int pa2d_gemm_bwd_data(const float* dy, long long lddy, const float* w, long long ldw, const float* pre,
                       long long ldpre, int act, float* dx, long long lddx, const void* wimg, void* ws, size_t ws_bytes,
                       int M, int N, int K, int engine, pa2d_stream_t stream);
/* Diagnostic (returns on the host): which kernel the library's one planner picks for a forward / data-gradient GEMM.
 * kind 0 / 1: the linear above / its data gradient, (d0, d1, d2) = (M, N, K), contiguous operands, epi = 1 bias | 2 residual
 * | 4 pre-activation stored (forward) or supplied (data gradient) | 8 output pitch % 4 != 0; kind 2 / 3: the conv below
 * (nk kernels stacked, taps 9 or 27, depth 1 for 3x3) / its data gradient, (d0, d1, d2) = (B, H, W).  bf16_storage: the
 * *_bf16 entry points (engine 2 whatever `engine` says); image: weight-image scratch is on offer.
 * out[PA2D_ROUTE_FIELDS]: 0 return code of the launch's kernel choice, 1 family (0 exact fp32 tiles, 1 small split tiles,
 * 2 bf16-engine tiles, 3 halo conv, 4 row-panel, 5 row-stationary), 2-4 tile bm, bn, bk, 5 bf16 planes per operand, 6 / 7
 * halo conv on 16x16x32 MFMAs / with fragment reads placed ahead, 8 bf16 outputs, 9 epilogue variant of the persistent
 * kernels (-1 none), 10 rows on the persistent kernel, 11-13 family, bm, bn of the tail (-1 none), 14 A is read as planes,
 * 15 conv weight pack (0 none, 1 fp32 chunk 16, 2 fp32 chunk 32, 3 bf16 planes), 16 the kernel(s) read the fp32 B
 * (data gradient: the transposed weight), 17 weight-image bytes. */
#define PA2D_ROUTE_FIELDS 18
int pa2d_gemm_route(int kind, int d0, int d1, int d2, int depth, int C, int nk, int taps, int act, int epi, int engine,
                    int bf16_storage, int image, int* out);
size_t pa2d_gemm_bwd_weight_workspace(int M, int N, int K, int engine);
/* dw[N,K] (+)= dy[M,N]^T . x[M,K];  db[N] (+)= column sums of dy (db may be NULL) */
int pa2d_gemm_bwd_weight(const float* dy, long long lddy, const float* x, long long ldx, float* dw, float* db,
                         void* ws, size_t ws_bytes, int M, int N, int K, int accumulate, int engine,
                         pa2d_stream_t stream);

/* ---- in_project_x / in_project_fx: two Conv2d(C, C, 3, 1, 1) on the same input,
 * Physics_Attention.py:74-75,91-97, as ONE implicit GEMM on the NHWC ([B,N,C]) tensor.
 * out[B*H*W, 2C] = [x_mid | fx_mid] (heads are channel groups h*D..h*D+D-1 of each half).
 * Weights in the checkpoint layout [C_out, C_in, 3, 3].  Requires C % 16 == 0.
 * ev_start / ev_stop: optional hipEvent_t (NULL = none) recorded on `stream` immediately around the
 * implicit-GEMM launch (forward: the [B*N,9C]x[9C,2C] product; backward: the data-gradient product),
 * so a benchmark can time that kernel alone without a profiler. */
size_t pa2d_conv3x3x2_workspace(int B, int H, int W, int C, int engine);       /* backward */
size_t pa2d_conv3x3x2_fwd_workspace(int B, int H, int W, int C, int engine);   /* forward  */
/* Packed weights.  The implicit GEMM reads the two [C,C,3,3] kernels from a K-major pack whose layout depends on
 * the tile / K-step chosen for (B,H,W,C) and on the engine.  By default fwd/bwd build it per call into `ws`
 * (weights change every optimizer step).  A caller that knows the weights are constant over several calls (the
 * T/step calls of one training iteration, a rollout) packs once with pa2d_conv3x3x2_pack and passes the result
 * as `prepacked`; direction 0 = forward pack, 1 = data-gradient pack (taps flipped, in/out swapped). */
size_t pa2d_conv3x3x2_pack_bytes(int C);
int pa2d_conv3x3x2_pack(const float* wx, const float* wf, void* pack, size_t pack_bytes, int B, int H, int W,
                        int C, int direction, int engine, pa2d_stream_t stream);
int pa2d_conv3x3x2_fwd(const float* xn, const float* wx, const float* bx, const float* wf, const float* bf,
                       float* out, const void* prepacked /* NULL = pack here */, void* ws, size_t ws_bytes,
                       int B, int H, int W, int C, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* dxn may be NULL (input needs no gradient); dwx/dbx/dwf/dbf (+)= per `accumulate` */
int pa2d_conv3x3x2_bwd(const float* dout, const float* xn, const float* wx, const float* wf, float* dxn,
                       float* dwx, float* dbx, float* dwf, float* dbf, const void* prepacked /* NULL = pack here */,
                       void* ws, size_t ws_bytes, int B, int H, int W, int C, int accumulate, int engine,
                       pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- in_project_x of the conv slice predictors (reference SliceLearner.py:71,124-126; LearnSlice.py forward_from_vorticity):
 * ONE Conv2d(C, C, 3, 1, 1) on the NHWC [B,N,C] tensor as the implicit GEMM [B*H*W, 9C] x [9C, C].  The kernels and the
 * engine choice of the pair above (forward and data gradient with N = C, Cin = C, K = 9C; the weight gradient of one half);
 * nothing of a second kernel is computed.  Same contract: C % 16 == 0, every engine, accumulate, dxn may be NULL, prepacked
 * (direction 0 = forward pack, 1 = data-gradient pack), ev_start / ev_stop, B <= 0 a no-op (dw / db zero-filled when
 * accumulate = 0); an operand past 4 GiB returns PA2D_ERR_UNSUPPORTED. */
size_t pa2d_conv3x3_workspace(int B, int H, int W, int C, int engine);       /* backward */
size_t pa2d_conv3x3_fwd_workspace(int B, int H, int W, int C, int engine);   /* forward  */
size_t pa2d_conv3x3_pack_bytes(int C);
int pa2d_conv3x3_pack(const float* w, void* pack, size_t pack_bytes, int B, int H, int W, int C, int direction, int engine,
                      pa2d_stream_t stream);
int pa2d_conv3x3_fwd(const float* xn, const float* w, const float* b, float* out, const void* prepacked /* NULL = pack here */,
                     void* ws, size_t ws_bytes, int B, int H, int W, int C, int engine, pa2d_stream_t stream, void* ev_start,
                     void* ev_stop);
int pa2d_conv3x3_bwd(const float* dout, const float* xn, const float* w, float* dxn, float* dw, float* db,
                     const void* prepacked /* NULL = pack here */, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                     int accumulate, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- in_project_x / in_project_fx of the structured 3-D mesh: two Conv3d(C, C, 3, 1, 1) on the same input,
 * reference model/Physics_Attention.py (Physics_Attention_Structured_Mesh_3D.forward), as ONE implicit GEMM
 * [B*H*W*D, 27C] x [27C, 2C] on the [B,N,C] tensor with N = H*W*D and point n = (h*W + w)*D + d (D fastest, the
 * reference's reshape to [B,H,W,D,C]).  Weights [C_out, C_in, 3, 3, 3] (kernel axes on H, W, D), zero padding on all
 * six faces.  Same contract as the 3x3 pair above (engines, C % 16 == 0, accumulate, B <= 0, prepacked packs:
 * direction 1 mirrors the taps 26 - t), with the depth D after W; B*H*W*D must fit an int. */
size_t pa2d_conv3x3x3x2_workspace(int B, int H, int W, int D, int C, int engine);      /* backward */
size_t pa2d_conv3x3x3x2_fwd_workspace(int B, int H, int W, int D, int C, int engine);  /* forward  */
size_t pa2d_conv3x3x3x2_pack_bytes(int C);
int pa2d_conv3x3x3x2_pack(const float* wx, const float* wf, void* pack, size_t pack_bytes, int B, int H, int W, int D,
                          int C, int direction, int engine, pa2d_stream_t stream);
int pa2d_conv3x3x3x2_fwd(const float* xn, const float* wx, const float* bx, const float* wf, const float* bf,
                         float* out, const void* prepacked /* NULL = pack here */, void* ws, size_t ws_bytes, int B,
                         int H, int W, int D, int C, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* dxn may be NULL (input needs no gradient); dwx/dbx/dwf/dbf (+)= per `accumulate` */
int pa2d_conv3x3x3x2_bwd(const float* dout, const float* xn, const float* wx, const float* wf, float* dxn,
                         float* dwx, float* dbx, float* dwf, float* dbf, const void* prepacked /* NULL = pack here */,
                         void* ws, size_t ws_bytes, int B, int H, int W, int D, int C, int accumulate, int engine,
                         pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- slice: softmax((x_mid . Ws^T + bs) / clamp(temperature, .1, 5)) and the weighted scatter of
 * N points into M tokens, Physics_Attention.py:98-101.  Emits per-chunk partial sums
 * spart [B,heads,nchunk,M,D] and npart [B,heads,nchunk,M] (npart NULL = skip), nchunk =
 * pa2d_slice_nchunk(B,N,heads); `v` is fx_mid in the forward and dY in backward phase A.
 * D in {8,16,32,64}, M <= 128.  clamp_temperature: 1 = clamp(temperature, 0.1, 5) as the structured-mesh
 * attention does (Physics_Attention.py:98-99); 0 = raw temperature (irregular mesh, :40).
 * `engine` (here, on de-slice and on the slice backward): PA2D_ENGINE_F32 = every contraction on the exact-fp32 matrix
 * instruction (v_mfma_f32_16x16x4_f32); PA2D_ENGINE_SPLIT / _BF16 = bf16 MFMA on exact 3-plane operand splits with fp32
 * accumulation (24-bit significand; the same parity tolerances).  The bf16-storage variants below have no such argument.
 * ev_start / ev_stop (here and on de-slice / slice backward): optional hipEvent_t recorded on `stream` right around
 * the point kernel, as for the conv. */
int pa2d_slice_nchunk(int B, int N, int heads);
int pa2d_slice_scatter(const float* xm, long long ldx, const float* v, long long ldv, const float* ws,
                       const float* bs, const float* temperature, float* spart, float* npart, int B, int N,
                       int heads, int D, int M, int clamp_temperature, int engine, pa2d_stream_t stream, void* ev_start,
                       void* ev_stop);

/* ---- token attention among the M slice tokens of each (batch, head): normalisation by
 * (slice_norm + 1e-5), to_q/to_k/to_v, softmax(q k^T D^-0.5), attn.v — Physics_Attention.py:102-111.
 * Outputs s (raw sums), nrm, o (out_slice_token), all [B*heads, M, (D)]. */
size_t pa2d_token_attn_lds_bytes(int M, int D, int backward);
int pa2d_token_attn_fwd(const float* spart, const float* npart, const float* wq, const float* wk,
                        const float* wv, float* s, float* nrm, float* o, int BH, int nchunk, int M, int D,
                        pa2d_stream_t stream);
size_t pa2d_token_attn_bwd_workspace(int BH, int D);
int pa2d_token_attn_bwd(const float* s, const float* nrm, const float* wq, const float* wk, const float* wv,
                        const float* dopart, float* ds, float* dn, float* dwq, float* dwk, float* dwv, void* ws,
                        size_t ws_bytes, int BH, int nchunk, int M, int D, int accumulate, pa2d_stream_t stream);

/* ---- training-mode dropout (Physics_Attention.py:51,110,282 and the Dropout of `to_out`, :28,85,257).
 * Masks come from Philox4x32-10 evaluated INSIDE the kernels (csrc/pa2d_philox.h); none is written or saved, the
 * backward evaluates the same function again.  A draw is (seed, offset, n), both 64-bit: element e < n takes word e & 3 of
 * philox(counter = (lo32(offset + e/4), hi32(offset + e/4), 0, 0), key = (lo32(seed), hi32(seed))) and is KEPT iff that word
 * >= thresh.  The caller passes thresh = floor(p * 2^32) and scale = (float)(1 / (1 - p)); no kernel computes with p.
 * A draw of n elements uses the counters offset .. offset + ceil(n / 4) - 1.
 *
 * pa2d_dropout_keep_host: HOST only; keep[i] = 1 iff element first + i of the draw is kept, i < count. */
int pa2d_dropout_keep_host(unsigned long long seed, unsigned long long offset, unsigned long long first,
                           unsigned long long count, unsigned thresh, unsigned char* keep);
/* out[e] = (res ? res[e] : 0) + (keep(e) ? z[e] * scale : 0), e < n; res may be NULL; product and sum round separately.
 * Flat and grid-stride, one Philox evaluation per four consecutive elements; 16-byte accesses where z, res and out are
 * 16-byte aligned, element by element otherwise (4-byte alignment is required: PA2D_ERR_ARG).  One trip of the grid
 * covers PA2D_DROPOUT_TRIP elements.  Forward: z = to_out(y), res = fx, element index (b N + n) C + c; backward:
 * z = dout, res = NULL gives the gradient entering to_out. */
#define PA2D_DROPOUT_TRIP (2048 * 256 * 4)
int pa2d_dropout_residual(const float* z, const float* res, float* out, long long n, unsigned thresh, float scale,
                          unsigned long long seed, unsigned long long offset, pa2d_stream_t stream);
/* pa2d_token_attn_fwd / _bwd with dropout on the attention matrix after the softmax: At = A (.) keep * scale, o = At V;
 * element ((bh M + m) M + n) of a draw of BH*M*M elements.  Backward: dV = At^T dO, dA = (dO V^T) (.) keep * scale,
 * dP = A (.) (dA - rowsum(dO (.) O)) with the UNDROPPED A (recomputed in the kernel).  Same limits as the entry points
 * above; thresh = 0, scale = 1 gives their results bit for bit. */
int pa2d_token_attn_fwd_dropout(const float* spart, const float* npart, const float* wq, const float* wk,
                                const float* wv, float* s, float* nrm, float* o, int BH, int nchunk, int M, int D,
                                unsigned thresh, float scale, unsigned long long seed, unsigned long long offset,
                                pa2d_stream_t stream);
int pa2d_token_attn_bwd_dropout(const float* s, const float* nrm, const float* wq, const float* wk, const float* wv,
                                const float* dopart, float* ds, float* dn, float* dwq, float* dwk, float* dwv, void* ws,
                                size_t ws_bytes, int BH, int nchunk, int M, int D, int accumulate, unsigned thresh,
                                float scale, unsigned long long seed, unsigned long long offset, pa2d_stream_t stream);

/* ---- de-slice: out_x = slice_weights . out_slice_token, written directly as [B,N,(h d)]
 * (Physics_Attention.py:116-117); slice weights are recomputed from x_mid, never stored. */
int pa2d_deslice_fwd(const float* xm, long long ldx, const float* o, const float* ws, const float* bs,
                     const float* temperature, float* y, long long ldy, int B, int N, int heads, int D, int M,
                     int clamp_temperature, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- backward of slice + de-slice w.r.t. the points (autograd of
 * Physics_Attention.py:98-101,116): given dY, O, dS, dn produces dx_mid, dfx_mid and the fully
 * reduced dWs [M,D], dbs [M], dtemperature [heads] (clamp mask applied; (+)= per `accumulate`). */
size_t pa2d_slice_bwd_workspace(int B, int N, int heads, int D, int M);
int pa2d_slice_bwd_points(const float* xm, long long ldx, const float* fm, long long ldf, const float* dy,
                          long long lddy, const float* ws, const float* bs, const float* temperature,
                          const float* o, const float* ds, const float* dn, float* dxm, long long lddx,
                          float* dfm, long long lddf, float* dws, float* dbs, float* dtemperature, void* ws_buf,
                          size_t ws_bytes, int B, int N, int heads, int D, int M, int clamp_temperature,
                          int accumulate, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- auto-encoder attention (reference Physics_Attention_Structured_Mesh_2D_Auto_Encoder: encode caches the softmax
 * slice weights, reconstruct_fx / decode project them with a Linear(M, M) and de-slice with the projected tensor).
 * Exact fp32 (VALU FMA) whatever engine the rest of the model uses; no engine argument.  D in {8,16,32,64}, 1 <= M <= 128,
 * N >= 1; B = 0 is a no-op (reductions zero-filled when accumulate = 0); an operand past 4 GiB returns
 * PA2D_ERR_UNSUPPORTED before any launch.  ev_start / ev_stop as for the slice stages.
 * slice weights: sw[B,heads,N,M] = softmax_m((x_mid[b,n,h*D:(h+1)*D] . ws[m,:] + bs[m]) / t_h), t_h = temperature[h]
 * (clamped to [0.1, 5] with clamp_temperature = 1); x_mid rows of pitch ldx (ldx % 4 == 0, 16-byte aligned: the column view
 * [x_mid | fx_mid] of the conv output has ldx = 2C). */
int pa2d_slice_weights_fwd(const float* xm, long long ldx, const float* ws, const float* bs, const float* temperature,
                           float* sw, int B, int N, int heads, int D, int M, int clamp_temperature, pa2d_stream_t stream,
                           void* ev_start, void* ev_stop);
/* backward from dsw [B,heads,N,M] (the weights are recomputed from x_mid): dxm (may be NULL) a plain store of rows of pitch
 * lddx; dws [M,D], dbs [M], dtemperature [heads] reduced over (b, h, n), (+)= per `accumulate` (clamp mask applied) */
size_t pa2d_slice_weights_bwd_workspace(int B, int N, int heads, int D, int M);
int pa2d_slice_weights_bwd(const float* xm, long long ldx, const float* ws, const float* bs, const float* temperature,
                           const float* dsw, float* dxm, long long lddx, float* dws, float* dbs, float* dtemperature,
                           void* ws_buf, size_t ws_bytes, int B, int N, int heads, int D, int M, int clamp_temperature,
                           int accumulate, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* de-slice with explicit weights: y[b, n, h*D + d] = sum_g w[b,h,n,g] code[b,h,g,d] (einsum "bhgc,bhng->bhnc" and the
 * rearrange to [B,N,(h d)]); code [B,heads,M,D], w [B,heads,N,M] contiguous, y rows of pitch ldy */
int pa2d_deslice_weights_fwd(const float* code, const float* w, float* y, long long ldy, int B, int N, int heads, int D,
                             int M, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* dcode [B,heads,M,D] (reduced over n; overwritten) and dw [B,heads,N,M]; either may be NULL (a frozen encoder's weights,
 * a code that needs no gradient); the workspace is needed for dcode only */
size_t pa2d_deslice_weights_bwd_workspace(int B, int N, int heads, int D, int M);
int pa2d_deslice_weights_bwd(const float* code, const float* w, const float* dy, long long lddy, float* dcode, float* dw,
                             void* ws_buf, size_t ws_bytes, int B, int N, int heads, int D, int M, pa2d_stream_t stream,
                             void* ev_start, void* ev_stop);

/* ---- SequenSolver latent sequence model (reference SequenSolver.py, class SequenSolver).  Both stages run fp32 FMAs on the
 * VALU (fp64 for the attention score sums and the small final reductions) whatever engine the rest of the model uses: no
 * engine argument.  B = 0 is a no-op (parameter gradients zero-filled when
 * accumulate = 0); an unsupported shape returns PA2D_ERR_UNSUPPORTED before any pointer is looked at.
 * sequence attention among the T frame tokens of a sample, one head (SequenSolver.py:319-331): q, k, v [B, T, dim] (the three
 * bias-free Linear(dim, dim) of the LayerNorm output: pa2d_gemm_bias_act_fwd), attn [B, T, T] = softmax_T(q k^T * scale),
 * out [B, T, dim] = attn v (+ res: the block's residual `+ tokens`, :150; may be NULL).  1 <= T <= 32, dim % 4 == 0, 4 <= dim <= 1024 (the LayerNorm limit of the tokens); pointers
 * 16-byte aligned.  attn is an output of the forward (saved for the backward; never NULL). */
int pa2d_seq_attn_fwd(const float* q, const float* k, const float* v, const float* res, float* out, float* attn, int B,
                      int T, int dim, float scale, pa2d_stream_t stream);
/* dq, dk, dv [B, T, dim] from dout (autograd of SequenSolver.py:325-328); plain stores (activations: no accumulate flag) */
size_t pa2d_seq_attn_bwd_workspace(int B, int T);
int pa2d_seq_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dout, float* dq,
                      float* dk, float* dv, void* ws, size_t ws_bytes, int B, int T, int dim, float scale,
                      pa2d_stream_t stream);
/* causal mode (the merged model's mask, SequenSolverMerged.py SequenSolver.attention): same operands, limits and workspace
 * as pa2d_seq_attn_fwd / _bwd; the row softmax runs over j <= i only and attn[i, j > i] is stored as exactly 0; in the
 * backward the ds sum runs over k <= i and ds[i, j > i] is exactly 0 */
int pa2d_seq_attn_causal_fwd(const float* q, const float* k, const float* v, const float* res, float* out, float* attn,
                             int B, int T, int dim, float scale, pa2d_stream_t stream);
int pa2d_seq_attn_causal_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dout, float* dq,
                             float* dk, float* dv, void* ws, size_t ws_bytes, int B, int T, int dim, float scale,
                             pa2d_stream_t stream);
/* fused head attention of the merged SequenSolver (SequenSolverMerged.py, SequenSolver.attention): x [G, T, sd] is the
 * LayerNorm output [B, T, dim] read as G = B*heads groups of T pseudo-rows of sd = dim / heads floats; wq, wk, wv [sd, sd]
 * (bias-free Linear(sd, sd), shared by all groups); per group q, k, v = x wq^T, x wk^T, x wv^T,
 * attn [G, T, T] = softmax_T(q k^T * scale) (causal != 0: over j <= i, attn[i, j > i] = 0 exactly),
 * out [G, T, sd] = attn v (+ res, may be NULL).  One launch.  1 <= T <= 32, sd % 4 == 0, 4 <= sd <= 64; pointers 16-byte
 * aligned; G = 0 is a no-op.  attn is an output of the forward (the only tensor saved for the backward; never NULL). */
int pa2d_head_seq_attn_fwd(const float* x, const float* wq, const float* wk, const float* wv, const float* res, float* out,
                           float* attn, int G, int T, int sd, float scale, int causal, pa2d_stream_t stream);
/* dx [G, T, sd] = dq wq + dk wk + dv wv (plain store) and dwq, dwk, dwv [sd, sd] (+)= per `accumulate`; q, k, v are
 * recomputed from x.  The workspace holds one partial record of the three weight gradients per workgroup (at most 32),
 * summed in a fixed order in fp64 by a second launch. */
size_t pa2d_head_seq_attn_bwd_workspace(int G, int T, int sd);
int pa2d_head_seq_attn_bwd(const float* x, const float* wq, const float* wk, const float* wv, const float* attn,
                           const float* dout, float* dx, float* dwq, float* dwk, float* dwv, void* ws, size_t ws_bytes,
                           int G, int T, int sd, float scale, int causal, int accumulate, pa2d_stream_t stream);
/* slice weights predicted from the code (SequenSolver.py:159-170, use_gt=False: the loop that fills a [B, N, M, C+2] tensor
 * with cat(code[b, 0, m, :], pos[b, n, :2]), weight_projection = MLP(C+2, 64, 1) with n_layers=1 and res=True (:18-43, :102),
 * softmax over M): sw[b, 0, n, :] = softmax_m(w3 . (h + gelu(w2 h + b2)) + b3), h = gelu(w1 [code_m ; pos_n] + b1), GELU exact.
 * The concatenated tensor is never made.  code [B, M, C], pos [B, N, 2], w1 [hidden, C+2], b1 [hidden], w2 [hidden, hidden],
 * b2 [hidden], w3 [1, hidden], b3 [1], sw [B, 1, N, M].  C in {8, 16, 32, 64}, 1 <= M <= 128, N >= 1, hidden = 64 and
 * depth = 1 (the hidden layers of the MLP) only.  ev_start / ev_stop as for the slice stages.
 * These three entry points are the P = 2 case of pa2d_point_slice_weights_* below (pos is feat, w1 is [hidden, C+P]) and
 * forward to them: same kernels, same checks in the same order, same return codes.  Two consequences a caller can see:
 * the backward workspace is the point path's, 256 B per point and its dW1p records included (8 MiB more at B = 8,
 * N = 4096, M = 16 than these entry points once asked for; size the buffer from pa2d_code_slice_weights_bwd_workspace),
 * and the extent limit is the point path's, B*N*max(M, 64)*4 < 4 GiB (for M < 64 about 16.7 M points per call, not
 * 2^30 / M).  In the results, the two point columns dw1[:, C:C+2] are summed as the point path sums dW1p (fixed ranges of
 * points, their records in fp64), which rounds differently from the per-tile wave sums these entry points once had; every
 * other output keeps its bits. */
int pa2d_code_slice_weights_fwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, float* sw, int B, int N, int M, int C,
                                int hidden, int depth, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* backward from dsw [B, 1, N, M] (the forward is recomputed): dcode [B, M, C] (plain store; may be NULL) and the six
 * parameter gradients, reduced over (b, n, m) in a fixed order, (+)= per `accumulate`.  The positions get no gradient. */
size_t pa2d_code_slice_weights_bwd_workspace(int B, int N, int M, int C);
int pa2d_code_slice_weights_bwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, const float* dsw, float* dcode,
                                float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ws_buf,
                                size_t ws_bytes, int B, int N, int M, int C, int hidden, int depth, int accumulate,
                                pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- LearnSlice (reference LearnSlice.py:41-153, class LearnSlice; SequenSolver.py:182-291 loads it): slice weights from
 * the code and P features per mesh point, weight_projection = MLP(C+P, 64, 1) on cat(code[b, m, :], feat[b, n, :]) and a
 * softmax over M.  The point part of the first layer is P wide and the point term W1p feat_n is made once per point;
 * pa2d_code_slice_weights_* above is the case P = 2.  code [B, M, C], feat [B, N, P], w1 [hidden, C+P], the other operands as above,
 * sw [B, 1, N, M].  1 <= P <= 128, C in {8, 16, 32, 64}, 1 <= M <= 128, N >= 1, hidden = 64, depth = 1.  Exact fp32 FMAs on
 * every engine; B = 0 and unsupported shapes as for the SequenSolver stages. */
int pa2d_point_slice_weights_fwd(const float* code, const float* feat, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* w3, const float* b3, float* sw, int B, int N, int M, int C,
                                 int P, int hidden, int depth, pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* backward from dsw [B, 1, N, M] (the forward is recomputed): dcode [B, M, C] (plain store; may be NULL) and the six
 * parameter gradients, reduced over (b, n, m) in a fixed order, (+)= per `accumulate`.  The features get no gradient. */
size_t pa2d_point_slice_weights_bwd_workspace(int B, int N, int M, int C, int P);
int pa2d_point_slice_weights_bwd(const float* code, const float* feat, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* w3, const float* b3, const float* dsw, float* dcode,
                                 float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ws_buf,
                                 size_t ws_bytes, int B, int N, int M, int C, int P, int hidden, int depth, int accumulate,
                                 pa2d_stream_t stream, void* ev_start, void* ev_stop);
/* the trainer's loss (LearnSlice.py:499-510, the sum over the points of F.mse_loss(w_n, target_n)): sw, target [rows, M]
 * with rows = B*N, loss[0] = sum_rows (1/M) sum_m (sw - target)^2 (per-workgroup partial sums over fixed ranges, added in
 * order in fp64); dsw = gout[0] * 2/M * (sw - target), gout a device scalar.  rows = 0: loss 0. */
size_t pa2d_slice_mse_workspace(long long rows, int M);
int pa2d_slice_mse_fwd(const float* sw, const float* target, float* loss, void* ws, size_t ws_bytes, long long rows, int M,
                       pa2d_stream_t stream);
int pa2d_slice_mse_bwd(const float* sw, const float* target, const float* gout, float* dsw, long long rows, int M,
                       pa2d_stream_t stream);

/* ---- conv slice predictors (reference SliceLearner.py, class SliceLearner; LearnSlice.py:155-193 forward_from_vorticity).
 * Exact fp32 on every engine (no engine argument); every sum over the rows is made of per-workgroup partial sums over fixed
 * ranges, added in a fixed order (the final sums in fp64): no atomics, bitwise repeatable.  rows = 0 is a no-op (parameter
 * gradients zero-filled when accumulate = 0); an unsupported shape returns PA2D_ERR_UNSUPPORTED before any pointer is looked
 * at, an operand past 4 GiB likewise.
 * z-score over a WHOLE tensor (LearnSlice.py: (t - t.mean()) / (t.std(unbiased=False) + 1e-8), batch included):
 * y [rows, C] (contiguous) = (x - mu) / (sigma + 1e-8), x rows of pitch ldx (a column view of a wider tensor is fine);
 * stats[0] = mu, stats[1] = sigma (population), both fp64 in device memory.  C % 4 == 0, rows >= 1; pointers 16-byte aligned.
 * A constant input gives exact zeros and sigma = 0: a variance within rounding of zero (n*Q - S^2 <= 2^-46 n*Q for the fp64
 * sums S, Q of x, x^2) is taken as zero. */
size_t pa2d_zscore_workspace(long long rows, int C);
int pa2d_zscore_fwd(const float* x, long long ldx, float* y, double* stats, void* ws, size_t ws_bytes, long long rows, int C,
                    pa2d_stream_t stream);
/* dx = (dy - mean(dy) - y * mean(dy*y) * (sigma + eps) / sigma) / (sigma + eps), rows of pitch lddy / lddx; y and stats from
 * the forward.  sigma = 0 is outside the contract (the reference's autograd gives NaN there). */
int pa2d_zscore_bwd(const float* dy, long long lddy, const float* y, const double* stats, float* dx, long long lddx, void* ws,
                    size_t ws_bytes, long long rows, int C, pa2d_stream_t stream);
/* The same z-score over `groups` independent groups of ONE tensor of pitch ldx: group g owns the rows
 * [g * rows_per_group, (g + 1) * rows_per_group) and has its own stats[g][2] = (mu, sigma).  One partial-sum launch and one
 * map launch serve all groups (the group is a grid axis), with the partition of pa2d_zscore_* on rows_per_group rows inside
 * every group: group g's y, stats and dx are BIT FOR BIT those of pa2d_zscore_fwd / _bwd on its rows alone (groups = 1 is
 * that call).  C % 4, the pitch and the alignment as above; the 4 GiB extent covers the whole tensor; 1 <= groups <= 65535
 * (else PA2D_ERR_ARG / PA2D_ERR_UNSUPPORTED); groups * rows_per_group = 0 is a no-op; a NULL operand is PA2D_ERR_ARG. */
size_t pa2d_zscore_grouped_workspace(int groups, long long rows_per_group, int C);
int pa2d_zscore_grouped_fwd(const float* x, long long ldx, float* y, double* stats, void* ws, size_t ws_bytes, int groups,
                            long long rows_per_group, int C, pa2d_stream_t stream);
int pa2d_zscore_grouped_bwd(const float* dy, long long lddy, const float* y, const double* stats, float* dx, long long lddx,
                            void* ws, size_t ws_bytes, int groups, long long rows_per_group, int C, pa2d_stream_t stream);
/* wide slice weights (SliceLearner.py:127-128: softmax(in_project_slice(x_mid) / clamp(temperature, .1, 5)); the last layer
 * of the code-conditioned predictor's MLP): sw[r, :] = softmax_m((x[r, :] . ws[m, :] + bs[m]) / t), x [rows, D] of pitch ldx,
 * ws [M, D], bs [M], t = temperature[0] (clamped to [0.1, 5] with clamp_temperature = 1), sw [rows, M].
 * D % 4 == 0, 16 <= D <= 512, 1 <= M <= 128 (any M, power of two or not).  One launch. */
int pa2d_wide_slice_weights_fwd(const float* x, long long ldx, const float* ws, const float* bs, const float* temperature,
                                float* sw, int rows, int D, int M, int clamp_temperature, pa2d_stream_t stream,
                                void* ev_start, void* ev_stop);
/* backward from dsw [rows, M] (the logits and weights are recomputed from x): dl = sw * (dsw - <sw, dsw>) / t;
 * dx = dl . ws (plain store, rows of pitch lddx; may be NULL); dws [M, D], dbs [M], dtemperature [1] reduced over the rows,
 * (+)= per `accumulate`; dtemperature = -(1/t) sum dl * logit, zero where the clamp is active.  ev_start / ev_stop around
 * the point kernel. */
size_t pa2d_wide_slice_weights_bwd_workspace(int rows, int D, int M);
int pa2d_wide_slice_weights_bwd(const float* x, long long ldx, const float* ws, const float* bs, const float* temperature,
                                const float* dsw, float* dx, long long lddx, float* dws, float* dbs, float* dtemperature,
                                void* ws_buf, size_t ws_bytes, int rows, int D, int M, int clamp_temperature, int accumulate,
                                pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ---- fused block tail for no-grad forwards: ONE launch for what the default path runs as
 * pa2d_deslice_fwd, pa2d_gemm_bias_act_fwd (to_out + residual), pa2d_layernorm_fwd (ln_2), two pa2d_gemm_bias_act_fwd
 * (the MLP) and the next pa2d_layernorm_fwd (Physics_Attention.py:116-119, …_2D.py:69-75).  For the R = B*N rows
 *   y   = deslice(xm, o[b], ws, bs, temperature, clamp)        as pa2d_deslice_fwd (clamp_temperature = 0: irregular mesh)
 *   a   = y . wo^T + bo + fx                                    fx [R, C] of pitch ldfx: the block's input
 *   h   = act(LN(a; g2, be2) . w1^T + b1)                       w1 [hidden, C]; act: any id of enum pa2d_act (no flag bits)
 *   out = h . w2^T + b2 + a                                     w2 [C, hidden]; out [R, C], always written
 *   xn  = LN(out; gn, bn)                                       only when gn / bn are given (both or neither); xn [R, C]
 * C = heads * D.  xm rows have pitch ldx (the first C columns of the conv's [B, N, 2C] output: ldx = 2C); o [B, heads, M, D].
 * y_dbg [R, C], a_dbg [R, C], h_dbg [R, hidden]: optional copies of the intermediate stages (NULL = not written; tests).
 * Supported (pa2d_block_tail_supported returns 1, else pa2d_block_tail_fwd returns PA2D_ERR_UNSUPPORTED before it looks
 * at a pointer): engine PA2D_ENGINE_SPLIT only — 3-plane bf16 splits of both operands, six MFMA terms, fp32 accumulation;
 * the other engines are refused, never run on this arithmetic; C in {64, 128, 256}, D in {8, 16, 32, 64}, 1 <= M <= 128,
 * hidden = r C with r in 1..4, any B*N (B = 0 is a no-op); an operand past 4 GiB returns PA2D_ERR_UNSUPPORTED.
 * Weight images: the kernel reads wo, w1, w2 from fragment-order bf16 plane images, pa2d_block_tail_image_bytes(N, K) bytes
 * each, made by pa2d_block_tail_weight_image(w [N, K] of pitch ldw, ...).  wimg_o / wimg_1 / wimg_2 may each be NULL: the
 * call then makes that image from the fp32 weight in `ws` (pa2d_block_tail_workspace(C, hidden) bytes hold all three; one
 * small launch each); with all three given, wo / w1 / w2 and ws may be NULL.  Pointers 16-byte aligned, ldx, ldfx % 4 == 0.
 * pa2d_block_tail_lds_bytes: the dynamic LDS of the tallest panel the launch may choose (<= 160 KiB); 0 if unsupported.
 * PA2D_TAIL_PANEL=16|32 forces the panel height (A/B timing; rows are independent, so the results are the same bits). */
int pa2d_block_tail_supported(int C, int heads, int D, int M, int hidden, int act, int engine);
size_t pa2d_block_tail_lds_bytes(int C, int heads, int D, int M, int hidden, int act, int engine);
size_t pa2d_block_tail_image_bytes(int N, int K);
int pa2d_block_tail_weight_image(const float* w, long long ldw, void* img, size_t img_bytes, int N, int K, int engine,
                                 pa2d_stream_t stream);
size_t pa2d_block_tail_workspace(int C, int hidden);
int pa2d_block_tail_fwd(const float* xm, long long ldx, const float* o, const float* ws, const float* bs,
                        const float* temperature, const float* fx, long long ldfx, const float* wo, const float* bo,
                        const float* g2, const float* be2, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* gn, const float* bn, float* out, float* xn, float* y_dbg,
                        float* a_dbg, float* h_dbg, const void* wimg_o, const void* wimg_1, const void* wimg_2, void* wsp,
                        size_t wsp_bytes, int B, int N, int heads, int D, int M, int hidden, int act, int clamp_temperature,
                        int engine, float eps, pa2d_stream_t stream);

/* ---- output head mlp2 = nn.Linear(C, out_dim), out_dim <= 8 (…_2D.py:66,73) */
int pa2d_head_fwd(const float* xn, const float* w, const float* b, float* y, int rows, int C, int out_dim,
                  pa2d_stream_t stream);
size_t pa2d_head_bwd_workspace(int rows, int C, int out_dim);
int pa2d_head_bwd(const float* dy, const float* xn, const float* w, float* dxn, float* dw, float* db, void* ws,
                  size_t ws_bytes, int rows, int C, int out_dim, int accumulate, pa2d_stream_t stream);

/* ---- elementwise out = dy * act'(pre): backward of the activation of a generic Linear+act layer
 * (MLP hidden layers with n_layers > 0, …_2D.py:28,32-36; not used by the NS/Darcy configurations) */
int pa2d_act_bwd(const float* dy, const float* pre, float* out, long long n, int act, pa2d_stream_t stream);
/* elementwise out = act(pre), the function the GEMM epilogues apply: the activation of a layer whose per-sample bias row was
 * added by the broadcast embedding add: the folded code-conditioned slice predictor */
int pa2d_act_fwd(const float* pre, float* out, long long n, int act, pa2d_stream_t stream);

/* ---- optimizer / loss side of the exp_ns iteration over flat fp32 buffers
 * (exp_ns.py:198-218: TestLoss rel-L2 sum, clip_grad_norm_, AdamW.step; lr/beta1 of the step come from
 * OneCycleLR on the host).  Buffers 16-byte aligned. */
size_t pa2d_sumsq_workspace(long long n);
int pa2d_sumsq(const float* g, long long n, float* out, void* ws, size_t ws_bytes, pa2d_stream_t stream);
/* one multi-tensor AdamW update of p (decoupled weight decay; bias corrections for step_index >= 1 are evaluated
 * in double on the host, like torch's Python scalars);
 * gnorm_sq (device scalar, may be NULL) + max_norm > 0 apply clip_grad_norm_'s coefficient on the fly */
int pa2d_adamw_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int step_index, const float* gnorm_sq,
                    float max_norm, pa2d_stream_t stream);
/* the values the AdamW kernel uses at one step, as one 32-byte row: out[8] = (lr / bias1, 1 - lr * weight_decay,
 * 1 - beta1, beta2, 1 - beta2, sqrt(bias2), eps, max_norm), each evaluated in double and rounded to float once.
 * HOST only (no stream, `out` is host memory); pa2d_adamw_step fills its kernel argument with it.
 * step_index < 1 or out == NULL: PA2D_ERR_ARG */
int pa2d_adamw_coefficients(double lr, double beta1, double beta2, double eps, double weight_decay, int step_index,
                            float max_norm, float* out);
/* pa2d_adamw_step with that row read from DEVICE memory (coef_dev: 8 floats, 16-byte aligned, PA2D_ERR_ARG otherwise;
 * written by an earlier operation of the same stream).  Same per-element arithmetic as pa2d_adamw_step (one device
 * function): equal results bit for bit.  No host work depends on the step, so the launch can sit in a hipGraph. */
int pa2d_adamw_step_dev(float* p, const float* g, float* m, float* v, long long n, const float* coef_dev,
                        const float* gnorm_sq, pa2d_stream_t stream);
/* per-sample ||pred-y||, ||y|| and their ratio (utils/testloss.py:31-42), and the gradient w.r.t. pred:
 * dpred[b] = gout[b] * (pred_b - y_b) / (dnorm_b * ynorm_b); gout is the per-sample upstream gradient [B];
 * a sample with dnorm_b == 0 gets the zero sub-gradient (as torch.norm's backward), never inf/NaN */
int pa2d_rel_l2_fwd(const float* pred, const float* y, float* dnorm, float* ynorm, float* ratio, int B,
                    long long L, pa2d_stream_t stream);
int pa2d_rel_l2_bwd(const float* pred, const float* y, const float* dnorm, const float* ynorm,
                    const float* gout, float* dpred, int B, long long L, pa2d_stream_t stream);

/* ---- the exp_darcy loss (exp_darcy.py:213-226) on the normalised head output, fused: out_n, y_n [B, s*s];
 * `mean` / `std` are the y-normaliser's scalars ON THE DEVICE (utils/normalizer.py; no host read); o = out_n std + mean,
 * y = y_n std + mean; l2_b = ||o - y|| / ||y||; o~ = o with its one-pixel border zeroed; gx / gy = zero-padded central
 * differences / (2 dx) (central_diff, exp_darcy.py:59-68); dxr_b = ||gx(o~) - gx(y)|| / ||gx(y)||, dyr_b likewise.
 * fwd: sums[3] = (sum_b l2_b + 0.1 sum_b (dxr_b + dyr_b), sum_b l2_b, sum_b (dxr_b + dyr_b)); norms [6][B] = the six
 * per-sample norms in the order above (difference, target) x (l2, d/dx, d/dy), saved for bwd.  Partial sums per row
 * tile are added in a fixed order: two calls give the same bits.  ws: pa2d_darcy_loss_workspace(B, s) bytes.
 * bwd: dout = d (coef[0] sum_b l2_b + coef[1] sum_b (dxr_b + dyr_b)) / d out_n, coef = 2 floats on the device; the
 * derivative terms vanish on the border ring; a zero difference norm gives that term the zero sub-gradient.
 * There is no gradient to y_n.  B = 0: sums are zero-filled, nothing else is touched.  An image whose rows do not fit
 * the LDS tile (s > 2048) returns PA2D_ERR_UNSUPPORTED. */
size_t pa2d_darcy_loss_workspace(int B, int s);
int pa2d_darcy_loss_fwd(const float* out_n, const float* y_n, const float* mean, const float* std, float* norms,
                        float* sums, void* ws, size_t ws_bytes, int B, int s, float dx, pa2d_stream_t stream);
int pa2d_darcy_loss_bwd(const float* out_n, const float* y_n, const float* mean, const float* std, const float* norms,
                        const float* coef, float* dout, int B, int s, float dx, pa2d_stream_t stream);

/* ---- the decoded, strided relative-L2 loss of the airfoil / pipe / elasticity / plasticity drivers (exp_pipe.py:210-213):
 * per sample ||o - y|| / ||y|| with o = pred std + mean, y = y_n std + mean (both decoded, then subtracted, as
 * pa2d_darcy_loss does).  mean / std: one-element device tensors, or NULL for BOTH = identity.  pred: [B, L] contiguous;
 * the target element (b, i) is y[b * y_batch_stride + i * y_elem_stride] (strides in elements, y_elem_stride >= 1), so a
 * slice such as yy[..., t:t+1] of [B, N, 4, T] is read in place.  Pointers need 4-byte alignment only; the kernels use
 * 16-byte accesses where the operands of a row are aligned alike and scalar accesses elsewhere.
 * fwd: a sample is split over up to PA2D_REL_L2_AFFINE_SPLIT workgroups whose partial sums are added in a fixed order
 * (two calls give the same bits); dnorm / ynorm [B] are saved for bwd, ratio [B] are the per-sample losses.
 * ws: at least 2 * B * PA2D_REL_L2_AFFINE_SPLIT floats.
 * bwd: dpred[b] = gout[b] std (o_b - y_b) / (dnorm_b ynorm_b); gout [B] is the per-sample upstream gradient; a sample
 * with dnorm_b == 0 gets the zero sub-gradient.  There is no gradient to y.  B = 0 or L = 0: nothing is touched. */
#define PA2D_REL_L2_AFFINE_SPLIT 64
int pa2d_rel_l2_affine_fwd(const float* pred, const float* y, long long y_elem_stride, long long y_batch_stride,
                           const float* mean, const float* std, float* dnorm, float* ynorm, float* ratio, void* ws,
                           size_t ws_bytes, int B, long long L, pa2d_stream_t stream);
int pa2d_rel_l2_affine_bwd(const float* pred, const float* y, long long y_elem_stride, long long y_batch_stride,
                           const float* mean, const float* std, const float* dnorm, const float* ynorm,
                           const float* gout, float* dpred, int B, long long L, pa2d_stream_t stream);

/* ---- the broadcast adds of the input embedding (model/_core.py TransolverBase._embed):
 * fwd: z[b, n, :] = (h[b, n, :] + placeholder[:]) + tvec[b, :], the sums of the torch expressions in their order, so
 * the same bits.  placeholder [C] and tvec [B, C] may each be NULL; z may be h.
 * bwd: the gradient to h is dz itself; dtvec[b, c] = sum_n dz[b, n, c] and dplaceholder[c] = sum_b dtvec[b, c], by one
 * partial-sum pass and a fixed-order finish (two calls give the same bits).  dtvec NULL: dplaceholder is reduced
 * straight from the [B N, C] rows; dplaceholder NULL: only dtvec.  Outputs are overwritten (zero-filled when B N == 0).
 * ws: at least PA2D_EMBED_BIAS_CHUNKS * (dtvec ? B : 1) * C floats.
 * C % 4 != 0 returns PA2D_ERR_UNSUPPORTED.  h, placeholder, tvec, z, dz and ws are accessed 16 bytes at a time and must be
 * 16-byte aligned (else PA2D_ERR_ARG); dplaceholder and dtvec are written element by element (4-byte alignment). */
#define PA2D_EMBED_BIAS_CHUNKS 64
int pa2d_embed_bias_fwd(const float* h, const float* placeholder, const float* tvec, float* z, int B, int N, int C,
                        pa2d_stream_t stream);
int pa2d_embed_bias_bwd(const float* dz, float* dplaceholder, float* dtvec, void* ws, size_t ws_bytes, int B, int N,
                        int C, pa2d_stream_t stream);

/* ==== first layer of the previous-slice predictor (reference LearnSlice.py:125-134: the MLP over
 * cat(slice weights [M], flattened code [M C]); the concatenation is never formed).
 *   h0[b, n, :] = act( sum_m sw[b, n, m] wsw[:, m] + tb[b, :] )
 * sw [B, N, M] slice weights (data), wsw [H, M] the first M columns of the layer's weight (contiguous), tb [B, H] the
 * per-sample row code[b] . Wtok^T + bias (a row GEMM of the caller), h0 [B, N, H]; act: the activation id of the GEMM
 * epilogues.  Exact fp32 FMAs, m ascending from tb.  One launch for any B.
 * bwd: recomputes the pre-activation from sw, wsw, tb; dpre = dh0 act'(pre);
 *   dwsw[h, m] = sum_{b, n} dpre[b, n, h] sw[b, n, m],   dtb[b, h] = sum_n dpre[b, n, h]
 * by one partial record per (sample, chunk of rows) and a fixed-order finish (two calls give the same bits; no float
 * atomics).  Both outputs are overwritten (zero-filled when B N == 0).  ws: pa2d_prev_slice_entry_workspace bytes.
 * M outside 1..64 or H % 4 != 0: PA2D_ERR_UNSUPPORTED; so is any tensor of 4 GiB or more (the buffer addressing covers
 * 32 bits) and B * ceil(N / 64) > 262140.  NULL pointers (with B N > 0) and wsw, tb, h0, dh0, ws not 16-byte aligned:
 * PA2D_ERR_ARG. */
size_t pa2d_prev_slice_entry_workspace(int B, int N, int M, int H);
int pa2d_prev_slice_entry_fwd(const float* sw, const float* wsw, const float* tb, float* h0, int B, int N, int M, int H,
                              int act, pa2d_stream_t stream);
int pa2d_prev_slice_entry_bwd(const float* dh0, const float* sw, const float* wsw, const float* tb, float* dwsw,
                              float* dtb, void* ws, size_t ws_bytes, int B, int N, int M, int H, int act,
                              pa2d_stream_t stream);

/* ==== operand-planes interface of the bf16 engines (fp32 storage; PA2D_ENGINE_SPLIT: 3 planes, PA2D_ENGINE_BF16: 1).
 * The conv GEMMs of these engines stage their activation operand as a bf16 plane image [row][C/32][NT][32].  By default
 * pa2d_conv3x3x2_fwd/bwd make it from the fp32 tensor in a pre-pass; with the entry points below the PRODUCER of the
 * operand writes the image and nothing else: LayerNorm forward (…_2D.py:70 feeding Physics_Attention.py:94,96) and the
 * slice backward (autograd of Physics_Attention.py:98-101 feeding the autograd of :94,96), which also yields the conv
 * bias gradients (`nrm` [B*heads, M] = the forward's slice norms, pa2d_token_attn_fwd: the column sums of dF are
 * sum_m nrm[m] dS[m][:], those of dX sum_m dbs_partial[m] Ws[m][:] — token-level sums, no pass over the points).
 * Use when pa2d_conv3x3x2_planes_mask(...) == 7. */
size_t pa2d_planes_bytes(long long rows, int C, int engine);
int pa2d_conv3x3x2_planes_mask(int B, int H, int W, int C, int engine);
int pa2d_layernorm_fwd_planes(const float* x, const float* gamma, const float* beta, void* planes, float* mean,
                              float* rstd, int rows, int C, float eps, int engine, pa2d_stream_t stream);
int pa2d_conv3x3x2_fwd_planes(const void* xn_planes, const float* wx, const float* bx, const float* wf, const float* bf,
                              float* out, const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                              int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);
size_t pa2d_conv3x3x2_workspace_planes(int B, int H, int W, int C, int engine);
int pa2d_conv3x3x2_bwd_planes(const void* dout_planes, const void* xn_planes, const float* wx, const float* wf, float* dxn,
                              float* dwx, float* dwf, const void* prepacked, void* ws, size_t ws_bytes, int B, int H,
                              int W, int C, int accumulate, int engine, pa2d_stream_t stream, void* ev_start,
                              void* ev_stop);
int pa2d_slice_bwd_points_planes(const float* xm, long long ldx, const float* fm, long long ldf, const float* dy,
                                 long long lddy, const float* ws, const float* bs, const float* temperature,
                                 const float* o, const float* ds, const float* dn, const float* nrm, void* dxf_planes,
                                 float* dbx, float* dbf, float* dws, float* dbs, float* dtemperature, void* ws_buf,
                                 size_t ws_bytes, int B, int N, int heads, int D, int M, int clamp_temperature,
                                 int accumulate, int engine, pa2d_stream_t stream, void* ev_start, void* ev_stop);

/* ==== bf16-STORAGE variants (BASELINE configs[2] "NS 64x64 bf16 ... DDP" and configs[4] "Darcy ... bf16"; the reference
 * would reach these numerics with torch.autocast(bfloat16) around model/Transolver_Structured_Mesh_2D.py:202-220).
 * Same stages, same argument order as the fp32 entry points above, but every ACTIVATION pointer (inputs, outputs,
 * saved tensors, inter-kernel gradients: the `void*` arguments) holds bf16; parameters, biases, LayerNorm statistics,
 * slice partial sums / norms, token tensors and every parameter gradient stay fp32; all accumulation is fp32.  GEMMs
 * use ONE bf16 MFMA term (the arithmetic of PA2D_ENGINE_BF16; conv weight packs are made by pa2d_conv3x3x2_pack_bf16).
 * ld* are in elements.  Dense layers need K % 32 == 0 (and N, K % 32 == 0 for the weight
 * gradient, whose operands must be contiguous), the conv C % 32 == 0: otherwise PA2D_ERR_UNSUPPORTED. */
int pa2d_layernorm_fwd_bf16(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                            int rows, int C, float eps, pa2d_stream_t stream);
int pa2d_layernorm_bwd_bf16(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                            const void* dres, void* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                            int rows, int C, int accumulate, pa2d_stream_t stream);
int pa2d_gemm_bias_act_fwd_bf16(const void* x, long long ldx, const float* w, long long ldw, const float* bias,
                                const void* res, long long ldres, void* y, long long ldy, void* pre, long long ldpre,
                                int M, int N, int K, int act, pa2d_stream_t stream);
int pa2d_gemm_bwd_data_bf16(const void* dy, long long lddy, const float* w, long long ldw, const void* pre,
                            long long ldpre, int act, void* dx, long long lddx, float* wt_ws, int M, int N, int K,
                            pa2d_stream_t stream);
size_t pa2d_gemm_bwd_weight_workspace_bf16(int M, int N, int K);
int pa2d_gemm_bwd_weight_bf16(const void* dy, long long lddy, const void* x, long long ldx, float* dw, float* db,
                              void* ws, size_t ws_bytes, int M, int N, int K, int accumulate, pa2d_stream_t stream);
/* weight pack for pa2d_conv3x3x2_{fwd,bwd}_bf16 (`prepacked`): pa2d_conv3x3x2_pack_bytes(C) bytes; direction as above */
int pa2d_conv3x3x2_pack_bf16(const float* wx, const float* wf, void* pack, size_t pack_bytes, int C, int direction,
                             pa2d_stream_t stream);
size_t pa2d_conv3x3x2_workspace_bf16(int B, int H, int W, int C);       /* backward */
size_t pa2d_conv3x3x2_fwd_workspace_bf16(int B, int H, int W, int C);   /* forward  */
int pa2d_conv3x3x2_fwd_bf16(const void* xn, const float* wx, const float* bx, const float* wf, const float* bf,
                            void* out, const void* prepacked, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                            pa2d_stream_t stream, void* ev_start, void* ev_stop);
int pa2d_conv3x3x2_bwd_bf16(const void* dout, const void* xn, const float* wx, const float* wf, void* dxn, float* dwx,
                            float* dbx, float* dwf, float* dbf, const void* prepacked, void* ws, size_t ws_bytes,
                            int B, int H, int W, int C, int accumulate, pa2d_stream_t stream, void* ev_start,
                            void* ev_stop);
int pa2d_slice_scatter_bf16(const void* xm, long long ldx, const void* v, long long ldv, const float* ws,
                            const float* bs, const float* temperature, float* spart, float* npart, int B, int N,
                            int heads, int D, int M, int clamp_temperature, pa2d_stream_t stream, void* ev_start,
                            void* ev_stop);
int pa2d_deslice_fwd_bf16(const void* xm, long long ldx, const float* o, const float* ws, const float* bs,
                          const float* temperature, void* y, long long ldy, int B, int N, int heads, int D, int M,
                          int clamp_temperature, pa2d_stream_t stream, void* ev_start, void* ev_stop);
int pa2d_slice_bwd_points_bf16(const void* xm, long long ldx, const void* fm, long long ldf, const void* dy,
                               long long lddy, const float* ws, const float* bs, const float* temperature,
                               const float* o, const float* ds, const float* dn, void* dxm, long long lddx,
                               void* dfm, long long lddf, float* dws, float* dbs, float* dtemperature, void* ws_buf,
                               size_t ws_bytes, int B, int N, int heads, int D, int M, int clamp_temperature,
                               int accumulate, pa2d_stream_t stream, void* ev_start, void* ev_stop);
int pa2d_head_fwd_bf16(const void* xn, const float* w, const float* b, float* y, int rows, int C, int out_dim,
                       pa2d_stream_t stream);
int pa2d_head_bwd_bf16(const float* dy, const void* xn, const float* w, void* dxn, float* dw, float* db, void* ws,
                       size_t ws_bytes, int rows, int C, int out_dim, int accumulate, pa2d_stream_t stream);

/* ---- the step tail of the velocity-field trainers (ns_velocity.py, ns_velocity_unrolling.py, ns_unrolling2_with_t.py): one
 * prediction is k = `step` columns of a [B, N, T] trajectory.  fp32, no float atomics; partial sums are added in a fixed
 * order (two calls give the same bits); caller-owned workspace / record, explicit stream, no static state; operands need
 * 4-byte alignment only (PA2D_ERR_ARG otherwise).  k outside [1, PA2D_WINDOW_MAX_K], F < k, F > PA2D_WINDOW_MAX_F or
 * B > 65535 return PA2D_ERR_UNSUPPORTED before any pointer is looked at; B = 0 or N = 0 touches nothing.
 * rel_l2_window: per sample ||pred - y|| / ||y|| of pred [B, N, k] (contiguous) against a column window of a wider
 * tensor read in place: target element (b, n, j) is y[b * y_batch_stride + n * y_row_stride + j], j < k (strides in
 * elements).  fwd writes dnorm, ynorm, ratio [B]; ws: at least 2 * B * PA2D_WINDOW_SPLIT floats.  bwd: dpred[b] =
 * gout[b] (pred_b - y_b) / (dnorm_b ynorm_b), the zero sub-gradient where dnorm_b == 0; no gradient goes to y. */
#define PA2D_WINDOW_SPLIT 64
#define PA2D_WINDOW_MAX_K 8
#define PA2D_WINDOW_MAX_F 64
int pa2d_rel_l2_window_fwd(const float* pred, const float* y, long long y_row_stride, long long y_batch_stride,
                           float* dnorm, float* ynorm, float* ratio, void* ws, size_t ws_bytes, int B, int N, int k,
                           pa2d_stream_t stream);
int pa2d_rel_l2_window_bwd(const float* pred, const float* y, long long y_row_stride, long long y_batch_stride,
                           const float* dnorm, const float* ynorm, const float* gout, float* dpred, int B, int N, int k,
                           pa2d_stream_t stream);
/* One launch per step of a no-grad prediction-feedback rollout, given pred [B, N, k]: (1) the input window [B, N, F] is
 * shifted by k columns IN PLACE and pred appended (window[..., :F-k] = window[..., k:], window[..., F-k:] = pred; a tile of
 * rows is read completely before any of its rows is written, tiles own disjoint rows); (2) traj != NULL: pred is written
 * into columns [c, c + k) of traj [B, N, T], every other column is left alone (c < 0 or c + k > T: PA2D_ERR_ARG);
 * (3) y != NULL (addressed as for rel_l2_window): this step's partial sums of (pred - y)^2 and y^2 per sample go into
 * slot s of record [S, B, PA2D_WINDOW_SPLIT, 2] (s outside [0, S) or record NULL: PA2D_ERR_ARG).
 * pa2d_rollout_score, once after the last step, adds the record in a fixed order (double): step_ratio [S, B] =
 * ||pred_s - y_s|| / ||y_s|| and full_ratio [B] = sqrt(sum_s d_s) / sqrt(sum_s y_s), which is the relative L2 of the
 * concatenated prediction against the whole target because the steps' columns partition it.  N must be the N of the
 * tail calls (it fixes how many slots of a sample are in use). */
int pa2d_rollout_tail(const float* pred, float* window, float* traj, long long T, long long c, const float* y,
                      long long y_row_stride, long long y_batch_stride, float* record, int s, int S, int B, int N, int k,
                      int F, pa2d_stream_t stream);
int pa2d_rollout_score(const float* record, float* step_ratio, float* full_ratio, int S, int B, int N,
                       pa2d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PA2D_H */
