// Engine selection, plan_kc (the one planner of every forward / data-gradient GEMM: every routing predicate is here and
// static), launch_kc (the one dispatch: checks, extents, plan, one switch), the fp32 weight re-layouts and the C ABI of the
// dense (linear) stages, pa2d_gemm_route included; the C ABI of the conv stages is pa2d_conv.hip.  Kernels and their plain
// launchers live in pa2d_gemm_kc.hip (exact fp32), pa2d_gemm_split.hip / pa2d_conv_halo.hip / pa2d_gemm_panel.hip /
// pa2d_gemm_rowpanel.hip (bf16 engines) and pa2d_gemm_mc.hip (weight gradients).
#include "pa2d_gemm_common.h"
#include <string.h>

// Engines (explicit `engine` argument of every dense entry point; the library keeps NO engine state, so two
// models in one process can use different engines): 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = 6-term bf16
// split at fp32 accuracy (conv GEMMs and large-M plain GEMMs; small GEMMs stay exact), 2 = bf16 compute for every GEMM (fp32 accumulate
// and storage).  pa2d_default_engine() only reads the environment (PA2D_GEMM=f32|split|bf16), default = split.

// ---- the one place the library reads the environment (pa2d_internal.h: Pa2dEnv)
static Pa2dEnv read_env() {
    auto is = [](const char* n, const char* pre) { const char* e = getenv(n); return e && strncmp(e, pre, strlen(pre)) == 0; };
    auto num = [](const char* n, int dflt) { const char* e = getenv(n); return (e && e[0]) ? atoi(e) : dflt; };
    Pa2dEnv v;
    v.conv_halo = is("PA2D_CONV_HALO", "o") ? 0 : (is("PA2D_CONV_HALO", "f") ? 2 : 1);
    v.mc_big_off = is("PA2D_MC_BIG", "o") ? 1 : 0;
    v.kc_bk16 = num("PA2D_KC_BK", 0) == 16 ? 1 : 0;
    v.mc_bk = num("PA2D_MC_BK", 16) == 32 ? 32 : 16;
    v.mc_splits = num("PA2D_MC_SPLITS", 0);
    v.mcb_splits = num("PA2D_MCB_SPLITS", 0);
    v.lin_dw_split = is("PA2D_LIN_DW_SPLIT", "of") ? 0 : 1;
    v.lin_panel = is("PA2D_LIN_PANEL", "of") ? 0 : 1;
    v.lin_rowpanel = is("PA2D_LIN_ROWPANEL", "of") ? 0 : 1;
    v.lin_small_split = is("PA2D_LIN_SMALL_SPLIT", "of") ? 0 : 1;
    v.conv_mfma16 = num("PA2D_CONV_MFMA", 16) == 32 ? 0 : 1;
    v.conv_ahead = num("PA2D_CONV_AHEAD", 1) == 0 ? 0 : 1;
    v.mc_mfma16 = num("PA2D_MC_MFMA", 16) == 32 ? 0 : 1;
    v.mc_dma = num("PA2D_MC_DMA", 1) == 0 ? 0 : 1;
    v.mc_chain = num("PA2D_MC_CHAIN", 1) == 0 ? 0 : 1;
    v.split_big = num("PA2D_SPLIT_BIG", 1);
    v.slice_map = is("PA2D_SLICE_MAP", "l") ? 0 : 1;
    v.default_engine = is("PA2D_GEMM", "f") ? 0 : (is("PA2D_GEMM", "b") ? 2 : 1);
    v.tail_panel = num("PA2D_TAIL_PANEL", 0);
    return v;
}
static Pa2dEnv g_env = read_env();
const Pa2dEnv& pa2d_env() { return g_env; }

// =============================================================================================
// plan_kc: which kernel runs a forward / data-gradient GEMM.  Every predicate of that choice is in this section and is called
// from plan_kc only; the launchers in the kernel files take the KCChoice and decide nothing.

// K-step: 32 (half the barriers of 16, full 128-byte row segments; 3-4 % faster on the conv, ~10 % on the small tiles)
// whenever the layout allows it: plain GEMMs always, the conv when Cin % 32 == 0; otherwise 16.
static int kc_bk(bool im2col, int Cin) {
    // PA2D_KC_BK=16: 16-wide K-step for the conv (124 VGPRs, 40 KB LDS -> 4 workgroups per CU)
    if (im2col && pa2d_env().kc_bk16) return 16;
    return (!im2col || (Cin % 32) == 0) ? 32 : 16;
}
// tile choice of the fp32 engine: 128x128 when that already gives >= 1.5 workgroups per CU, otherwise smaller
// tiles so that small problems (rollout at batch 1: M = 4096) still fill the 256 CUs.  The fp32 conv weight packs follow
// it (the pack's channel chunk must equal the K-step: KCChoice::pack).
static KCTile kc_tile(int M, int N, bool im2col, int Cin) {
    const int tiles_m = ceil_div(M, 128);
    const long long t128 = (long long)tiles_m * ceil_div(N, 128);
    const long long t12864 = (long long)tiles_m * ceil_div(N, 64);
    const int bk = kc_bk(im2col, Cin);
    if (N > 64 && t128 >= 384) return {128, 128, bk};
    if (t12864 >= 384 || M <= 64) return {128, 64, bk};
    return {64, 64, bk};
}
// (per-TILE kernels: the split engine serves the conv implicit GEMMs only.  Measured round 2: the K = C linears as
// 6-term splits on 128x128 tiles run at the SAME 0.155 ms as on the exact engine — they are bound by their short K loop
// (8 K-steps between a cold prologue and an epilogue), not by the matrix pipe.  Large-M linears of the bf16 engines
// therefore take the persistent row-panel kernel instead, see panel_applies / pa2d_gemm_panel.hip.)
static bool use_split(int engine, int N, bool im2col, int Cin) {
    const int m = engine;
    if (m == 1) return im2col && N > 64 && (Cin % 32) == 0;
    if (m == 2) return N > 64 && (!im2col || (Cin % 32) == 0);
    return false;
}
// Small plain GEMMs of the split engine (rollout / training at batch 1-4: a few thousand rows): 64 x 64 tiles so that
// M = 4096, N = 256 still makes 256 workgroups, both operands split while staged.  The exact-fp32 kernel these launches
// used to take spends 1024 matrix-pipe cycles per 32-deep K-step and wave (16 x v_mfma_f32_32x32x2_f32), this one 384.
static bool kc_split_small_applies(const KCParams& p, bool im2col) {
    if (!pa2d_env().lin_small_split || im2col || p.io_bf16 || p.engine != 1) return false;
    if ((p.K % 32) != 0 || p.K < 64 || p.N < 64 || p.M < 256) return false;
    return (long long)ceil_div(p.M, 128) * ceil_div(p.N, 128) < 384;      // where kc_tile leaves the 128 x 128 tiles
}
// epilogue variant of the two persistent kernels (KCChoice::mode); -1: they do not carry this epilogue
static int persistent_mode(const KCParams& p) {
    const bool gelu = p.act == ACT_GELU, has_res = p.res != nullptr;
    if (p.epi == 0) return 0;
    if (gelu && !has_res && (p.epi == (EPI_ACT | EPI_STORE_PRE) || p.epi == EPI_ACT)) return 1;
    if (gelu && !has_res && p.epi == EPI_MUL_DACT && !p.bias) return 2;
    return -1;
}
// Large-M plain GEMMs of the bf16 engines (fp32 storage: engines 1 / 2) on the persistent row-panel kernel.
// PA2D_LIN_PANEL=off sends them back to the per-tile kernels (A/B measurements).
static bool panel_applies(const KCParams& p, bool im2col) {
    if (!pa2d_env().lin_panel || im2col) return false;
    // (bf16 storage stays on the per-tile kernels: with one MFMA term and 2-byte operands the layer is a pure streaming
    //  problem and two small workgroups per CU keep more bytes in flight than one persistent one: measured 131 vs 138
    //  samples/s on the bf16-storage bench)
    if (p.io_bf16 || (p.engine != 1 && p.engine != 2)) return false;
    if ((p.K % 32) != 0 || p.N < 64) return false;
    if (persistent_mode(p) < 0) return false;
    if (p.epi == EPI_ACT && p.aux) return false;
    return (long long)(p.M / 256) * ceil_div(p.N, 128) >= 256;        // at least one tile per CU
}
// bytes of the weight plane image of an [N, K] layer (0: the row-stationary kernel does not take this shape / engine)
static size_t rowpanel_image_bytes(int N, int K, int engine) {
    if (engine != 1 || (K != 128 && K != 256) || N < 128 || N > 1024 || (N % 128) != 0) return 0;      // pairs of 64 columns, two in flight
    return (size_t)N * K * 6;
}
static bool rowpanel_applies(const KCParams& p) {
    if (!pa2d_env().lin_rowpanel || p.io_bf16) return false;
    if (rowpanel_image_bytes(p.N, p.K, p.engine) == 0) return false;
    if (persistent_mode(p) < 0 || (p.epi == EPI_ACT && p.aux)) return false;
    // 16-byte loads / stores of accumulator quads: every leading dimension a multiple of 4 elements
    if ((p.lda & 3) || (p.ldc & 3) || (p.res && (p.ldres & 3)) || (p.aux && (p.ldaux & 3))) return false;
    return p.M / 128 >= 256;                                     // at least one round per CU
}
// the halo-in-LDS conv.  PA2D_CONV_HALO=off|auto|force: 0 = never, 1 = when the launch fills the chip (default), 2 = always (tests)
static bool conv_halo_applies(const KCParams& p) {
    const int pol = pa2d_env().conv_halo;
    if (p.taps == 27) return false;      // 3x3 halo only: the 3x3x3 conv never comes here
    if (pol == 0 || !p.apre || (p.Cin % 32) != 0 || p.H <= 0 || p.W <= 0 || (p.M % (p.H * p.W)) != 0) return false;
    const long long tiles = (long long)(p.M / (p.H * p.W)) * ceil_div(p.H, KC_HALO_TH) * ceil_div(p.W, KC_HALO_TW) * ceil_div(p.N, 128);
    return pol == 2 || tiles >= 512;
}

KCChoice plan_kc(const KCParams& p, bool im2col) {
    KCChoice c = {};
    c.mode = c.tail_family = c.tail_bm = c.tail_bn = -1;
    c.out_bf16 = p.io_bf16;
    c.reads_b = true;
    c.wimg_bytes = im2col ? 0 : rowpanel_image_bytes(p.N, p.K, p.engine);
    const int nt = p.engine == 2 ? 1 : 3;
    if (!im2col && p.wimg && rowpanel_applies(p)) {
        c.family = KC_ROWPANEL; c.bm = 128; c.bn = 64; c.bk = 64; c.nt = 3;
    } else if (panel_applies(p, im2col)) {
        c.family = KC_PANEL; c.bm = 256; c.bn = 128; c.bk = 32; c.nt = nt;
    } else if (p.io_bf16 || use_split(p.engine, p.N, im2col, p.Cin)) {
        // the bf16 engines' per-tile kernels: the conv on plane images (bf16 storage: the tensor itself, also at the narrow
        // shapes the fp32-I/O engines hand to the exact kernel), the plain GEMMs of engine 2 converting while they stage
        c.family = KC_SPLIT; c.bm = 128; c.bn = 128; c.bk = 32; c.nt = nt;
        c.a_planes = im2col ? p.apre != 0 : p.io_bf16 != 0;
        if (im2col) c.pack = KC_PACK_PLANES;
        if (im2col ? !p.apre : p.engine != 2) c.rc = PA2D_ERR_ARG;
        else if (p.io_bf16 && (p.taps == 27 || p.engine != 2 || (!im2col && (p.K % 32) != 0))) c.rc = PA2D_ERR_UNSUPPORTED;
        else if (im2col && conv_halo_applies(p)) {
            c.family = KC_HALO; c.bm = 256;
            c.mfma16 = nt == 3 && pa2d_env().conv_mfma16 && (p.N % 4) == 0 && (p.ldc % 4) == 0;      // 16-byte stores of accumulator quads
            c.ahead = c.mfma16 && pa2d_env().conv_ahead;
        } else if (im2col && !p.io_bf16 && nt == 3) {
            // tile ladder of the split conv, 9 and 27 taps.  256x128 (128x64 per consumer wave): 25 % less L2->LDS staging and
            // LDS reads per MFMA; 64x128 for small launches (rollout at batch 1: 32 x 4 tiles of 128 x 128 leave half of the
            // 256 CUs idle)
            const int tiles_n = ceil_div(p.N, 128);
            if (pa2d_env().split_big && (p.M % 256) == 0 && (long long)(p.M / 256) * tiles_n >= 512) c.bm = 256;
            else if ((long long)ceil_div(p.M, 128) * tiles_n < 256) c.bm = 64;
        }
    } else if (kc_split_small_applies(p, im2col)) {
        c.family = KC_SPLIT_SMALL; c.bm = 64; c.bn = 64; c.bk = 32; c.nt = 3;
    } else {
        const KCTile t = kc_tile(p.M, p.N, im2col, p.Cin);
        c.family = KC_EXACT; c.bm = t.bm; c.bn = t.bn; c.bk = t.bk;
        if (im2col) c.pack = t.bk == 32 ? KC_PACK_F32_32 : KC_PACK_F32_16;
    }
    if (c.family == KC_PANEL || c.family == KC_ROWPANEL) {
        // the whole bm-row blocks; the tail is planned on the TAIL's rows, without an image
        c.mode = persistent_mode(p);
        c.head_rows = p.M - p.M % c.bm;
        if (c.head_rows < p.M) {
            KCParams pt = p;
            pt.wimg = nullptr;
            pt.M = p.M - c.head_rows;
            const KCChoice t = plan_kc(pt, false);
            c.tail_family = t.family; c.tail_bm = t.bm; c.tail_bn = t.bn;
        }
        c.reads_b = c.family == KC_PANEL || c.head_rows < p.M;
    }
    return c;
}

// Every 32-bit extent of the buffer descriptors, from the choice; false: one does not fit.  A and B are held to their fp32
// extent whatever they hold (the answer of an oversized call does not depend on the engine), then described as what the
// kernel reads: bf16 storage, plane images, the planes pack.
static bool kc_extents(KCParams& p, bool im2col, const KCChoice& c) {
    const unsigned long long lim = 0xFFFFFFF0ull;
    const unsigned long long es = p.io_bf16 ? 2ull : 4ull;      // storage size of C / res / aux
    unsigned long long ab = ((unsigned long long)(p.M - 1) * p.lda + (im2col ? p.Cin : p.K)) * 4ull;
    unsigned long long bb = ((unsigned long long)(p.N - 1) * p.ldb + p.K) * 4ull;
    const unsigned long long cb = ((unsigned long long)(p.M - 1) * p.ldc + p.N) * es;
    const unsigned long long rb = p.res ? ((unsigned long long)(p.M - 1) * p.ldres + p.N) * es : 0ull;
    const unsigned long long xb = p.aux ? ((unsigned long long)(p.M - 1) * p.ldaux + p.N) * es : 0ull;
    if (ab >= lim || bb >= lim || cb >= lim || rb >= lim || xb >= lim) return false;
    if (c.a_planes) ab = im2col ? (unsigned long long)p.M * (p.Cin / 32) * c.nt * 64 : ab / 2;      // planes : a bf16 matrix
    if (c.pack == KC_PACK_PLANES) bb = (unsigned long long)p.N * (p.K / 32) * c.nt * 64;            // (<= 1.5 x the fp32 pack)
    if (ab >= lim) return false;
    p.a_bytes = (unsigned)ab; p.b_bytes = (unsigned)bb;
    p.c_bytes = (unsigned)cb; p.res_bytes = (unsigned)rb; p.aux_bytes = (unsigned)xb;
    return true;
}

// The whole bm-row blocks on the persistent kernel, the (< bm-row) tail on the per-tile kernel plan_kc picks for it.  The
// tail starts from the caller's parameters: no image, fresh extents, its own bias_split fix-up.
static int launch_head_tail(const KCParams& p_in, const KCParams& p, const KCChoice& c, hipStream_t st) {
    int rc;
    if (c.family == KC_ROWPANEL && p.wsrc) {      // NULL: the caller made the image (pa2d_gemm_weight_image) while the weights stand still
        rc = launch_pack_weight_image(p.wsrc, p.wsn, p.wsk, p.wimg, p.N, p.K, st);
        if (rc) return rc;
    }
    KCParams ph = p;
    ph.M = c.head_rows;
    rc = c.family == KC_ROWPANEL ? launch_kc_rowpanel(ph, c, st) : launch_kc_panel(ph, c, st);
    if (rc || c.head_rows == p.M) return rc;
    KCParams pt = p_in;
    pt.wimg = nullptr;
    pt.M = p.M - c.head_rows;
    pt.A = p.A + (size_t)c.head_rows * p.lda;
    pt.C = p.C + (size_t)c.head_rows * p.ldc;
    if (p.res) pt.res = p.res + (size_t)c.head_rows * p.ldres;
    if (p.aux) pt.aux = p.aux + (size_t)c.head_rows * p.ldaux;
    return launch_kc(pt, false, st);
}

int launch_kc(const KCParams& p_in, bool im2col, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    KCParams p = p_in;
    if (!engine_ok(p.engine)) return PA2D_ERR_ARG;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return PA2D_OK;
    if (!p.bias2) p.bias_split = 0x7fffffff;
    const KCChoice c = plan_kc(p, im2col);
    if (!kc_extents(p, im2col, c)) return PA2D_ERR_UNSUPPORTED;      // 32-bit byte offsets inside the buffer descriptors
    if ((p.K & 3) || (p.lda & 3) || (p.ldb & 3)) return PA2D_ERR_ARG;
    if (im2col && ((p.Cin & 15) || p.K != (p.taps == 27 ? 27 : 9) * p.Cin)) return PA2D_ERR_UNSUPPORTED;
    if (im2col && (p.epi != 0 || p.res)) return PA2D_ERR_ARG;      // conv kernels carry the bias-only epilogue
    if (ev0 && hipEventRecord(ev0, st) != hipSuccess) return PA2D_ERR_ARG;
    if (c.rc) return c.rc;
    int rc;
    switch (c.family) {
        case KC_ROWPANEL:
        case KC_PANEL: rc = launch_head_tail(p_in, p, c, st); break;
        case KC_HALO: rc = launch_conv_halo(p, c, st); break;
        case KC_SPLIT:
        case KC_SPLIT_SMALL: rc = launch_kc_split(p, im2col, c, st); break;
        default: rc = launch_kc_f32(p, im2col, KCTile{c.bm, c.bn, c.bk}, st);
    }
    if (rc) return rc;
    if (ev1 && hipEventRecord(ev1, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

// ---------------------------------------------------------------------------------------------
// weight re-layouts (tiny; weights change every optimizer step so they are redone per call)
// mode 0: plain transpose  dst[k][n] = src[n][k]                                  (linear bwd-data)
// mode 1: conv fwd pack    dst[co'][cic][tap][c16] = W_{co'<C ? x : f}[co][cic*16+c16][tap]       ([2C][9*Cin])
// mode 2: conv bwd pack    dst[ci][cic'][tap'][c16] = W_{..}[co = cic'*16+c16][ci][8 - tap']        ([Cin][9*2C])
//         (K order of gemm_kc's implicit GEMM: 16-channel chunk outer, tap inner)
// TAPS = 27: modes 1 / 2 for the [C,C,3,3,3] kernels of the 3x3x3 conv (taps flipped as 26 - tap)
// NK = kernels in the pack: 2 = the pair [Wx | Wf]; 1 = no second kernel (pa2d_conv3x3_*: w1 is never read)
template <int TAPS>
__global__ void repack_kernel(const float* __restrict__ w0, const float* __restrict__ w1, float* __restrict__ dst,
                              int mode, int N, int K, int C, int Cin, int NK) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 0) {
        if (idx >= (long long)N * K) return;
        const int n = (int)(idx % N), k = (int)(idx / N);
        dst[idx] = w0[(size_t)n * K + k];
    } else if (mode == 1) {
        if (idx >= (long long)NK * C * TAPS * Cin) return;
        const int CH = K;      // channels per K-step (16 for the f32 engine, 32 for the split engine)
        const int c16 = (int)(idx % CH);
        const int tap = (int)((idx / CH) % TAPS);
        const int cic = (int)((idx / (TAPS * CH)) % (Cin / CH));
        const int co = (int)(idx / ((long long)Cin * TAPS));
        const int ci = cic * CH + c16;
        const float* src = co < C ? w0 : w1;
        dst[idx] = src[((size_t)(co % C) * Cin + ci) * TAPS + tap];
    } else {
        if (idx >= (long long)NK * C * TAPS * Cin) return;
        const int CH = K;
        const int c16 = (int)(idx % CH);
        const int tap = (int)((idx / CH) % TAPS);
        const int cic = (int)((idx / (TAPS * CH)) % (NK * C / CH));
        const int ci = (int)(idx / ((long long)NK * C * TAPS));
        const int co = cic * CH + c16;
        const float* src = co < C ? w0 : w1;
        dst[idx] = src[((size_t)(co % C) * Cin + ci) * TAPS + (TAPS - 1 - tap)];
    }
}

int launch_repack(const float* w0, const float* w1, float* dst, int mode, int N, int K, int C, int Cin, hipStream_t st,
                  int taps) {
    const int nk = w1 ? 2 : 1;
    const long long count = mode == 0 ? (long long)N * K : (long long)nk * C * taps * Cin;
    const dim3 grid((unsigned)ceil_div_ll(count, 256));
    if (taps == 27)
        hipLaunchKernelGGL(repack_kernel<27>, grid, dim3(256), 0, st, w0, w1, dst, mode, N, K, C, Cin, nk);
    else
        hipLaunchKernelGGL(repack_kernel<9>, grid, dim3(256), 0, st, w0, w1, dst, mode, N, K, C, Cin, nk);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// KCParams of y = act(x . w^T + bias) (+ res), pre = the pre-activation (or its derivative, PA2D_ACT_SAVE_DERIVATIVE_BIT);
// io_bf16: x, res, y, pre are bf16 (always the bf16 engine)
static KCParams dense_fwd_params(const void* x, long long ldx, const float* w, long long ldw, const float* bias,
                                 const void* res, long long ldres, void* y, long long ldy, void* pre, long long ldpre, int M,
                                 int N, int K, int act, int engine, bool io_bf16) {
    KCParams p = {};
    p.engine = engine; p.io_bf16 = io_bf16 ? 1 : 0; p.apre = io_bf16 ? 1 : 0;
    p.aux_deriv = (act & PA2D_ACT_SAVE_DERIVATIVE_BIT) ? 1 : 0;
    act &= ~PA2D_ACT_SAVE_DERIVATIVE_BIT;
    p.A = (const float*)x; p.lda = ldx; p.B = w; p.ldb = ldw; p.C = (float*)y; p.ldc = ldy; p.bias = bias;
    p.res = (const float*)res; p.ldres = ldres; p.aux = (float*)pre; p.ldaux = ldpre; p.M = M; p.N = N; p.K = K; p.act = act;
    p.epi = (act != ACT_NONE ? EPI_ACT : 0) | (pre ? EPI_STORE_PRE : 0);
    return p;
}
// KCParams of dx[M,K] = (dy[M,N] . w[N,K]) * act'(pre[M,K]) on the transposed weight wt[K][N]
static KCParams dense_bwd_data_params(const void* dy, long long lddy, const float* wt, const void* pre, long long ldpre,
                                      int act, void* dx, long long lddx, int M, int N, int K, int engine, bool io_bf16) {
    KCParams p = {};
    p.engine = engine; p.io_bf16 = io_bf16 ? 1 : 0; p.apre = io_bf16 ? 1 : 0;
    p.aux_deriv = (act & PA2D_ACT_SAVE_DERIVATIVE_BIT) ? 1 : 0;
    act &= ~PA2D_ACT_SAVE_DERIVATIVE_BIT;
    p.A = (const float*)dy; p.lda = lddy; p.B = wt; p.ldb = N; p.C = (float*)dx; p.ldc = lddx; p.M = M; p.N = K; p.K = N;
    p.aux = (float*)const_cast<void*>(pre); p.ldaux = ldpre; p.act = act;
    p.epi = (pre && act != ACT_NONE) ? EPI_MUL_DACT : 0;
    return p;
}

// =============================================================================================
// C ABI (declared in include/pa2d.h)
extern "C" {

// The engine a caller should use when it has no preference: env PA2D_GEMM=f32|split|bf16, else the fp32-accurate
// split engine.  A pure function of the environment — nothing in the library reads it implicitly.
int pa2d_default_engine(void) { return pa2d_env().default_engine; }

void pa2d_reload_env(void) { g_env = read_env(); }

// bytes of scratch with which the forward / data-gradient linears of an [N, K] weight take their fastest kernel under
// `engine` (split engine, K in {128, 256}, N % 64 == 0: the row-stationary kernel's weight plane image); the calls
// work with less (data gradient: at least K*N floats for the transposed weight) on the other kernels
static size_t weight_image_bytes(int N, int K, int engine) {
    KCParams p = {};
    p.N = N; p.K = K; p.engine = engine;
    return plan_kc(p, false).wimg_bytes;
}
size_t pa2d_gemm_fwd_workspace(int N, int K, int engine) { return weight_image_bytes(N, K, engine); }
size_t pa2d_gemm_bwd_data_workspace(int N, int K, int engine) {
    return (size_t)N * K * sizeof(float) + weight_image_bytes(K, N, engine);
}

// The weight plane image on its own: callers that know the weights stand still over several calls (the model calls and
// the backward pass of one training iteration, a rollout) make it once and pass it as `wimg`.  transposed = 0: the image of
// w[N, K] for the forward of that layer; 1: the image of w^T for its data gradient (N = the layer's input width, K = its
// output width, w stored [K, N] with row pitch ldw).  img_bytes >= pa2d_gemm_fwd_workspace(N, K, engine) > 0.
int pa2d_gemm_weight_image(const float* w, long long ldw, int transposed, void* img, size_t img_bytes, int N, int K,
                           int engine, hipStream_t st) {
    const size_t need = weight_image_bytes(N, K, engine);
    if (need == 0) return PA2D_ERR_UNSUPPORTED;
    if (!img || img_bytes < need) return PA2D_ERR_WORKSPACE;
    return transposed ? launch_pack_weight_image(w, 1, ldw, img, N, K, st) : launch_pack_weight_image(w, ldw, 1, img, N, K, st);
}

int pa2d_gemm_bias_act_fwd(const float* x, long long ldx, const float* w, long long ldw, const float* bias,
                           const float* res, long long ldres, float* y, long long ldy, float* pre, long long ldpre,
                           const void* wimg, void* ws, size_t ws_bytes, int M, int N, int K, int act, int engine,
                           hipStream_t st) {
    KCParams p = dense_fwd_params(x, ldx, w, ldw, bias, res, ldres, y, ldy, pre, ldpre, M, N, K, act, engine, false);
    const size_t img = plan_kc(p, false).wimg_bytes;
    if (img && wimg) p.wimg = const_cast<void*>(wimg);      // ready-made (p.wsrc stays NULL: nothing to pack)
    else if (ws && img && ws_bytes >= img) { p.wimg = ws; p.wsrc = w; p.wsn = ldw; p.wsk = 1; }
    return launch_kc(p, false, st);
}

// dx[M,K] = (dy[M,N] . w[N,K]) * act'(pre[M,K])   (pre may be NULL -> plain product)
// ws: at least K*N floats (the transposed weight of the per-tile kernels); pa2d_gemm_bwd_data_workspace(N, K, engine)
// bytes let the split engine's row-stationary kernel run: [transposed weight | weight plane image].
int pa2d_gemm_bwd_data(const float* dy, long long lddy, const float* w, long long ldw, const float* pre,
                       long long ldpre, int act, float* dx, long long lddx, const void* wimg, void* ws, size_t ws_bytes, int M,
                       int N, int K, int engine, hipStream_t st) {
    if (ldw != K) return PA2D_ERR_ARG;
    if (N & 3) return PA2D_ERR_ARG;
    if (M <= 0) return PA2D_OK;
    if (ws_bytes < (size_t)N * K * sizeof(float)) return PA2D_ERR_WORKSPACE;
    float* const wt_ws = (float*)ws;
    KCParams p = dense_bwd_data_params(dy, lddy, wt_ws, pre, ldpre, act, dx, lddx, M, N, K, engine, false);
    const size_t img = plan_kc(p, false).wimg_bytes;
    if (img && wimg) p.wimg = const_cast<void*>(wimg);      // ready-made image of w^T (pa2d_gemm_weight_image, transposed = 1)
    else if (img && ws_bytes >= (size_t)N * K * sizeof(float) + img) {
        p.wimg = (char*)ws + (size_t)N * K * sizeof(float); p.wsrc = w; p.wsn = 1; p.wsk = ldw;
    }
    if (plan_kc(p, false).reads_b) {      // someone reads the fp32 transpose
        const int rc = launch_repack(w, nullptr, wt_ws, 0, N, K, 0, 0, st);
        if (rc) return rc;
    }
    return launch_kc(p, false, st);
}

// Diagnostic: the KCChoice of a forward / data-gradient GEMM, asked for as the entry points ask for it (contiguous operands;
// bf16 storage implies engine 2).  kind 0 / 1: the linear y[M,N] = x[M,K] . w[N,K]^T / its data gradient, (d0, d1, d2) = (M, N, K);
// kind 2 / 3: the conv on [B, H, W, depth, C] / its data gradient, (d0, d1, d2) = (B, H, W), nk kernels stacked, taps 9 | 27.
// epi (linears): 1 = bias, 2 = residual, 4 = pre-activation stored (forward) / supplied (data gradient), 8 = an output pitch
// that is no multiple of 4.  image: weight-image scratch is on offer.  out[PA2D_ROUTE_FIELDS]: rc, family, bm, bn, bk, nt,
// mfma16, ahead, out_bf16, mode, head_rows, tail family / bm / bn, a_planes, pack, reads_b, wimg_bytes (see KCChoice).
int pa2d_gemm_route(int kind, int d0, int d1, int d2, int depth, int C, int nk, int taps, int act, int epi, int engine,
                    int bf16_storage, int image, int* out) {
    static char mark;      // stands for every pointer that is "there": plan_kc looks at null-ness only
    if (!out || kind < 0 || kind > 3 || !engine_ok(engine)) return PA2D_ERR_ARG;
    const bool bf = bf16_storage != 0;
    if (bf) engine = 2;
    KCParams p;
    if (kind <= 1) {
        const int M = d0, N = d1, K = d2, pad = (epi & 8) ? 2 : 0;
        const void* const bias = (epi & 1) ? &mark : nullptr;
        const void* const res = (epi & 2) ? &mark : nullptr;
        void* const pre = (epi & 4) ? &mark : nullptr;
        if (kind == 0) p = dense_fwd_params(&mark, K, (const float*)&mark, K, (const float*)bias, res, N, &mark, N + pad, pre, N, M, N, K, act, engine, bf);
        else p = dense_bwd_data_params(&mark, N, (const float*)&mark, pre, K, act, &mark, K + pad, M, N, K, engine, bf);
        if (image && plan_kc(p, false).wimg_bytes) p.wimg = &mark;
    } else {
        const int NC = nk * C;
        p = kc_conv_shape(engine, bf, d0 * d1 * d2 * depth, kind == 2 ? NC : C, kind == 2 ? C : NC, taps, d1, d2, depth);
    }
    const KCChoice c = plan_kc(p, kind >= 2);
    const int v[PA2D_ROUTE_FIELDS] = {c.rc, c.family, c.bm, c.bn, c.bk, c.nt, c.mfma16, c.ahead, c.out_bf16, c.mode, c.head_rows,
                                      c.tail_family, c.tail_bm, c.tail_bn, c.a_planes, c.pack, c.reads_b, (int)c.wimg_bytes};
    memcpy(out, v, sizeof(v));
    return PA2D_OK;
}

// dw[N,K] = dy[M,N]^T . x[M,K] as the weight-gradient dispatch sees it
static MCDesc linear_wgrad(const void* dy, long long lddy, const void* x, long long ldx, int M, int N, int K, MCSrc src,
                           int engine) {
    MCDesc d = {};
    d.A = dy; d.lda = lddy; d.B = x; d.ldb = ldx; d.Mi = N; d.Nj = K; d.Mk = M;
    d.taps = 1; d.H = 1; d.W = 1; d.depth = 1; d.Cin = K; d.src = src; d.engine = engine;
    return d;
}

size_t pa2d_gemm_bwd_weight_workspace(int M, int N, int K, int engine) {
    const MCChoice c = plan_wgrad(linear_wgrad(nullptr, N, nullptr, K, M, N, K, MC_SRC_F32, engine));
    return c.slab_bytes + (size_t)c.pl.splits * N * sizeof(float);      // [slabs | per-split column sums of dy]
}

// dw[N,K] (+)= dy[M,N]^T . x[M,K] ; db[N] (+)= column sums of dy (db may be NULL).  accumulate != 0: add to what dw / db
// hold (gradient accumulation straight into the caller's bucket, done inside the slab-reduce pass).
int pa2d_gemm_bwd_weight(const float* dy, long long lddy, const float* x, long long ldx, float* dw, float* db,
                         void* ws, size_t ws_bytes, int M, int N, int K, int accumulate, int engine, hipStream_t st) {
    if (!engine_ok(engine)) return PA2D_ERR_ARG;
    if (M <= 0) {
        if (accumulate) return PA2D_OK;
        const int rz = pa2d_zero(dw, sizeof(float) * N * K, st);
        return rz ? rz : pa2d_zero(db, sizeof(float) * N, st);
    }
    if (ws_bytes < pa2d_gemm_bwd_weight_workspace(M, N, K, engine)) return PA2D_ERR_WORKSPACE;
    MCDesc d = linear_wgrad(dy, lddy, x, ldx, M, N, K, MC_SRC_F32, engine);
    const MCChoice c = plan_wgrad(d);
    const MCPlan& pl = c.pl;
    // the bias gradient (column sums of dy) rides in the GEMM: the workgroups of column tile 0 sum the dy tiles they stage
    float* cs = db ? (float*)ws + pl.slab_floats : nullptr;
    d.colsum = cs;
    int rc = launch_wgrad(d, c, (float*)ws, st);
    if (rc) return rc;
    rc = launch_reduce((const float*)ws, pl.splits, (long long)N * K, dw, nullptr, 0, 0, 0, st, accumulate);
    if (rc) return rc;
    if (db) rc = launch_reduce(cs, pl.splits, N, db, nullptr, 0, 0, 0, st, accumulate);
    return rc;
}

// =============================================================================================
// bf16-STORAGE variants (BASELINE configs[2] / [4] as stated): activations, saved tensors and inter-kernel gradients are
// bf16 in HBM; weights, biases and every parameter gradient stay fp32; all products are ONE bf16 MFMA term with fp32
// accumulation (the arithmetic of PA2D_ENGINE_BF16, minus its fp32 round trips: a bf16 tensor IS the 1-plane operand
// image the bf16 kernels stage, so the activation pre-passes disappear).  ld* are in ELEMENTS.  Requires K % 32 == 0
// (PA2D_ERR_UNSUPPORTED otherwise, never a silent fallback).  The conv of this family is in pa2d_conv.hip.

int pa2d_gemm_bias_act_fwd_bf16(const void* x, long long ldx, const float* w, long long ldw, const float* bias,
                                const void* res, long long ldres, void* y, long long ldy, void* pre, long long ldpre,
                                int M, int N, int K, int act, hipStream_t st) {
    return launch_kc(dense_fwd_params(x, ldx, w, ldw, bias, res, ldres, y, ldy, pre, ldpre, M, N, K, act, 2, true), false, st);
}

// dx[M,K] = (dy[M,N] . w[N,K]) * act'(pre[M,K]); dy, pre, dx bf16; w fp32; wt_ws: K*N floats (transposed weight)
int pa2d_gemm_bwd_data_bf16(const void* dy, long long lddy, const float* w, long long ldw, const void* pre,
                            long long ldpre, int act, void* dx, long long lddx, float* wt_ws, int M, int N, int K,
                            hipStream_t st) {
    if (ldw != K) return PA2D_ERR_ARG;
    if (N & 3) return PA2D_ERR_ARG;
    if (M <= 0) return PA2D_OK;
    int rc = launch_repack(w, nullptr, wt_ws, 0, N, K, 0, 0, st);
    if (rc) return rc;
    return launch_kc(dense_bwd_data_params(dy, lddy, wt_ws, pre, ldpre, act, dx, lddx, M, N, K, 2, true), false, st);
}

size_t pa2d_gemm_bwd_weight_workspace_bf16(int M, int N, int K) {
    const MCChoice c = plan_wgrad(linear_wgrad(nullptr, N, nullptr, K, M, N, K, MC_SRC_BF16, 2));
    const size_t b = (size_t)colsum_blocks(M) * N * sizeof(float);      // the column-sum partials reuse the slabs' space
    return c.slab_bytes > b ? c.slab_bytes : b;
}

// dw[N,K] (+)= dy[M,N]^T . x[M,K] (fp32), db[N] (+)= column sums of dy; dy, x bf16 and CONTIGUOUS (lddy == N, ldx == K)
int pa2d_gemm_bwd_weight_bf16(const void* dy, long long lddy, const void* x, long long ldx, float* dw, float* db,
                              void* ws, size_t ws_bytes, int M, int N, int K, int accumulate, hipStream_t st) {
    if (lddy != N || ldx != K) return PA2D_ERR_ARG;
    if ((N & 31) || (K & 31)) return PA2D_ERR_UNSUPPORTED;
    if (M <= 0) {
        if (accumulate) return PA2D_OK;
        const int rz = pa2d_zero(dw, sizeof(float) * N * K, st);
        return rz ? rz : pa2d_zero(db, sizeof(float) * N, st);
    }
    if (ws_bytes < pa2d_gemm_bwd_weight_workspace_bf16(M, N, K)) return PA2D_ERR_WORKSPACE;
    const MCDesc d = linear_wgrad(dy, lddy, x, ldx, M, N, K, MC_SRC_BF16, 2);
    const MCChoice c = plan_wgrad(d);
    const MCPlan& pl = c.pl;
    int rc = launch_wgrad(d, c, (float*)ws, st);
    if (rc) return rc;
    rc = launch_reduce((const float*)ws, pl.splits, (long long)N * K, dw, nullptr, 0, 0, 0, st, accumulate);
    if (rc) return rc;
    if (db) rc = launch_colsum_bf16(dy, lddy, M, N, db, (float*)ws, st, nullptr, 0, accumulate);
    return rc;
}

}  // extern "C"
