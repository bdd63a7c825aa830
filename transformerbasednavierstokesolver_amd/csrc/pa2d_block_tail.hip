// Fused block tail for no-grad forwards — gfx950 / CDNA4.  ONE launch computes, for a panel of rows per workgroup,
//   y   = deslice(x_mid, o[b], Ws, bs, temperature)            (Physics_Attention.py:116-117)
//   a   = y . Wo^T + bo + fx                                    (to_out + residual, :119; …_2D.py:70)
//   h   = act(LN(a; g2, be2) . W1^T + b1)                       (ln_2, MLP linear_pre, …_2D.py:71)
//   out = h . W2^T + b2 + a                                     (MLP linear_post + residual)
//   xn  = LN(out; gn, bn)                                       (the next block's ln_1, or ln_3; optional)
// what the default path runs as six launches (pa2d_deslice_fwd, 3 x pa2d_gemm_bias_act_fwd, 2 x pa2d_layernorm_fwd) with
// five HBM round trips of a [B N, C] or [B N, r C] tensor.  Every stage is row-local, so workgroups are independent: a
// plain launch, no flags, no grid barrier.
//
// Engine: PA2D_ENGINE_SPLIT only (exact 3-plane bf16 splits of both operands, the six terms i + j <= 2 on
// v_mfma_f32_16x16x32_bf16, fp32 accumulation; pa2d_bf16_split.h).  The other engines are refused, never emulated.
//
// A workgroup is 8 waves and owns P = 16 PT rows (PT = 1, 2).  LDS (dynamic):
//   fbuf  float [P][C + 4]          a, then out (the residual stream of the panel)
//   pl1   bf16 [3][P][C + 8]        operand planes: y, then LN2(a)
//   pl2   bf16 [3][P][C + 8]        operand planes: one C-wide chunk of h
// = P (16 C + 112) bytes: 134,656 at P = 32, C = 256.  hidden = r C is walked in r chunks of C columns: fc1 makes a chunk
// of h in pl2, fc2 adds its contribution to accumulators that stay in registers, so h never exists whole.
//
// All three GEMMs are computed TRANSPOSED, out^T = W . X^T: the weight tile is the A operand (row li = output column), the
// panel is the B operand (column li = panel row), and the result has column li = panel row, rows 4 kq + r = four CONSECUTIVE
// output columns: every epilogue is float4 / 8-byte-plane traffic for one row.  The weights are read from a fragment-order
// image made once per weight (pa2d_block_tail_weight_image): [N / 16][K / 32][3 planes][64 lanes][8 bf16], one coalesced
// 16-byte load per lane and plane, no split arithmetic per workgroup.
//
// De-slice (one wave per (head, 16-row tile)): T-layout as pa2d_slice3.hip — logits^T = Ws . X_h^T puts the M weights of a
// point in one lane column (softmax = in-lane + two cross-group steps) and they ARE the B operand of Y^T = O^T . W^T.  `o`
// is per sample: a tile whose rows belong to several samples runs the second product once per sample and every lane keeps
// the result of its own row's sample.
#include "pa2d_slice_common.h"
#include "pa2d_bf16_split.h"

namespace {

constexpr int TAIL_WAVES = 8, TAIL_THREADS = 64 * TAIL_WAVES;
constexpr int FPAD = 4, PPAD = 8;
constexpr int TILE_IMG = 3 * 1024;      // bytes of one (16 x 32) weight tile: 3 planes x 64 lanes x 16 bytes

struct TailParams {
    const float* xm; long long ldx;
    const float* o; const float* ws; const float* bs; const float* temperature;
    const float* fx; long long ldfx;
    const float* bo; const float* g2; const float* be2; const float* b1; const float* b2; const float* gn; const float* bn;
    const unsigned char* img_o; const unsigned char* img_1; const unsigned char* img_2;
    float* out; float* xn; float* y_dbg; float* a_dbg; float* h_dbg;
    int R, N, heads, D, M, C, hidden, act, clamp;
    float eps;
};

__device__ __forceinline__ f32x8 load8(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    return (f32x8){a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
__device__ __forceinline__ void store_planes4(unsigned char* pl, unsigned plane_bytes, unsigned off, float4 v) {
    bf16x4 hi, mid, lo;
    split3(v, hi, mid, lo);
    *reinterpret_cast<bf16x4*>(pl + off) = hi;
    *reinterpret_cast<bf16x4*>(pl + plane_bytes + off) = mid;
    *reinterpret_cast<bf16x4*>(pl + 2 * plane_bytes + off) = lo;
}

// acc[i][rt] += W tile (nt0 + 8 i, image k-steps s0 .. s0 + sn - 1) . planes[rows of tile rt][k-steps 0 .. sn - 1], i = 0, 1: the
// wave's two column tiles together — one read of the panel fragments serves both, and 2 PT independent accumulator chains
// keep the matrix pipe busy between the dependent MFMAs of one chain.  The weight fragments of k-step s + 1 are loaded
// before the MFMAs of k-step s (their L2 latency hides behind 12 PT MFMAs).  two = false: the second tile does not exist.
template <int PT>
__device__ __forceinline__ void gemm_pair(f32x4 (&acc)[2][PT], bool two, const unsigned char* pl, unsigned plane_bytes, int PP,
                                          const unsigned char* img, int ks_total, int nt0, int s0, int sn, int lane) {
    const int li = lane & 15, kq = lane >> 4;
    const unsigned char* ib0 = img + ((size_t)nt0 * ks_total + s0) * TILE_IMG + lane * 16;
    const unsigned char* ib1 = two ? ib0 + (size_t)TAIL_WAVES * ks_total * TILE_IMG : ib0;
    const unsigned char* ab = pl + (li * PP + 8 * kq) * 2;
    bf16x8 wf[2][3], wn[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        wf[0][q] = *reinterpret_cast<const bf16x8*>(ib0 + q * 1024);
        wf[1][q] = *reinterpret_cast<const bf16x8*>(ib1 + q * 1024);
    }
    for (int s = 0; s < sn; ++s) {
        const size_t nx = (size_t)(s + 1 < sn ? s + 1 : s) * TILE_IMG;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            wn[0][q] = *reinterpret_cast<const bf16x8*>(ib0 + nx + q * 1024);
            wn[1][q] = *reinterpret_cast<const bf16x8*>(ib1 + nx + q * 1024);
        }
#pragma unroll
        for (int rt = 0; rt < PT; ++rt) {
            bf16x8 xf[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                xf[q] = *reinterpret_cast<const bf16x8*>(ab + q * plane_bytes + rt * 16 * PP * 2 + s * 64);
            acc[0][rt] = mfma_terms<3, 3>(wf[0], xf, acc[0][rt]);
            if (two) acc[1][rt] = mfma_terms<3, 3>(wf[1], xf, acc[1][rt]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) { wf[0][q] = wn[0][q]; wf[1][q] = wn[1][q]; }
    }
}

// LayerNorm of the P rows of fbuf, one wave per row, lane = 4 consecutive columns; the result goes to operand planes
// (pl != nullptr) or to global rows (dst, rows below rows_left only)
template <int PT>
__device__ __forceinline__ void ln_rows(const float* fbuf, int C, const float* gamma, const float* beta, float eps,
                                        unsigned char* pl, unsigned plane_bytes, float* dst, int rows_left) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, FP = C + FPAD, PP = C + PPAD;
    const bool on = 4 * lane < C;
    const float invC = 1.0f / (float)C;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), be = g;
    if (on) { g = *reinterpret_cast<const float4*>(gamma + 4 * lane); be = *reinterpret_cast<const float4*>(beta + 4 * lane); }
    for (int row = wave; row < 16 * PT; row += TAIL_WAVES) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) v = *reinterpret_cast<const float4*>(fbuf + row * FP + 4 * lane);
        const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * invC;
        float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
        if (!on) d = make_float4(0.f, 0.f, 0.f, 0.f);
        const float var = wave_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * invC;
        const float rstd = 1.0f / sqrtf(var + eps);
        const float4 y = make_float4(fmaf(d.x * rstd, g.x, be.x), fmaf(d.y * rstd, g.y, be.y), fmaf(d.z * rstd, g.z, be.z),
                                     fmaf(d.w * rstd, g.w, be.w));
        if (on) {
            if (pl) store_planes4(pl, plane_bytes, (unsigned)(row * PP + 4 * lane) * 2, y);
            else if (row < rows_left) *reinterpret_cast<float4*>(dst + (size_t)row * C + 4 * lane) = y;
        }
    }
}

template <int PT>
__global__ __launch_bounds__(TAIL_THREADS, 1) void block_tail_kernel(const TailParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = 16 * PT;
    const int C = p.C, FP = C + FPAD, PP = C + PPAD, R = p.R;
    float* fbuf = reinterpret_cast<float*>(smem);
    const unsigned plane_bytes = (unsigned)(P * PP * 2);
    unsigned char* pl1 = smem + (size_t)P * FP * 4;
    unsigned char* pl2 = pl1 + 3 * plane_bytes;
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4, wave = threadIdx.x >> 6;
    const int row0 = (int)blockIdx.x * P;              // first row of the panel (R < 2^31 / 4: extents are checked)
    const int ctiles = C >> 4, cks = C >> 5;

    // ---- stage 0: de-slice -> planes of y in pl1
    {
        const int D = p.D, M = p.M, mtn = (M + 15) >> 4, kst = (D + 31) >> 5, dtn = (D + 15) >> 4, mun = (mtn + 1) >> 1;
        for (int item = wave; item < p.heads * PT; item += TAIL_WAVES) {
            const int h = item / PT, rt = item % PT;
            const int g0 = row0 + 16 * rt;
            if (g0 >= R) continue;                      // no row of this tile exists; its planes are never stored from
            const int myrow = min(g0 + li, R - 1), myb = myrow / p.N;
            const float* xr = p.xm + (size_t)myrow * p.ldx + h * D;
            bf16x8 xp[2][3];
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (s < kst) {
                    const int d = 32 * s + 8 * kq;
                    f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (d < D) v = load8(xr + d);
                    split8<3>(v, xp[s]);
                }
            const float tau = p.temperature[h];
            const float scale = LOG2E / (p.clamp ? clamp_tau(tau) : tau);
            f32x4 w[8];
            float mx = NEG_BIG;
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                w[mt] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
                if (mt < mtn) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        if (s < kst) {
                            const int m = 16 * mt + li, d = 32 * s + 8 * kq;
                            f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                            if (m < M && d < D) v = load8(p.ws + (size_t)m * D + d);
                            bf16x8 wpl[3];
                            split8<3>(v, wpl);
                            acc = mfma_terms<3, 3>(wpl, xp[s], acc);
                        }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int mr = 16 * mt + 4 * kq + r;
                        const float z = mr < M ? (acc[r] + p.bs[mr < M ? mr : 0]) * scale : NEG_BIG;
                        w[mt][r] = z;
                        mx = fmaxf(mx, z);
                    }
                }
            }
            mx = kq_max_shfl(mx);
            float sm = 0.f;
#pragma unroll
            for (int mt = 0; mt < 8; ++mt)
                if (mt < mtn) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = ex2(w[mt][r] - mx);
                        w[mt][r] = e;
                        sm += e;
                    }
                } else {
                    w[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            sm = kq_sum_shfl(sm);
            const float inv = 1.0f / sm;
            f32x4 yres[4];
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) yres[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int b_lo = g0 / p.N, b_hi = min(g0 + 15, R - 1) / p.N;
            for (int b = b_lo; b <= b_hi; ++b) {
                const float* ob = p.o + (size_t)(b * p.heads + h) * M * D;
                f32x4 yacc[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) yacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < mun) {
                        // k slot (kq, j) of step u: slice 32 u + 4 kq + j (j < 4), 32 u + 16 + 4 kq + j - 4 otherwise
                        const f32x8 wv = {w[2 * u][0], w[2 * u][1], w[2 * u][2], w[2 * u][3],
                                          w[2 * u + 1][0], w[2 * u + 1][1], w[2 * u + 1][2], w[2 * u + 1][3]};
                        bf16x8 wp[3];
                        split8<3>(wv, wp);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt)
                            if (dt < dtn) {
                                const int d = 16 * dt + li;
                                f32x8 ov;
#pragma unroll
                                for (int j = 0; j < 8; ++j) {
                                    const int m = 32 * u + (j < 4 ? 4 * kq + j : 12 + 4 * kq + j);
                                    ov[j] = (m < M && d < D) ? ob[(size_t)m * D + d] : 0.f;
                                }
                                bf16x8 opl[3];
                                split8<3>(ov, opl);
                                yacc[dt] = mfma_terms<3, 3>(opl, wp, yacc[dt]);
                            }
                    }
                if (myb == b) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) yres[dt] = yacc[dt];
                }
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                if (dt < dtn && 16 * dt + 4 * kq < D) {
                    const int col = h * D + 16 * dt + 4 * kq;
                    const float4 y = make_float4(yres[dt][0] * inv, yres[dt][1] * inv, yres[dt][2] * inv, yres[dt][3] * inv);
                    store_planes4(pl1, plane_bytes, (unsigned)((16 * rt + li) * PP + col) * 2, y);
                    if (p.y_dbg && g0 + li < R) *reinterpret_cast<float4*>(p.y_dbg + (size_t)(g0 + li) * C + col) = y;
                }
        }
    }
    __syncthreads();

    // ---- stage 1: a = y . Wo^T + bo + fx -> fbuf.  A wave owns the column tiles wave and wave + 8 (C <= 256: at most two)
    const bool has0 = wave < ctiles, two = wave + TAIL_WAVES < ctiles;
    auto zero2 = [](f32x4 (&acc)[2][PT]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rt = 0; rt < PT; ++rt) acc[i][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    if (has0) {
        f32x4 acc[2][PT];
        zero2(acc);
        gemm_pair<PT>(acc, two, pl1, plane_bytes, PP, p.img_o, cks, wave, 0, cks, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i == 1 && !two) break;
            const int n0 = 16 * (wave + TAIL_WAVES * i) + 4 * kq;
            const float4 bo = *reinterpret_cast<const float4*>(p.bo + n0);
#pragma unroll
            for (int rt = 0; rt < PT; ++rt) {
                const int row = 16 * rt + li, g = row0 + row;
                const float4 f = *reinterpret_cast<const float4*>(p.fx + (size_t)min(g, R - 1) * p.ldfx + n0);
                const float4 a = make_float4((acc[i][rt][0] + bo.x) + f.x, (acc[i][rt][1] + bo.y) + f.y,
                                             (acc[i][rt][2] + bo.z) + f.z, (acc[i][rt][3] + bo.w) + f.w);
                *reinterpret_cast<float4*>(fbuf + row * FP + n0) = a;
                if (p.a_dbg && g < R) *reinterpret_cast<float4*>(p.a_dbg + (size_t)g * C + n0) = a;
            }
        }
    }
    __syncthreads();

    // ---- stage 2: LN2(a) -> planes in pl1 (y is no longer needed)
    ln_rows<PT>(fbuf, C, p.g2, p.be2, p.eps, pl1, plane_bytes, nullptr, 0);
    __syncthreads();

    // ---- stage 3: per C-wide chunk of the hidden layer: h chunk -> pl2, out accumulators += W2[:, chunk] . h chunk
    f32x4 oacc[2][PT];
    zero2(oacc);
    const int nchunk = p.hidden / C, hks = p.hidden >> 5;
    for (int c = 0; c < nchunk; ++c) {
        if (has0) {
            f32x4 acc[2][PT];
            zero2(acc);
            gemm_pair<PT>(acc, two, pl1, plane_bytes, PP, p.img_1, cks, c * ctiles + wave, 0, cks, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i == 1 && !two) break;
                const int n0 = 16 * (wave + TAIL_WAVES * i) + 4 * kq, hb = c * C + n0;
                const float4 b1 = *reinterpret_cast<const float4*>(p.b1 + hb);
#pragma unroll
                for (int rt = 0; rt < PT; ++rt) {
                    const int row = 16 * rt + li, g = row0 + row;
                    const float4 hv = make_float4(act_fwd(p.act, acc[i][rt][0] + b1.x), act_fwd(p.act, acc[i][rt][1] + b1.y),
                                                  act_fwd(p.act, acc[i][rt][2] + b1.z), act_fwd(p.act, acc[i][rt][3] + b1.w));
                    store_planes4(pl2, plane_bytes, (unsigned)(row * PP + n0) * 2, hv);
                    if (p.h_dbg && g < R) *reinterpret_cast<float4*>(p.h_dbg + (size_t)g * p.hidden + hb) = hv;
                }
            }
        }
        __syncthreads();
        if (has0) gemm_pair<PT>(oacc, two, pl2, plane_bytes, PP, p.img_2, hks, wave, c * cks, cks, lane);
        __syncthreads();
    }
    // out = acc + b2 + a, kept in fbuf for the trailing LayerNorm
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int nt = wave + TAIL_WAVES * i;
        if (nt < ctiles) {
            const int n0 = 16 * nt + 4 * kq;
            const float4 b2 = *reinterpret_cast<const float4*>(p.b2 + n0);
#pragma unroll
            for (int rt = 0; rt < PT; ++rt) {
                const int row = 16 * rt + li, g = row0 + row;
                const float4 a = *reinterpret_cast<const float4*>(fbuf + row * FP + n0);
                const float4 v = make_float4((oacc[i][rt][0] + b2.x) + a.x, (oacc[i][rt][1] + b2.y) + a.y,
                                             (oacc[i][rt][2] + b2.z) + a.z, (oacc[i][rt][3] + b2.w) + a.w);
                *reinterpret_cast<float4*>(fbuf + row * FP + n0) = v;
                if (g < R) *reinterpret_cast<float4*>(p.out + (size_t)g * C + n0) = v;
            }
        }
    }
    if (!p.gn) return;
    __syncthreads();

    // ---- stage 4: xn = LN(out)
    ln_rows<PT>(fbuf, C, p.gn, p.bn, p.eps, nullptr, 0, p.xn + (size_t)row0 * C, R - row0);
}

// w [N][K] (row pitch ldw) -> fragment-order plane image, one wave per (16 x 32) tile
__global__ __launch_bounds__(64) void tail_image_kernel(const float* w, long long ldw, unsigned char* img, int ks_total) {
    const int lane = threadIdx.x, li = lane & 15, kq = lane >> 4;
    const int nt = (int)blockIdx.x / ks_total, s = (int)blockIdx.x % ks_total;
    const f32x8 v = load8(w + (size_t)(16 * nt + li) * ldw + 32 * s + 8 * kq);
    bf16x8 pl[3];
    split8<3>(v, pl);
    unsigned char* dst = img + (size_t)blockIdx.x * TILE_IMG + lane * 16;
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8*>(dst + q * 1024) = pl[q];
}

size_t tail_lds(int C, int P) { return (size_t)P * (C + FPAD) * 4 + (size_t)6 * P * (C + PPAD) * 2; }
size_t tail_image_bytes(int N, int K) { return (size_t)N * K * 6; }

// panel height: 16 rows keep every CU busy up to 4096 rows; from 2 panels of 32 per CU on, the taller panel halves the
// weight-image reads per row.  PA2D_TAIL_PANEL=16|32 forces one (A/B timing).
int tail_panel(int R) {
    const int forced = pa2d_env().tail_panel;
    if (forced == 16 || forced == 32) return forced;
    return R >= 32 * 512 ? 32 : 16;
}

bool past_4g(unsigned long long rows, unsigned long long ld, unsigned long long w) {
    return rows && ((rows - 1) * ld + w) * 4ull >= 0xFFFFFFF0ull;
}

}  // namespace

extern "C" {

int pa2d_block_tail_supported(int C, int heads, int D, int M, int hidden, int act, int engine) {
    if (engine != 1) return 0;
    if (C != 64 && C != 128 && C != 256) return 0;
    if (D != 8 && D != 16 && D != 32 && D != 64) return 0;
    if (heads < 1 || (long long)heads * D != C) return 0;
    if (M < 1 || M > 128) return 0;
    if (hidden < C || hidden % C != 0 || hidden / C > 4) return 0;
    if (act < 0 || act > 7) return 0;
    return 1;
}

size_t pa2d_block_tail_lds_bytes(int C, int heads, int D, int M, int hidden, int act, int engine) {
    if (!pa2d_block_tail_supported(C, heads, D, M, hidden, act, engine)) return 0;
    return tail_lds(C, 32);
}

size_t pa2d_block_tail_image_bytes(int N, int K) { return (N % 16 || K % 32 || N < 16 || K < 32) ? 0 : tail_image_bytes(N, K); }

int pa2d_block_tail_weight_image(const float* w, long long ldw, void* img, size_t img_bytes, int N, int K, int engine,
                                 hipStream_t st) {
    if (engine != 1 || N < 16 || K < 32 || N % 16 || K % 32) return PA2D_ERR_UNSUPPORTED;
    if (past_4g((unsigned long long)N, (unsigned long long)ldw, (unsigned long long)K)) return PA2D_ERR_UNSUPPORTED;
    if (!w || !img || ldw < K || (ldw & 3) || ((uintptr_t)w & 15) || ((uintptr_t)img & 15)) return PA2D_ERR_ARG;
    if (img_bytes < tail_image_bytes(N, K)) return PA2D_ERR_WORKSPACE;
    hipLaunchKernelGGL(tail_image_kernel, dim3((N / 16) * (K / 32)), dim3(64), 0, st, w, ldw, (unsigned char*)img, K / 32);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

size_t pa2d_block_tail_workspace(int C, int hidden) {
    if (C < 32 || hidden < 32 || C % 32 || hidden % 32) return 0;
    return tail_image_bytes(C, C) + 2 * tail_image_bytes(hidden, C);
}

int pa2d_block_tail_fwd(const float* xm, long long ldx, const float* o, const float* ws, const float* bs,
                        const float* temperature, const float* fx, long long ldfx, const float* wo, const float* bo,
                        const float* g2, const float* be2, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* gn, const float* bn, float* out, float* xn, float* y_dbg,
                        float* a_dbg, float* h_dbg, const void* wimg_o, const void* wimg_1, const void* wimg_2, void* wsp,
                        size_t wsp_bytes, int B, int N, int heads, int D, int M, int hidden, int act, int clamp_temperature,
                        int engine, float eps, hipStream_t st) {
    const int C = heads > 0 && D > 0 && (long long)heads * D <= 1024 ? heads * D : 0;
    if (!pa2d_block_tail_supported(C, heads, D, M, hidden, act, engine)) return PA2D_ERR_UNSUPPORTED;
    if (B < 0 || N < 1) return PA2D_ERR_ARG;
    const unsigned long long R = (unsigned long long)B * (unsigned long long)N;
    if (R >= 0x7FFFFFFFull || past_4g(R, (unsigned long long)(ldx > 0 ? ldx : C), C) ||
        past_4g(R, (unsigned long long)(ldfx > 0 ? ldfx : C), C) || past_4g(R, (unsigned long long)hidden, hidden) ||
        past_4g((unsigned long long)B * heads * M, D, D))
        return PA2D_ERR_UNSUPPORTED;
    if (B == 0) return PA2D_OK;
    if (!xm || !o || !ws || !bs || !temperature || !fx || !bo || !g2 || !be2 || !b1 || !b2 || !out) return PA2D_ERR_ARG;
    if ((gn == nullptr) != (bn == nullptr) || (gn && !xn)) return PA2D_ERR_ARG;
    if (ldx < C || ldfx < C || (ldx & 3) || (ldfx & 3)) return PA2D_ERR_ARG;
    const uintptr_t al = (uintptr_t)xm | (uintptr_t)o | (uintptr_t)ws | (uintptr_t)fx | (uintptr_t)bo | (uintptr_t)g2 |
                         (uintptr_t)be2 | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)gn | (uintptr_t)bn | (uintptr_t)out |
                         (uintptr_t)xn | (uintptr_t)y_dbg | (uintptr_t)a_dbg | (uintptr_t)h_dbg | (uintptr_t)wimg_o |
                         (uintptr_t)wimg_1 | (uintptr_t)wimg_2 | (uintptr_t)wsp;
    if (al & 15) return PA2D_ERR_ARG;
    // images not supplied are made here, in the caller's workspace (one small launch each)
    const size_t io = tail_image_bytes(C, C), ih = tail_image_bytes(hidden, C);
    unsigned char* wsb = (unsigned char*)wsp;
    size_t need = (wimg_o ? 0 : io) + (wimg_1 ? 0 : ih) + (wimg_2 ? 0 : ih), used = 0;
    if (need && (!wsp || wsp_bytes < need)) return PA2D_ERR_WORKSPACE;
    if ((!wimg_o && !wo) || (!wimg_1 && !w1) || (!wimg_2 && !w2)) return PA2D_ERR_ARG;
    if (!wimg_o) {
        int rc = pa2d_block_tail_weight_image(wo, C, wsb + used, io, C, C, engine, st);
        if (rc) return rc;
        wimg_o = wsb + used; used += io;
    }
    if (!wimg_1) {
        int rc = pa2d_block_tail_weight_image(w1, C, wsb + used, ih, hidden, C, engine, st);
        if (rc) return rc;
        wimg_1 = wsb + used; used += ih;
    }
    if (!wimg_2) {
        int rc = pa2d_block_tail_weight_image(w2, hidden, wsb + used, ih, C, hidden, engine, st);
        if (rc) return rc;
        wimg_2 = wsb + used; used += ih;
    }
    TailParams p;
    p.xm = xm; p.ldx = ldx; p.o = o; p.ws = ws; p.bs = bs; p.temperature = temperature; p.fx = fx; p.ldfx = ldfx;
    p.bo = bo; p.g2 = g2; p.be2 = be2; p.b1 = b1; p.b2 = b2; p.gn = gn; p.bn = bn;
    p.img_o = (const unsigned char*)wimg_o; p.img_1 = (const unsigned char*)wimg_1; p.img_2 = (const unsigned char*)wimg_2;
    p.out = out; p.xn = xn; p.y_dbg = y_dbg; p.a_dbg = a_dbg; p.h_dbg = h_dbg;
    p.R = (int)R; p.N = N; p.heads = heads; p.D = D; p.M = M; p.C = C; p.hidden = hidden; p.act = act;
    p.clamp = clamp_temperature ? 1 : 0; p.eps = eps;
    const int P = tail_panel((int)R);
    const size_t smem = tail_lds(C, P);
    const void* kern = P == 32 ? reinterpret_cast<const void*>(&block_tail_kernel<2>)
                               : reinterpret_cast<const void*>(&block_tail_kernel<1>);
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((R + P - 1) / P)), block(TAIL_THREADS);
    if (P == 32) hipLaunchKernelGGL(block_tail_kernel<2>, grid, block, smem, st, p);
    else hipLaunchKernelGGL(block_tail_kernel<1>, grid, block, smem, st, p);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
