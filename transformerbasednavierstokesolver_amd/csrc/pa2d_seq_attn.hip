// Sequence attention of the SequenSolver latent model (reference SequenSolver.py:319-331): single-head attention among
// the T frame tokens of one sample, each token a whole code of width dim = M*C.
//
//   attn[b] = softmax_T(q[b] k[b]^T * scale)      [T, T]        out[b] = attn[b] v[b] (+ res[b])      [T, dim]
//
// T is small (<= 32) and dim is large (<= 1024): the shape is the transpose of the slice-token attention of
// pa2d_tokens.hip (many tokens of few channels, projections fused), so the work is laid out the other way round.
//   scores kernel  one workgroup per sample; q and k travel through LDS in chunks of DC channels (at T = 32, dim = 1024
//                  each of q, k, v is 128 KiB: the three never fit the 160 KiB of LDS together), every thread owns up to
//                  four of the T*T scores and accumulates them in fp64 (exact products of floats); the T x T
//                  scores (<= 4 KiB) then get their row softmax (forward) or the softmax backward (backward: the same
//                  kernel on (dout, v) gives dA, and ds = attn * (dA - <attn, dA>) * scale).
//   apply kernel   out = W v (or W^T v) for a [T, T] matrix W: grid (dim / CW, B, problems); the backward's three products
//                  dq = ds k, dk = ds^T q, dv = attn^T dout are one launch.
// fp32 FMA on the VALU (fp64 for the score sums) on every engine (2 T^2 dim FLOP per product: 2 MFLOP at the largest shape); every sum runs
// in a fixed order inside one thread, so results repeat bit for bit.  No parameters, hence no accumulate flag.
#include "pa2d_internal.h"

namespace {

constexpr int NT = 256;
constexpr int TMAX = 32;         // tokens
constexpr int DIM_MAX = 1024;    // the LayerNorm limit of the tokens (256 * LN_MAXV)
constexpr int DC = 128;          // channels per LDS chunk of the scores kernel
constexpr int QS = DC + 4;       // its row pitch: 16-byte aligned rows, row r starts at bank 4r
constexpr int CW = 256;          // channels per workgroup of the apply kernel
constexpr int SP = TMAX + 1;     // pitch of the score matrix in LDS

// MODE 0: out = softmax(x y^T * scale) rows;  MODE 1: out = a * (x y^T - <a, x y^T>_row) * scale with a = attn
// CAUSAL (the merged SequenSolver's mask, SequenSolverMerged.py): row i sees the entries j <= i only: their dot products are
// the only ones formed, the softmax and the ds sum run over them, and out[i, j > i] is stored as exactly 0
template <int MODE, bool CAUSAL>
__global__ __launch_bounds__(NT) void seq_scores_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ attn, float* __restrict__ out, int T,
                                                        int dim, float scale) {
    __shared__ __attribute__((aligned(16))) float xs[TMAX * QS];
    __shared__ __attribute__((aligned(16))) float ys[TMAX * QS];
    __shared__ float sc[TMAX * SP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (long long)b * T * dim;
    const float* yb = y + (long long)b * T * dim;
    const int TT = T * T;
    // the T*T dot products run over up to 1024 channels and feed differences of nearly equal scores (the softmax and
    // its backward): they are accumulated in fp64, where a product of two floats is exact (2 T^2 dim FLOP: nothing)
    double acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = 0.0;
    for (int d0 = 0; d0 < dim; d0 += DC) {
        __syncthreads();                           // the previous chunk's readers are done
        for (int e = tid; e < T * (DC / 4); e += NT) {
            const int r = e / (DC / 4), c = (e % (DC / 4)) * 4;
            float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), yv = xv;
            if (d0 + c < dim) {                    // dim % 4 == 0: a float4 is inside the row or outside it
                xv = *reinterpret_cast<const float4*>(xb + (long long)r * dim + d0 + c);
                yv = *reinterpret_cast<const float4*>(yb + (long long)r * dim + d0 + c);
            }
            *reinterpret_cast<float4*>(xs + r * QS + c) = xv;
            *reinterpret_cast<float4*>(ys + r * QS + c) = yv;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = tid + s * NT;
            if (e < TT && (!CAUSAL || e % T <= e / T)) {
                const float4* xr = reinterpret_cast<const float4*>(xs + (e / T) * QS);
                const float4* yr = reinterpret_cast<const float4*>(ys + (e % T) * QS);
                double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
                for (int c = 0; c < DC / 4; ++c) {
                    const float4 u = xr[c], w = yr[c];
                    a0 = fma((double)u.x, (double)w.x, a0);
                    a1 = fma((double)u.y, (double)w.y, a1);
                    a0 = fma((double)u.z, (double)w.z, a0);
                    a1 = fma((double)u.w, (double)w.w, a1);
                }
                acc[s] += a0 + a1;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = tid + s * NT;
        if (e < TT) sc[(e / T) * SP + e % T] = (float)acc[s];
    }
    __syncthreads();
    if (tid >= T) return;
    const float* row = sc + tid * SP;
    float* o = out + (long long)b * TT + tid * T;
    const int n = CAUSAL ? tid + 1 : T;
    for (int j = n; j < T; ++j) o[j] = 0.f;
    if (MODE == 0) {
        float mx = -INFINITY;
        for (int j = 0; j < n; ++j) mx = fmaxf(mx, row[j] * scale);
        float sum = 0.f;
        for (int j = 0; j < n; ++j) sum += expf(row[j] * scale - mx);
        for (int j = 0; j < n; ++j) o[j] = expf(row[j] * scale - mx) / sum;
    } else {
        const float* a = attn + (long long)b * TT + tid * T;
        // dA_j - <a, dA> written as sum_k a_k (dA_j - dA_k) (sum a = 1): nothing is lost to cancellation near one-hot rows
        for (int j = 0; j < n; ++j) {
            float sd = 0.f;
            for (int k = 0; k < n; ++k) sd = fmaf(a[k], row[j] - row[k], sd);
            o[j] = a[j] * sd * scale;
        }
    }
}

// up to three products o_p[b] = W_p[b] v_p[b] (trans_p = 0) or W_p[b]^T v_p[b] (1) (+ r_p[b] when r_p is not NULL: the
// residual of the block), W_p [B, T, T], v_p / o_p / r_p [B, T, dim]
struct ApplyArgs {
    const float* w[3];
    const float* v[3];
    const float* r[3];
    float* o[3];
    int trans[3];
};

__global__ __launch_bounds__(NT) void seq_apply_kernel(const ApplyArgs args, int T, int dim) {
    __shared__ float wl[TMAX * TMAX];
    __shared__ __attribute__((aligned(16))) float vs[TMAX * CW];
    const int tid = threadIdx.x, b = blockIdx.y, c0 = blockIdx.x * CW;
    const float* W;
    const float* V;
    const float* Rr;
    float* O;
    int trans;
    if (blockIdx.z == 0) { W = args.w[0]; V = args.v[0]; Rr = args.r[0]; O = args.o[0]; trans = args.trans[0]; }
    else if (blockIdx.z == 1) { W = args.w[1]; V = args.v[1]; Rr = args.r[1]; O = args.o[1]; trans = args.trans[1]; }
    else { W = args.w[2]; V = args.v[2]; Rr = args.r[2]; O = args.o[2]; trans = args.trans[2]; }
    W += (long long)b * T * T;
    V += (long long)b * T * dim;
    O += (long long)b * T * dim;
    if (Rr) Rr += (long long)b * T * dim;
    for (int e = tid; e < T * T; e += NT) {
        const int i = e / T, j = e % T;
        wl[e] = trans ? W[j * T + i] : W[e];
    }
    for (int e = tid; e < T * (CW / 4); e += NT) {
        const int r = e / (CW / 4), c = (e % (CW / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + c < dim) v = *reinterpret_cast<const float4*>(V + (long long)r * dim + c0 + c);
        *reinterpret_cast<float4*>(vs + r * CW + c) = v;
    }
    __syncthreads();
    const int c = (tid % (CW / 4)) * 4;            // one wave per row group: its lanes read one wl element
    if (c0 + c >= dim) return;
    for (int i = tid / (CW / 4); i < T; i += NT / (CW / 4)) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < T; ++j) {
            const float w = wl[i * T + j];
            const float4 v = *reinterpret_cast<const float4*>(vs + j * CW + c);
            a.x = fmaf(w, v.x, a.x);
            a.y = fmaf(w, v.y, a.y);
            a.z = fmaf(w, v.z, a.z);
            a.w = fmaf(w, v.w, a.w);
        }
        if (Rr) {
            const float4 r = *reinterpret_cast<const float4*>(Rr + (long long)i * dim + c0 + c);
            a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
        }
        *reinterpret_cast<float4*>(O + (long long)i * dim + c0 + c) = a;
    }
}

int check_shape(int B, int T, int dim) {
    if (T < 1 || T > TMAX) return PA2D_ERR_UNSUPPORTED;
    if (dim < 4 || (dim & 3) || dim > DIM_MAX) return PA2D_ERR_UNSUPPORTED;
    if (B < 0) return PA2D_ERR_ARG;
    if ((unsigned long long)B * T * dim * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}
bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

template <bool CAUSAL>
int seq_attn_fwd(const float* q, const float* k, const float* v, const float* res, float* out, float* attn, int B, int T,
                 int dim, float scale, void* stream) {
    const int rc = check_shape(B, T, dim);
    if (rc) return rc;
    if (B == 0) return PA2D_OK;
    if (!q || !k || !v || !out || !attn) return PA2D_ERR_ARG;
    if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out) || misaligned(res)) return PA2D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((seq_scores_kernel<0, CAUSAL>), dim3(B), dim3(NT), 0, st, q, k, (const float*)nullptr, attn, T, dim,
                       scale);
    PA2D_CHECK_LAUNCH();
    ApplyArgs a = {};
    a.w[0] = attn; a.v[0] = v; a.r[0] = res; a.o[0] = out; a.trans[0] = 0;
    hipLaunchKernelGGL(seq_apply_kernel, dim3(ceil_div(dim, CW), B, 1), dim3(NT), 0, st, a, T, dim);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

size_t bwd_workspace(int B, int T) {
    if (B <= 0 || T < 1 || T > TMAX) return 0;
    return sizeof(float) * (size_t)B * T * T;
}

template <bool CAUSAL>
int seq_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dout, float* dq, float* dk,
                 float* dv, void* ws, size_t ws_bytes, int B, int T, int dim, float scale, void* stream) {
    const int rc = check_shape(B, T, dim);
    if (rc) return rc;
    if (B == 0) return PA2D_OK;
    if (!q || !k || !v || !attn || !dout || !dq || !dk || !dv) return PA2D_ERR_ARG;
    if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(dout) || misaligned(dq) || misaligned(dk) || misaligned(dv))
        return PA2D_ERR_ARG;
    if (!ws || ws_bytes < bwd_workspace(B, T)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* ds = (float*)ws;
    hipLaunchKernelGGL((seq_scores_kernel<1, CAUSAL>), dim3(B), dim3(NT), 0, st, dout, v, attn, ds, T, dim, scale);
    PA2D_CHECK_LAUNCH();
    ApplyArgs a = {};
    a.w[0] = ds;   a.v[0] = k;    a.o[0] = dq; a.trans[0] = 0;      // dq = ds k
    a.w[1] = ds;   a.v[1] = q;    a.o[1] = dk; a.trans[1] = 1;      // dk = ds^T q
    a.w[2] = attn; a.v[2] = dout; a.o[2] = dv; a.trans[2] = 1;      // dv = attn^T dout
    hipLaunchKernelGGL(seq_apply_kernel, dim3(ceil_div(dim, CW), B, 3), dim3(NT), 0, st, a, T, dim);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // namespace

extern "C" {

int pa2d_seq_attn_fwd(const float* q, const float* k, const float* v, const float* res, float* out, float* attn, int B,
                      int T, int dim, float scale, void* stream) {
    return seq_attn_fwd<false>(q, k, v, res, out, attn, B, T, dim, scale, stream);
}

size_t pa2d_seq_attn_bwd_workspace(int B, int T) { return bwd_workspace(B, T); }

int pa2d_seq_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dout, float* dq,
                      float* dk, float* dv, void* ws, size_t ws_bytes, int B, int T, int dim, float scale, void* stream) {
    return seq_attn_bwd<false>(q, k, v, attn, dout, dq, dk, dv, ws, ws_bytes, B, T, dim, scale, stream);
}

int pa2d_seq_attn_causal_fwd(const float* q, const float* k, const float* v, const float* res, float* out, float* attn,
                             int B, int T, int dim, float scale, void* stream) {
    return seq_attn_fwd<true>(q, k, v, res, out, attn, B, T, dim, scale, stream);
}

int pa2d_seq_attn_causal_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dout, float* dq,
                             float* dk, float* dv, void* ws, size_t ws_bytes, int B, int T, int dim, float scale,
                             void* stream) {
    return seq_attn_bwd<true>(q, k, v, attn, dout, dq, dk, dv, ws, ws_bytes, B, T, dim, scale, stream);
}

}  // extern "C"
