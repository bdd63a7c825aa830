// Materialised slice weights and the de-slice with an explicit weight tensor: the two per-point operations of the
// structured-mesh auto-encoder attention (reference model/Physics_Attention.py,
// Physics_Attention_Structured_Mesh_2D_Auto_Encoder.encode / reconstruct_fx / decode), which caches the softmax slice
// weights, projects them with a Linear(M, M) and de-slices with the projected tensor.
//
//   slice weights  sw[b,h,n,m] = softmax_m((x_mid[b,n,h*D:(h+1)*D] . Ws[m,:] + bs[m]) / t_h)
//   de-slice       y[b,n,h*D+d] = sum_g w[b,h,n,g] code[b,h,g,d]          (einsum "bhgc,bhng->bhnc" + rearrange)
//
// Every contraction is an fp32 FMA on the VALU (exact fp32 on every engine; these stages move at most 16 FLOP per byte
// of the [B,heads,N,M] tensor at D <= 32, so HBM, not the matrix cores, is their limit).  Parameter-gradient and code-
// gradient reductions write one partial-sum record per workgroup and sum the records in a fixed order: deterministic.
#include "pa2d_internal.h"

namespace {

constexpr int NT = 256;      // threads per workgroup (4 waves)
constexpr int R = 32;        // points per LDS tile of the backward / de-slice kernels

__device__ __forceinline__ float clamp_t(float t, int clamp) { return clamp ? fminf(fmaxf(t, 0.1f), 5.0f) : t; }

// Row groups: G lanes own one point's M slice logits (lane q holds m = q and, for MP = 128, m = q + 64); G divides 64,
// so a group never straddles a wave and the softmax reductions are xor shuffles inside it.
template <int MP> struct Rows {
    static constexpr int G = MP < 64 ? MP : 64;
    static constexpr int MPL = MP / G;           // slice indices per lane: 1, or 2 at MP = 128
    static constexpr int RPP = NT / G;           // points per pass of the workgroup
};
template <int G> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// softmax over the M logits held by one group; l[j] = -inf for m >= M
template <int MP> __device__ __forceinline__ void group_softmax(const float (&l)[Rows<MP>::MPL], float (&p)[Rows<MP>::MPL]) {
    constexpr int G = Rows<MP>::G, MPL = Rows<MP>::MPL;
    float mx = l[0];
#pragma unroll
    for (int j = 1; j < MPL; ++j) mx = fmaxf(mx, l[j]);
    mx = group_max<G>(mx);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        p[j] = expf(l[j] - mx);
        s += p[j];
    }
    s = group_sum<G>(s);
#pragma unroll
    for (int j = 0; j < MPL; ++j) p[j] = p[j] / s;
}

// ------------------------------------------------------------------------------------------------ slice weights
// grid (chunks, B*heads); each workgroup walks points [n0, n1) of one (b, h), one point per row group.  The slice
// projection lives in registers (D floats per slice index of the lane); the point's x_mid head segment is read by
// every lane of its group (one cache line, broadcast).
template <int D, int MP>
__global__ __launch_bounds__(NT) void slice_weights_fwd_kernel(const float* __restrict__ xm, long long ldx,
                                                              const float* __restrict__ ws, const float* __restrict__ bs,
                                                              const float* __restrict__ temperature, float* __restrict__ sw,
                                                              int N, int heads, int M, int clamp, int ppb) {
    using RW = Rows<MP>;
    constexpr int G = RW::G, MPL = RW::MPL, RPP = RW::RPP;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int q = threadIdx.x % G, rp = threadIdx.x / G;
    const int n0 = blockIdx.x * ppb;
    const int n1 = min(N, n0 + ppb);
    float w[MPL][D], bias[MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        const int m = q + j * G;
#pragma unroll
        for (int d = 0; d < D; ++d) w[j][d] = m < M ? ws[m * D + d] : 0.f;
        bias[j] = m < M ? bs[m] : 0.f;
    }
    const float t = clamp_t(temperature[h], clamp);
    for (int n = n0 + rp; n < n1; n += RPP) {
        const float* xr = xm + ((long long)b * N + n) * ldx + h * D;
        float x[D];
#pragma unroll
        for (int d = 0; d < D; d += 4) {
            const float4 v = *reinterpret_cast<const float4*>(xr + d);
            x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
        }
        float l[MPL], p[MPL];
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            float z = bias[j];
#pragma unroll
            for (int d = 0; d < D; ++d) z = fmaf(x[d], w[j][d], z);
            l[j] = (q + j * G) < M ? z / t : -INFINITY;
        }
        group_softmax<MP>(l, p);
        float* out = sw + ((long long)bh * N + n) * M;
#pragma unroll
        for (int j = 0; j < MPL; ++j)
            if (q + j * G < M) out[q + j * G] = p[j];
    }
}

// Backward of the slice weights: recomputes the logits from x_mid (no sw input), then
//   dl = sw * (dsw - <sw, dsw>),  dz = dl / t,  dt_h = -(sum dl * l) / t (clamp mask),
//   dx_mid[n, d] = sum_m dz[n, m] Ws[m, d]   (plain store),   dWs += dz^T x_mid,  dbs += sum_n dz.
// One partial-sum record per workgroup: [dWs M*D | dbs M | dt heads] (only this head's dt slot non-zero).
template <int D, int MP>
__global__ __launch_bounds__(NT) void slice_weights_bwd_kernel(const float* __restrict__ xm, long long ldx,
                                                              const float* __restrict__ ws, const float* __restrict__ bs,
                                                              const float* __restrict__ temperature,
                                                              const float* __restrict__ dsw, float* __restrict__ dxm,
                                                              long long lddx, float* __restrict__ part, int N, int heads,
                                                              int M, int clamp, int ppb) {
    using RW = Rows<MP>;
    constexpr int G = RW::G, MPL = RW::MPL, RPP = RW::RPP;
    constexpr int XS = D + 1, ZS = MP + 1, WS = D + 1;
    constexpr int KW = (MP * D + NT - 1) / NT;        // owned dWs elements per thread
    __shared__ float xs[R * XS];
    __shared__ float zs[R * ZS];
    __shared__ float wl[MP * WS];
    __shared__ float red[NT * MPL];
    __shared__ float tred[NT / 64];
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int tid = threadIdx.x, q = tid % G, rp = tid / G;
    const int n0 = blockIdx.x * ppb;
    const int n1 = min(N, n0 + ppb);
    const int MD = M * D;
    for (int e = tid; e < MP * D; e += NT) {
        const int m = e / D, d = e % D;
        wl[m * WS + d] = m < M ? ws[e] : 0.f;
    }
    float bias[MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) bias[j] = (q + j * G) < M ? bs[q + j * G] : 0.f;
    const float traw = temperature[h];
    const float t = clamp_t(traw, clamp);
    float acc[KW], dbs_acc[MPL], dt_acc = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < MPL; ++j) dbs_acc[j] = 0.f;
    for (int t0 = n0; t0 < n1; t0 += R) {
        const int rows = min(R, n1 - t0);
        __syncthreads();                       // previous tile's readers are done (and wl is staged on the first tile)
        for (int e = tid; e < R * D; e += NT) {
            const int r = e / D, d = e % D;
            xs[r * XS + d] = r < rows ? xm[((long long)b * N + t0 + r) * ldx + h * D + d] : 0.f;
        }
        __syncthreads();
        for (int r = rp; r < R; r += RPP) {
            float dz[MPL];
            if (r < rows) {
                float l[MPL], p[MPL], g[MPL];
                const float* gr = dsw + ((long long)bh * N + t0 + r) * M;
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = q + j * G;
                    float z = bias[j];
#pragma unroll
                    for (int d = 0; d < D; ++d) z = fmaf(xs[r * XS + d], wl[m * WS + d], z);
                    l[j] = m < M ? z / t : -INFINITY;
                    g[j] = m < M ? gr[m] : 0.f;
                }
                group_softmax<MP>(l, p);
                float sd = 0.f;
#pragma unroll
                for (int j = 0; j < MPL; ++j) sd = fmaf(p[j], g[j], sd);
                sd = group_sum<G>(sd);
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const float dl = p[j] * (g[j] - sd);
                    dz[j] = dl / t;
                    if (q + j * G < M) dt_acc = fmaf(dl, l[j], dt_acc);
                    dbs_acc[j] += dz[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < MPL; ++j) dz[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < MPL; ++j) zs[r * ZS + q + j * G] = dz[j];
        }
        __syncthreads();
        if (dxm) {
            for (int e = tid; e < R * D; e += NT) {
                const int r = e / D, d = e % D;
                if (r >= rows) continue;
                float s = 0.f;
                for (int m = 0; m < M; ++m) s = fmaf(zs[r * ZS + m], wl[m * WS + d], s);
                dxm[((long long)b * N + t0 + r) * lddx + h * D + d] = s;
            }
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int e = tid + k * NT;
            if (e < MD) {
                const int m = e / D, d = e % D;
                float s = acc[k];
                for (int r = 0; r < rows; ++r) s = fmaf(zs[r * ZS + m], xs[r * XS + d], s);
                acc[k] = s;
            }
        }
    }
    // the record
    const int rec = MD + M + heads;
    float* out = part + (long long)(blockIdx.y * gridDim.x + blockIdx.x) * rec;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int e = tid + k * NT;
        if (e < MD) out[e] = acc[k];
    }
#pragma unroll
    for (int j = 0; j < MPL; ++j) red[tid * MPL + j] = dbs_acc[j];
    const float dtw = wave_sum(dt_acc);
    if ((tid & 63) == 0) tred[tid >> 6] = dtw;
    __syncthreads();
    for (int m = tid; m < M; m += NT) {
        const int qq = m % G, j = m / G;
        float s = 0.f;
        for (int r = 0; r < RPP; ++r) s += red[(r * G + qq) * MPL + j];
        out[MD + m] = s;
    }
    for (int i = tid; i < heads; i += NT) {
        float v = 0.f;
        if (i == h) {
            const float s = (tred[0] + tred[1]) + (tred[2] + tred[3]);
            const bool pass = !clamp || (traw >= 0.1f && traw <= 5.0f);      // d clamp / d t
            v = pass ? -s / t : 0.f;
        }
        out[MD + M + i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ de-slice
// y[b,n,h*D+d] = sum_g w[b,h,n,g] code[b,h,g,d]: the code of (b, h) is staged once per workgroup, the weight tile of R
// points (R*M contiguous floats) per tile; one thread per output element.
template <int D, int MP>
__global__ __launch_bounds__(NT) void deslice_weights_fwd_kernel(const float* __restrict__ code, const float* __restrict__ w,
                                                                float* __restrict__ y, long long ldy, int N, int heads,
                                                                int M, int ppb) {
    constexpr int WT = MP + 1;
    __shared__ float cl[MP * D];
    __shared__ float wt[R * WT];
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * ppb;
    const int n1 = min(N, n0 + ppb);
    for (int e = tid; e < M * D; e += NT) cl[e] = code[(long long)bh * M * D + e];
    for (int t0 = n0; t0 < n1; t0 += R) {
        const int rows = min(R, n1 - t0);
        const float* wr = w + ((long long)bh * N + t0) * M;
        __syncthreads();
        for (int e = tid; e < rows * M; e += NT) wt[(e / M) * WT + e % M] = wr[e];
        __syncthreads();
        for (int e = tid; e < rows * D; e += NT) {
            const int r = e / D, d = e % D;
            float s = 0.f;
            for (int g = 0; g < M; ++g) s = fmaf(wt[r * WT + g], cl[g * D + d], s);
            y[((long long)b * N + t0 + r) * ldy + h * D + d] = s;
        }
    }
}

// dw[b,h,n,g] = sum_d dy[b,n,h*D+d] code[b,h,g,d] (plain store; skipped when dw is NULL);
// dcode partial of the workgroup: sum over its points of w[n,g] dy[n,d] (one record of M*D floats; skipped when part
// is NULL).
template <int D, int MP>
__global__ __launch_bounds__(NT) void deslice_weights_bwd_kernel(const float* __restrict__ code, const float* __restrict__ w,
                                                                const float* __restrict__ dy, long long lddy,
                                                                float* __restrict__ dw, float* __restrict__ part, int N,
                                                                int heads, int M, int ppb) {
    constexpr int CT = MP + 1, WT = MP + 1, YT = D + 1;
    constexpr int KW = (MP * D + NT - 1) / NT;
    __shared__ float ct[D * CT];
    __shared__ float wt[R * WT];
    __shared__ float yt[R * YT];
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * ppb;
    const int n1 = min(N, n0 + ppb);
    const int MD = M * D;
    if (dw)
        for (int e = tid; e < MD; e += NT) ct[(e % D) * CT + e / D] = code[(long long)bh * MD + e];
    float acc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = 0.f;
    for (int t0 = n0; t0 < n1; t0 += R) {
        const int rows = min(R, n1 - t0);
        __syncthreads();
        for (int e = tid; e < rows * D; e += NT) {
            const int r = e / D, d = e % D;
            yt[r * YT + d] = dy[((long long)b * N + t0 + r) * lddy + h * D + d];
        }
        if (part) {
            const float* wr = w + ((long long)bh * N + t0) * M;
            for (int e = tid; e < rows * M; e += NT) wt[(e / M) * WT + e % M] = wr[e];
        }
        __syncthreads();
        if (dw) {
            float* dwr = dw + ((long long)bh * N + t0) * M;
            for (int e = tid; e < rows * M; e += NT) {
                const int r = e / M, g = e % M;
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) s = fmaf(yt[r * YT + d], ct[d * CT + g], s);
                dwr[e] = s;
            }
        }
        if (part) {
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const int e = tid + k * NT;
                if (e < MD) {
                    const int g = e / D, d = e % D;
                    float s = acc[k];
                    for (int r = 0; r < rows; ++r) s = fmaf(wt[r * WT + g], yt[r * YT + d], s);
                    acc[k] = s;
                }
            }
        }
    }
    if (part) {
        float* out = part + (long long)(blockIdx.y * gridDim.x + blockIdx.x) * MD;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int e = tid + k * NT;
            if (e < MD) out[e] = acc[k];
        }
    }
}

// dcode[bh, e] = sum over the nx records of (b, h), in record order
__global__ __launch_bounds__(NT) void dcode_reduce_kernel(const float* __restrict__ part, float* __restrict__ dcode,
                                                          long long total, int MD, int nx) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const long long bh = i / MD, e = i % MD;
    const float* p = part + bh * nx * MD + e;
    float s = 0.f;
    for (int c = 0; c < nx; ++c) s += p[(long long)c * MD];
    dcode[i] = s;
}

// ------------------------------------------------------------------------------------------------ host side
constexpr unsigned long long DESC_LIMIT = 0xFFFFFFF0ull;     // the 4 GiB contract of include/pa2d.h

int mp_for(int M) { return M <= 8 ? 8 : M <= 16 ? 16 : M <= 32 ? 32 : M <= 64 ? 64 : 128; }

int check_shape(int B, int N, int heads, int D, int M) {
    if (D != 8 && D != 16 && D != 32 && D != 64) return PA2D_ERR_UNSUPPORTED;
    if (M < 1 || M > 128) return PA2D_ERR_UNSUPPORTED;
    if (B < 0 || N < 1 || heads < 1) return PA2D_ERR_ARG;
    return PA2D_OK;
}
bool too_big_rows(int B, int N, long long ld, int heads, int D) {     // a [B*N, ld] activation touched up to heads*D
    return (((unsigned long long)B * N - 1) * (unsigned long long)ld + (unsigned long long)heads * D) * 4ull >= DESC_LIMIT;
}
bool too_big_sw(int B, int N, int heads, int M) {
    return (unsigned long long)B * heads * N * M * 4ull >= DESC_LIMIT;
}

// points per workgroup: a multiple of R, enough workgroups for about `target` in all
int points_per_block(int B, int N, int heads, int target) {
    const int bh = B * heads;
    int nx = ceil_div(target, bh);
    const int maxc = ceil_div(N, R);
    if (nx > maxc) nx = maxc;
    if (nx < 1) nx = 1;
    return ceil_div(ceil_div(N, nx), R) * R;
}
constexpr int FWD_TARGET = 4096, RED_TARGET = 512;

#define SW_DISPATCH(CALL)                                                        \
    switch (D * 1000 + mp_for(M)) {                                              \
        case 8008: CALL(8, 8); break;    case 8016: CALL(8, 16); break;          \
        case 8032: CALL(8, 32); break;   case 8064: CALL(8, 64); break;          \
        case 8128: CALL(8, 128); break;                                          \
        case 16008: CALL(16, 8); break;  case 16016: CALL(16, 16); break;        \
        case 16032: CALL(16, 32); break; case 16064: CALL(16, 64); break;        \
        case 16128: CALL(16, 128); break;                                        \
        case 32008: CALL(32, 8); break;  case 32016: CALL(32, 16); break;        \
        case 32032: CALL(32, 32); break; case 32064: CALL(32, 64); break;        \
        case 32128: CALL(32, 128); break;                                        \
        case 64008: CALL(64, 8); break;  case 64016: CALL(64, 16); break;        \
        case 64032: CALL(64, 32); break; case 64064: CALL(64, 64); break;        \
        case 64128: CALL(64, 128); break;                                        \
        default: return PA2D_ERR_UNSUPPORTED;                                    \
    }

}  // namespace

extern "C" {

int pa2d_slice_weights_fwd(const float* xm, long long ldx, const float* ws, const float* bs, const float* temperature,
                           float* sw, int B, int N, int heads, int D, int M, int clamp_temperature, void* stream,
                           void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, heads, D, M);
    if (rc) return rc;
    if (ldx < (long long)heads * D || (ldx & 3) || ((uintptr_t)xm & 15)) return PA2D_ERR_ARG;
    if (B == 0) return PA2D_OK;
    if (too_big_rows(B, N, ldx, heads, D) || too_big_sw(B, N, heads, M)) return PA2D_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int ppb = points_per_block(B, N, heads, FWD_TARGET);
    const dim3 grid(ceil_div(N, ppb), B * heads);
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_SWF(D_, MP_)                                                                                        \
    hipLaunchKernelGGL((slice_weights_fwd_kernel<D_, MP_>), grid, dim3(NT), 0, st, xm, ldx, ws, bs, temperature, sw, \
                       N, heads, M, clamp_temperature, ppb)
    SW_DISPATCH(CALL_SWF)
#undef CALL_SWF
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

size_t pa2d_slice_weights_bwd_workspace(int B, int N, int heads, int D, int M) {
    if (check_shape(B, N, heads, D, M) || B == 0) return 0;
    const int ppb = points_per_block(B, N, heads, RED_TARGET);
    const size_t nrec = (size_t)ceil_div(N, ppb) * B * heads;
    return sizeof(float) * nrec * ((size_t)M * D + M + heads);
}

int pa2d_slice_weights_bwd(const float* xm, long long ldx, const float* ws, const float* bs, const float* temperature,
                           const float* dsw, float* dxm, long long lddx, float* dws, float* dbs, float* dtemperature,
                           void* ws_buf, size_t ws_bytes, int B, int N, int heads, int D, int M, int clamp_temperature,
                           int accumulate, void* stream, void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, heads, D, M);
    if (rc) return rc;
    if (ldx < (long long)heads * D || (dxm && lddx < (long long)heads * D)) return PA2D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (accumulate) return PA2D_OK;
        if ((rc = pa2d_zero(dws, sizeof(float) * M * D, st))) return rc;
        if ((rc = pa2d_zero(dbs, sizeof(float) * M, st))) return rc;
        return pa2d_zero(dtemperature, sizeof(float) * heads, st);
    }
    if (!dws || !dbs || !dtemperature) return PA2D_ERR_ARG;
    if (too_big_rows(B, N, ldx, heads, D) || (dxm && too_big_rows(B, N, lddx, heads, D)) || too_big_sw(B, N, heads, M))
        return PA2D_ERR_UNSUPPORTED;
    if (ws_bytes < pa2d_slice_weights_bwd_workspace(B, N, heads, D, M) || !ws_buf) return PA2D_ERR_WORKSPACE;
    const int ppb = points_per_block(B, N, heads, RED_TARGET);
    const int nx = ceil_div(N, ppb);
    const dim3 grid(nx, B * heads);
    float* part = (float*)ws_buf;
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_SWB(D_, MP_)                                                                                           \
    hipLaunchKernelGGL((slice_weights_bwd_kernel<D_, MP_>), grid, dim3(NT), 0, st, xm, ldx, ws, bs, temperature, dsw, \
                       dxm, lddx, part, N, heads, M, clamp_temperature, ppb)
    SW_DISPATCH(CALL_SWB)
#undef CALL_SWB
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    const long long MD = (long long)M * D;
    ReduceSegs segs;
    segs.nseg = 3;
    segs.begin[0] = 0; segs.begin[1] = MD; segs.begin[2] = MD + M; segs.begin[3] = segs.begin[4] = MD + M + heads;
    segs.dst[0] = dws; segs.dst[1] = dbs; segs.dst[2] = dtemperature; segs.dst[3] = nullptr;
    return pa2d_launch_reduce_segs(part, nx * B * heads, MD + M + heads, segs, accumulate, st);
}

int pa2d_deslice_weights_fwd(const float* code, const float* w, float* y, long long ldy, int B, int N, int heads, int D,
                             int M, void* stream, void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, heads, D, M);
    if (rc) return rc;
    if (ldy < (long long)heads * D) return PA2D_ERR_ARG;
    if (B == 0) return PA2D_OK;
    if (too_big_rows(B, N, ldy, heads, D) || too_big_sw(B, N, heads, M)) return PA2D_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int ppb = points_per_block(B, N, heads, FWD_TARGET);
    const dim3 grid(ceil_div(N, ppb), B * heads);
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_DWF(D_, MP_) \
    hipLaunchKernelGGL((deslice_weights_fwd_kernel<D_, MP_>), grid, dim3(NT), 0, st, code, w, y, ldy, N, heads, M, ppb)
    SW_DISPATCH(CALL_DWF)
#undef CALL_DWF
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

size_t pa2d_deslice_weights_bwd_workspace(int B, int N, int heads, int D, int M) {
    if (check_shape(B, N, heads, D, M) || B == 0) return 0;
    const int ppb = points_per_block(B, N, heads, RED_TARGET);
    return sizeof(float) * (size_t)ceil_div(N, ppb) * B * heads * M * D;
}

int pa2d_deslice_weights_bwd(const float* code, const float* w, const float* dy, long long lddy, float* dcode, float* dw,
                             void* ws_buf, size_t ws_bytes, int B, int N, int heads, int D, int M, void* stream,
                             void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, heads, D, M);
    if (rc) return rc;
    if (lddy < (long long)heads * D) return PA2D_ERR_ARG;
    if (B == 0 || (!dcode && !dw)) return PA2D_OK;
    if (too_big_rows(B, N, lddy, heads, D) || too_big_sw(B, N, heads, M)) return PA2D_ERR_UNSUPPORTED;
    if (dcode && (ws_bytes < pa2d_deslice_weights_bwd_workspace(B, N, heads, D, M) || !ws_buf)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int ppb = points_per_block(B, N, heads, RED_TARGET);
    const int nx = ceil_div(N, ppb);
    const dim3 grid(nx, B * heads);
    float* part = dcode ? (float*)ws_buf : nullptr;
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_DWB(D_, MP_) \
    hipLaunchKernelGGL((deslice_weights_bwd_kernel<D_, MP_>), grid, dim3(NT), 0, st, code, w, dy, lddy, dw, part, N, heads, M, ppb)
    SW_DISPATCH(CALL_DWB)
#undef CALL_DWB
    PA2D_CHECK_LAUNCH();
    if (dcode) {
        const long long total = (long long)B * heads * M * D;
        hipLaunchKernelGGL(dcode_reduce_kernel, dim3((unsigned)ceil_div_ll(total, NT)), dim3(NT), 0, st, part, dcode, total,
                           M * D, nx);
        PA2D_CHECK_LAUNCH();
    }
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

}  // extern "C"
