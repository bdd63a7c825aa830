// First layer of the previous-slice predictor (reference LearnSlice.py:125-134, `weight_projection_form_slice`): the
// MLP's input is cat(slice weights of the point [M], flattened code [M C]), so its first Linear separates into a
// per-point product with the first M weight columns and ONE row per sample for the code columns:
//   h0[b, n, :] = act( sum_m sw[b, n, m] Wsw[:, m] + tb[b, :] ),   tb = code[b] . Wtok^T + bias   (a row GEMM elsewhere)
// sw [B, N, M], Wsw [H, M] (row-major, the first M columns of linear_pre's weight made contiguous), tb [B, H], h0 [B, N, H].
//   * pa2d_prev_slice_entry_fwd : one pass, one store per element.  K = M <= 64: exact fp32 FMAs on the vector pipe
//                                 (acc = tb, then m ascending), bounded by the 16-byte-per-lane store stream along H.
//   * pa2d_prev_slice_entry_bwd : reads dh0, recomputes the pre-activation (M FMAs per element, cheaper than saving and
//                                 re-reading an [R, H] tensor), dpre = dh0 act'(pre), and reduces
//                                   dWsw[h, m] = sum_rows dpre[r, h] sw[r, m],   dtb[b, h] = sum_{rows of b} dpre[r, h]
//                                 into one record per (sample, row chunk); the records are added in a fixed order by
//                                 pa2d_launch_reduce_segs: no float atomics, the same bits on every call.
// Work unit = one WAVE: 64 lanes x 4 columns of H (a 256-column tile) x one row chunk of ONE sample (a chunk never
// straddles two samples, so tb and the dtb record belong to one b).  The sw row of a point is uniform across the wave:
// it is read through scalar loads.  The lane's 4 x 16 weights stay in registers for the whole chunk when M <= 16 (the
// reference's M = 16); wider M walks 16-column chunks of Wsw, re-read per row tile (backward: one grid.z slice per
// 16-column chunk of dWsw, each recomputing the full pre-activation).  No LDS, no barriers.
#include "pa2d_internal.h"

#define PS_THREADS 256
#define PS_WAVES 4
#define PS_RT 4                       // rows per tile: independent accumulators / loads in flight
#define PS_MC 16                      // weight columns held in registers at a time
#define PS_ROWS_FWD 64                // rows of a forward chunk
#define PS_ROWS_BWD 128               // rows of a backward chunk == rows behind one partial record
#define PS_MAX_M 64

// w[j][mm] = Wsw[col0 + j][mc + mm], zero outside the matrix (the buffer range check returns 0 for OOB_OFF)
template <int MT>
static __device__ __forceinline__ void ps_load_w(float (&w)[4][PS_MC], __amdgpu_buffer_rsrc_t rw, int col0, int M, int mc,
                                                 bool active) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (MT == PS_MC) {
#pragma unroll
            for (int q = 0; q < PS_MC / 4; ++q) {
                const float4 v = buf_load4(rw, active ? ((unsigned)(col0 + j) * PS_MC + 4u * q) * 4u : OOB_OFF);
                w[j][4 * q + 0] = v.x; w[j][4 * q + 1] = v.y; w[j][4 * q + 2] = v.z; w[j][4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int mm = 0; mm < PS_MC; ++mm) {
                const int m = mc + mm;
                w[j][mm] = buf_load1(rw, (active && m < M) ? ((unsigned)(col0 + j) * (unsigned)M + (unsigned)m) * 4u : OOB_OFF);
            }
        }
    }
}

// sv[mm] = sw_row[mc + mm] (0 past M): wave-uniform addresses -> scalar loads; the index is clamped into the row so that
// nothing past the tensor is read
template <int MT>
static __device__ __forceinline__ void ps_load_sw(float (&sv)[PS_MC], const float* __restrict__ row, int M, int mc) {
#pragma unroll
    for (int mm = 0; mm < PS_MC; ++mm) {
        if (MT == PS_MC) {
            sv[mm] = row[mm];
        } else {
            const int m = mc + mm;
            const float v = row[m < M ? m : M - 1];
            sv[mm] = m < M ? v : 0.f;
        }
    }
}

struct PsGeom { int B, N, M, H, nchunk, rpc, act; };

// The unit of this wave: sample b, rows [r0, r1), column quad col0 (active = inside H).  False: nothing to do.
static __device__ __forceinline__ bool ps_unit(const PsGeom& g, int& b, int& c, int& r0, int& r1, int& col0, bool& active) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int cidx = (int)blockIdx.y * PS_WAVES + wave;
    if (cidx >= g.B * g.nchunk) return false;
    b = cidx / g.nchunk;
    c = cidx - b * g.nchunk;
    r0 = c * g.rpc;
    r1 = min(g.N, r0 + g.rpc);
    col0 = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    active = col0 < g.H;
    return true;
}

// pre[rr][j] = tb[b][col0 + j] + sum_m sw[row rr][m] Wsw[col0 + j][m] for the PS_RT rows r .. r + PS_RT - 1 (rows past
// r1 repeat row r1 - 1: the caller masks them).  `w` holds chunk 0 on entry when hoisted (MT == 16 or nmc == 1).
template <int MT>
static __device__ __forceinline__ void ps_pre(float (&pre)[PS_RT][4], float (&w)[4][PS_MC], const float4 t4,
                                              __amdgpu_buffer_rsrc_t rw, const float* __restrict__ swb, int r, int r1,
                                              int col0, bool active, int M, int nmc) {
#pragma unroll
    for (int rr = 0; rr < PS_RT; ++rr) { pre[rr][0] = t4.x; pre[rr][1] = t4.y; pre[rr][2] = t4.z; pre[rr][3] = t4.w; }
    for (int ic = 0; ic < nmc; ++ic) {
        if (MT != PS_MC && nmc > 1) ps_load_w<MT>(w, rw, col0, M, ic * PS_MC, active);
#pragma unroll
        for (int rr = 0; rr < PS_RT; ++rr) {
            const int row = min(r + rr, r1 - 1);
            float sv[PS_MC];
            ps_load_sw<MT>(sv, swb + (size_t)row * M, M, ic * PS_MC);
#pragma unroll
            for (int mm = 0; mm < PS_MC; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) pre[rr][j] = fmaf(sv[mm], w[j][mm], pre[rr][j]);
        }
    }
}

template <int MT>
__global__ __launch_bounds__(PS_THREADS) void ps_fwd_kernel(const float* __restrict__ sw, const float* __restrict__ wsw,
                                                            const float* __restrict__ tb, float* __restrict__ h0,
                                                            const PsGeom g) {
    int b, c, r0, r1, col0;
    bool active;
    if (!ps_unit(g, b, c, r0, r1, col0, active)) return;
    const int M = MT ? MT : g.M, H = g.H, N = g.N;
    const int nmc = MT ? 1 : (M + PS_MC - 1) / PS_MC;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(wsw, (unsigned)((size_t)H * M * 4));
    const __amdgpu_buffer_rsrc_t rt = make_rsrc(tb, (unsigned)((size_t)g.B * H * 4));
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(h0, (unsigned)((size_t)g.B * N * H * 4));
    const float4 t4 = buf_load4(rt, active ? ((unsigned)b * (unsigned)H + (unsigned)col0) * 4u : OOB_OFF);
    float w[4][PS_MC];
    if (MT == PS_MC || nmc == 1) ps_load_w<MT>(w, rw, col0, M, 0, active);
    const float* swb = sw + (size_t)b * N * M;
    for (int r = r0; r < r1; r += PS_RT) {
        float pre[PS_RT][4];
        ps_pre<MT>(pre, w, t4, rw, swb, r, r1, col0, active, M, nmc);
#pragma unroll
        for (int rr = 0; rr < PS_RT; ++rr) {
            const float4 o = make_float4(act_fwd(g.act, pre[rr][0]), act_fwd(g.act, pre[rr][1]), act_fwd(g.act, pre[rr][2]),
                                         act_fwd(g.act, pre[rr][3]));
            const unsigned off = (unsigned)((((size_t)b * N + (r + rr)) * H + col0) * 4);
            buf_store4(ro, (active && r + rr < r1) ? off : OOB_OFF, o);
        }
    }
}

// Records (floats): dW part [B nchunk][H][M] at rec_w, then dtb part [nchunk][B][H] at rec_t.  grid.z = 16-column chunk
// of dWsw this wave accumulates (slice 0 also writes the dtb record).
template <int MT>
__global__ __launch_bounds__(PS_THREADS) void ps_bwd_kernel(const float* __restrict__ dh0, const float* __restrict__ sw,
                                                            const float* __restrict__ wsw, const float* __restrict__ tb,
                                                            float* __restrict__ rec_w, float* __restrict__ rec_t,
                                                            const PsGeom g) {
    int b, c, r0, r1, col0;
    bool active;
    if (!ps_unit(g, b, c, r0, r1, col0, active)) return;
    const int M = MT ? MT : g.M, H = g.H, N = g.N;
    const int nmc = MT ? 1 : (M + PS_MC - 1) / PS_MC;
    const int zc = MT ? 0 : (int)blockIdx.z;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(wsw, (unsigned)((size_t)H * M * 4));
    const __amdgpu_buffer_rsrc_t rt = make_rsrc(tb, (unsigned)((size_t)g.B * H * 4));
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(dh0, (unsigned)((size_t)g.B * N * H * 4));
    const float4 t4 = buf_load4(rt, active ? ((unsigned)b * (unsigned)H + (unsigned)col0) * 4u : OOB_OFF);
    float w[4][PS_MC];
    if (MT == PS_MC || nmc == 1) ps_load_w<MT>(w, rw, col0, M, 0, active);
    const float* swb = sw + (size_t)b * N * M;
    float dw[4][PS_MC], dt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mm = 0; mm < PS_MC; ++mm) dw[j][mm] = 0.f;
    for (int r = r0; r < r1; r += PS_RT) {
        float4 d4[PS_RT];
#pragma unroll
        for (int rr = 0; rr < PS_RT; ++rr) {           // rows past r1 load 0: they add nothing below
            const unsigned off = (unsigned)((((size_t)b * N + (r + rr)) * H + col0) * 4);
            d4[rr] = buf_load4(rd, (active && r + rr < r1) ? off : OOB_OFF);
        }
        float pre[PS_RT][4];
        ps_pre<MT>(pre, w, t4, rw, swb, r, r1, col0, active, M, nmc);
#pragma unroll
        for (int rr = 0; rr < PS_RT; ++rr) {
            float dp[4];
            dp[0] = d4[rr].x * act_bwd(g.act, pre[rr][0]);
            dp[1] = d4[rr].y * act_bwd(g.act, pre[rr][1]);
            dp[2] = d4[rr].z * act_bwd(g.act, pre[rr][2]);
            dp[3] = d4[rr].w * act_bwd(g.act, pre[rr][3]);
            if (r + rr >= r1) { dp[0] = 0.f; dp[1] = 0.f; dp[2] = 0.f; dp[3] = 0.f; }
            const int row = min(r + rr, r1 - 1);
            float sv[PS_MC];
            ps_load_sw<MT>(sv, swb + (size_t)row * M, M, zc * PS_MC);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dt[j] += dp[j];
#pragma unroll
                for (int mm = 0; mm < PS_MC; ++mm) dw[j][mm] = fmaf(dp[j], sv[mm], dw[j][mm]);
            }
        }
    }
    if (!active) return;
    float* pw = rec_w + ((size_t)(b * g.nchunk + c) * H + col0) * M;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (MT == PS_MC) {
#pragma unroll
            for (int q = 0; q < PS_MC / 4; ++q)
                *reinterpret_cast<float4*>(pw + j * PS_MC + 4 * q) =
                    make_float4(dw[j][4 * q], dw[j][4 * q + 1], dw[j][4 * q + 2], dw[j][4 * q + 3]);
        } else {
#pragma unroll
            for (int mm = 0; mm < PS_MC; ++mm) {
                const int m = zc * PS_MC + mm;
                if (m < M) pw[(size_t)j * M + m] = dw[j][mm];
            }
        }
    }
    if (zc == 0)
        *reinterpret_cast<float4*>(rec_t + ((size_t)c * g.B + b) * H + col0) = make_float4(dt[0], dt[1], dt[2], dt[3]);
}

static const unsigned long long PS_EXTENT = 1ull << 32;        // bytes a buffer descriptor / 32-bit offset covers

// PA2D_OK, or why this shape is refused
static int ps_check(int B, int N, int M, int H, int act) {
    if (B < 0 || N < 0 || M < 1 || H < 1 || act < ACT_NONE || act > ACT_SILU) return PA2D_ERR_ARG;
    if (M > PS_MAX_M || H % 4) return PA2D_ERR_UNSUPPORTED;
    const unsigned long long R = (unsigned long long)B * (unsigned long long)N;
    if (R * H * 4 >= PS_EXTENT || R * M * 4 >= PS_EXTENT || (unsigned long long)B * H * 4 >= PS_EXTENT ||
        (unsigned long long)H * M * 4 >= PS_EXTENT)
        return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}
static bool ps_grid(int B, int N, int rows, PsGeom& g, dim3& grid, int H) {
    g.rpc = rows;
    g.nchunk = ceil_div(N, rows);
    const long long units = (long long)B * g.nchunk;
    const long long gy = ceil_div_ll(units, PS_WAVES);
    if (gy > 65535) return false;
    grid = dim3((unsigned)ceil_div(H, 256), (unsigned)gy, 1);
    return true;
}

extern "C" {

size_t pa2d_prev_slice_entry_workspace(int B, int N, int M, int H) {
    if (B <= 0 || N <= 0 || M < 1 || H < 1) return 0;
    const size_t nchunk = (size_t)ceil_div(N, PS_ROWS_BWD);
    return sizeof(float) * (size_t)B * nchunk * ((size_t)H * M + (size_t)H);
}

int pa2d_prev_slice_entry_fwd(const float* sw, const float* wsw, const float* tb, float* h0, int B, int N, int M, int H,
                              int act, hipStream_t st) {
    const int rc = ps_check(B, N, M, H, act);
    if (rc != PA2D_OK) return rc;
    if (B == 0 || N == 0) return PA2D_OK;
    if (!sw || !wsw || !tb || !h0) return PA2D_ERR_ARG;
    if ((((uintptr_t)wsw) | ((uintptr_t)tb) | ((uintptr_t)h0)) & 15 || ((uintptr_t)sw & 3)) return PA2D_ERR_ARG;
    PsGeom g = {B, N, M, H, 0, 0, act};
    dim3 grid;
    if (!ps_grid(B, N, PS_ROWS_FWD, g, grid, H)) return PA2D_ERR_UNSUPPORTED;
    if (M == PS_MC)
        hipLaunchKernelGGL(ps_fwd_kernel<PS_MC>, grid, dim3(PS_THREADS), 0, st, sw, wsw, tb, h0, g);
    else
        hipLaunchKernelGGL(ps_fwd_kernel<0>, grid, dim3(PS_THREADS), 0, st, sw, wsw, tb, h0, g);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// dwsw [H, M] and dtb [B, H] are overwritten (zero-filled when B N == 0); ws: pa2d_prev_slice_entry_workspace bytes
int pa2d_prev_slice_entry_bwd(const float* dh0, const float* sw, const float* wsw, const float* tb, float* dwsw,
                              float* dtb, void* ws, size_t ws_bytes, int B, int N, int M, int H, int act,
                              hipStream_t st) {
    int rc = ps_check(B, N, M, H, act);
    if (rc != PA2D_OK) return rc;
    if (!dwsw || !dtb) return PA2D_ERR_ARG;
    if (B == 0 || N == 0) {
        rc = pa2d_zero(dwsw, sizeof(float) * (size_t)H * M, st);
        if (rc == PA2D_OK) rc = pa2d_zero(dtb, sizeof(float) * (size_t)B * H, st);
        return rc;
    }
    if (!dh0 || !sw || !wsw || !tb || !ws) return PA2D_ERR_ARG;
    if ((((uintptr_t)wsw) | ((uintptr_t)tb) | ((uintptr_t)dh0) | ((uintptr_t)ws)) & 15 || ((uintptr_t)sw & 3))
        return PA2D_ERR_ARG;
    if (ws_bytes < pa2d_prev_slice_entry_workspace(B, N, M, H)) return PA2D_ERR_WORKSPACE;
    PsGeom g = {B, N, M, H, 0, 0, act};
    dim3 grid;
    if (!ps_grid(B, N, PS_ROWS_BWD, g, grid, H)) return PA2D_ERR_UNSUPPORTED;
    float* rec_w = (float*)ws;
    float* rec_t = rec_w + (size_t)B * g.nchunk * H * M;
    if (M == PS_MC) {
        hipLaunchKernelGGL(ps_bwd_kernel<PS_MC>, grid, dim3(PS_THREADS), 0, st, dh0, sw, wsw, tb, rec_w, rec_t, g);
    } else {
        grid.z = (unsigned)ceil_div(M, PS_MC);
        hipLaunchKernelGGL(ps_bwd_kernel<0>, grid, dim3(PS_THREADS), 0, st, dh0, sw, wsw, tb, rec_w, rec_t, g);
    }
    PA2D_CHECK_LAUNCH();
    ReduceSegs sw_ = {1, {0, (long long)H * M, 0, 0, 0}, {dwsw, nullptr, nullptr, nullptr}};
    rc = pa2d_launch_reduce_segs(rec_w, B * g.nchunk, (long long)H * M, sw_, 0, st);
    if (rc != PA2D_OK) return rc;
    ReduceSegs st_ = {1, {0, (long long)B * H, 0, 0, 0}, {dtb, nullptr, nullptr, nullptr}};
    return pa2d_launch_reduce_segs(rec_t, g.nchunk, (long long)B * H, st_, 0, st);
}

}  // extern "C"
