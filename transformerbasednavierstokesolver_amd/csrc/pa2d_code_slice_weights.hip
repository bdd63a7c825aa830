// Slice weights predicted from the code (reference SequenSolver.py:159-170, the use_gt=False branch): the reference fills a
// [B, N, M, C+2] tensor whose row (n, m) is cat(code[b, 0, m, :], pos[b, n, :2]) in a Python loop over the N points, runs
// weight_projection = MLP(C+2, 64, 1) (n_layers=1, res=True) on it and takes a softmax over the M slices:
//
//   a[n,m,:]  = W1 [code_m ; pos_n] + b1 = (W1c code_m + b1) + W1p pos_n      W1 = [W1c | W1p]  [64, C+2]
//   h = gelu(a),   u = h + gelu(W2 h + b2),   logit[n,m] = w3 . u + b3,   sw[b,0,n,:] = softmax_m(logit[n,:])
//
// Here the concatenated tensor never exists: the first layer separates into a table tb[m, 64] = W1c code_m + b1 per sample
// (made by every workgroup in LDS: M*64*C FMAs, the work of C/67 points) and a rank-2 term per point.  A thread owns one
// (point, slice) row: its 64 hidden values live in registers, the 64x64 layer (the FLOPs: 2*64*64 per row) is 64 dot
// products against rows of W2 that every lane reads at the same address (scalar loads), the softmax over the M rows of a
// point goes through LDS, so any 1 <= M <= 128 is served without padding to a power of two.
//
// Backward (one kernel plus three small deterministic reduce passes): the forward is recomputed per tile of 128 rows; h and
// the pre-activations z = W2 h + b2 are kept in LDS as [64][rows] tiles, turned into dz = dl w3 gelu'(z) in place, and
//   dW2 += dz^T h          (every thread owns a 4 x 8 block of the 64 x 64 matrix and walks the rows of the tile)
//   dh = dl w3 + dz W2,  da = dh gelu'(a),   dtb[m, :] += da   (LDS table, each element owned by one thread)
//   db2, dw3, db3, dW1p    wave butterfly sums, added to per-wave LDS accumulators by lane 0
// One partial-sum record per workgroup, summed in a fixed order (fp64 in the three small passes); then dcode = dtb W1c, dW1c = sum_(b,m) dtb^T code,
// db1 = sum_(b,m) dtb.  The positions get no gradient.  Exact fp32 FMA on the VALU on every engine: no engine argument.
#include "pa2d_code_sw_common.h"

namespace {

constexpr int FNT = 256;         // forward: threads = rows per tile
constexpr int BNT = 128;         // backward: threads = rows per tile
constexpr int RS = BNT + 4;      // pitch of the [64][rows] tiles (16-byte aligned rows)
constexpr int B_DTB = 2 * HID;   // record B: dW1p [64*2] | dtb [M*64]
constexpr int NWACC = 4 * HID + 1;   // per-wave accumulators: dw3 [64] | db2 [64] | dW1p [128] | db3

// grid (chunks, B): the workgroup walks points [n0, n1) of sample b, NTH / M points per tile, one (point, slice) per thread
__global__ __launch_bounds__(FNT) void code_sw_fwd_kernel(const float* __restrict__ code, const float* __restrict__ pos,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          const float* __restrict__ w3, const float* __restrict__ b3,
                                                          float* __restrict__ sw, int N, int M, int C, int ppb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tb = smem;                  // [M][TS]
    float* lg = smem + M * TS;         // [FNT]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n0 = blockIdx.x * ppb, n1 = min(N, n0 + ppb);
    const int ldw = C + 2;
    make_table<FNT>(tb, code + (long long)b * M * C, w1, b1, M, C, ldw);
    const int PT = FNT / M;
    const bool active = tid < PT * M;
    const int pl = tid / M, m = active ? tid % M : 0;
    __syncthreads();
    for (int t0 = n0; t0 < n1; t0 += PT) {
        const int n = t0 + pl;
        const bool valid = active && n < n1;
        const float* pr = pos + ((long long)b * N + (valid ? n : n0)) * 2;
        const float px = pr[0], py = pr[1];
        float h[HID];
        float lp[4] = {b3[0], 0.f, 0.f, 0.f};        // four partial sums of the logit: short fp32 chains
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + fmaf(w1[j * ldw + C + 1], py, w1[j * ldw + C] * px);
            h[j] = gelu_tail(a);
            lp[j & 3] = fmaf(w3[j], h[j], lp[j & 3]);
        }
        for (int k0 = 0; k0 < HID; k0 += 4) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = k0 + kk;
                lp[kk] = fmaf(w3[k], gelu_tail(hidden_dot(w2 + k * HID, b2[k], h)), lp[kk]);
            }
        }
        const float logit = (lp[0] + lp[1]) + (lp[2] + lp[3]);
        lg[tid] = logit;
        __syncthreads();
        if (valid) {
            const float* l = lg + pl * M;
            float mx = l[0];
            for (int i = 1; i < M; ++i) mx = fmaxf(mx, l[i]);
            float s = 0.f;
            for (int i = 0; i < M; ++i) s += expf(l[i] - mx);
            sw[((long long)b * N + n) * M + m] = expf(logit - mx) / s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BNT) void code_sw_bwd_kernel(const float* __restrict__ code, const float* __restrict__ pos,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          const float* __restrict__ w3, const float* __restrict__ b3,
                                                          const float* __restrict__ dsw, float* __restrict__ rec_a,
                                                          float* __restrict__ rec_b, int N, int M, int C, int ppb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* hs = smem;                          // [HID][RS]   h of the tile's rows
    float* zs = hs + HID * RS;                 // [HID][RS]   z, then dz, then da
    float* tb = zs + HID * RS;                 // [M][TS]
    float* dtb = tb + M * TS;                  // [M][HID]
    float* lg = dtb + M * HID;                 // [BNT]
    float* dsl = lg + BNT;                     // [BNT]
    float* wacc = dsl + BNT;                   // [2 waves][NWACC]
    const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * ppb, n1 = min(N, n0 + ppb);
    const int ldw = C + 2;
    make_table<BNT>(tb, code + (long long)b * M * C, w1, b1, M, C, ldw);
    for (int e = tid; e < M * HID; e += BNT) dtb[e] = 0.f;
    for (int e = tid; e < 2 * NWACC; e += BNT) wacc[e] = 0.f;
    const int PT = BNT / M;
    const bool active = tid < PT * M;
    const int pl = tid / M, m = active ? tid % M : 0;
    const int kb = (tid / 8) * 4, jb = (tid % 8) * 8;      // this thread's 4 x 8 block of dW2
    float* wa = wacc + wave * NWACC;
    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int t0 = n0; t0 < n1; t0 += PT) {
        __syncthreads();                       // the previous tile's readers are done (first tile: tb, dtb, wacc are staged)
        const int n = t0 + pl;
        const bool valid = active && n < n1;
        const float* pr = pos + ((long long)b * N + (valid ? n : n0)) * 2;
        const float px = pr[0], py = pr[1];
        float dh[HID];                         // h, later dh and da
        float lp[4] = {b3[0], 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + fmaf(w1[j * ldw + C + 1], py, w1[j * ldw + C] * px);
            dh[j] = gelu_tail(a);
            hs[j * RS + tid] = dh[j];
            lp[j & 3] = fmaf(w3[j], dh[j], lp[j & 3]);
        }
        for (int k0 = 0; k0 < HID; k0 += 4) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = k0 + kk;
                const float z = hidden_dot(w2 + k * HID, b2[k], dh);
                zs[k * RS + tid] = z;
                lp[kk] = fmaf(w3[k], gelu_tail(z), lp[kk]);
            }
        }
        const float logit = (lp[0] + lp[1]) + (lp[2] + lp[3]);
        lg[tid] = logit;
        dsl[tid] = valid ? dsw[((long long)b * N + n) * M + m] : 0.f;
        __syncthreads();
        // softmax backward of this row: dl = p (dsw - <p, dsw>); rows outside the tile carry dl = 0 and add nothing below
        float dl = 0.f;
        if (valid) {
            const float* l = lg + pl * M;
            const float* g = dsl + pl * M;
            float mx = l[0];
            for (int i = 1; i < M; ++i) mx = fmaxf(mx, l[i]);
            // g_r - <p, g> written as sum_i p_i (g_r - g_i) (sum p = 1): a dominant slice (p_r near 1) loses nothing to
            // the cancellation of g_r against <p, g>
            const float gr = dsl[tid];
            float s = 0.f, sd = 0.f;
            for (int i = 0; i < M; ++i) {
                const float e = expf(l[i] - mx);
                s += e;
                sd = fmaf(e, gr - g[i], sd);
            }
            dl = expf(logit - mx) / s * (sd / s);
        }
        float dh2[HID];                        // the odd k's partial sums of dh: two chains of 32 instead of one of 64
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            dh[j] = dl * w3[j];
            dh2[j] = 0.f;
        }
        for (int k0 = 0; k0 < HID; k0 += 2) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int k = k0 + kk;
                const float z = zs[k * RS + tid];
                float g, dg;
                gelu_both(z, g, dg);
                const float u = hs[k * RS + tid] + g;
                const float dz = dl * w3[k] * dg;
                zs[k * RS + tid] = dz;
                const float s1 = wave_sum(dl * u), s2 = wave_sum(dz);
                if (lane == 0) {
                    wa[k] += s1;
                    wa[HID + k] += s2;
                }
                if (kk == 0) {
#pragma unroll
                    for (int j = 0; j < HID; ++j) dh[j] = fmaf(dz, w2[k * HID + j], dh[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < HID; ++j) dh2[j] = fmaf(dz, w2[k * HID + j], dh2[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < HID; ++j) dh[j] += dh2[j];
        {
            const float s3 = wave_sum(dl);
            if (lane == 0) wa[4 * HID] += s3;
        }
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + fmaf(w1[j * ldw + C + 1], py, w1[j * ldw + C] * px);
            dh[j] *= dgelu_tail(a);
            const float s4 = wave_sum(dh[j] * px), s5 = wave_sum(dh[j] * py);
            if (lane == 0) {
                wa[2 * HID + 2 * j] += s4;
                wa[2 * HID + 2 * j + 1] += s5;
            }
        }
        __syncthreads();                       // every row's dz is in zs
        for (int r = 0; r < BNT; r += 4) {
            float4 zv[4], hv[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) zv[i] = *reinterpret_cast<const float4*>(zs + (kb + i) * RS + r);
#pragma unroll
            for (int j = 0; j < 8; ++j) hv[j] = *reinterpret_cast<const float4*>(hs + (jb + j) * RS + r);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float s = acc[i][j];
                    s = fmaf(zv[i].x, hv[j].x, s);
                    s = fmaf(zv[i].y, hv[j].y, s);
                    s = fmaf(zv[i].z, hv[j].z, s);
                    s = fmaf(zv[i].w, hv[j].w, s);
                    acc[i][j] = s;
                }
        }
        __syncthreads();                       // dz is consumed: the tile now takes da
#pragma unroll
        for (int j = 0; j < HID; ++j) zs[j * RS + tid] = dh[j];
        __syncthreads();
        for (int e = tid; e < M * HID; e += BNT) {
            const int mm = e / HID, j = e % HID;
            float s = dtb[e];
            for (int p = 0; p < PT; ++p) s += zs[j * RS + p * M + mm];
            dtb[e] = s;
        }
    }
    __syncthreads();
    const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    float* ra = rec_a + blk * REC_A;
    float* rb = rec_b + blk * (B_DTB + M * HID);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) ra[(kb + i) * HID + jb + j] = acc[i][j];
    if (tid < HID) {
        ra[A_DW3 + tid] = wacc[tid] + wacc[NWACC + tid];
        ra[A_DB2 + tid] = wacc[HID + tid] + wacc[NWACC + HID + tid];
    }
    rb[tid] = wacc[2 * HID + tid] + wacc[NWACC + 2 * HID + tid];        // BNT == 2 * HID: dW1p
    if (tid == 0) {
        ra[A_DB3] = wacc[4 * HID] + wacc[NWACC + 4 * HID];
        ra[A_END] = ra[A_END + 1] = ra[A_END + 2] = 0.f;
    }
    for (int e = tid; e < M * HID; e += BNT) rb[B_DTB + e] = dtb[e];
}

// dtbf[b][e] = sum over the nx records of sample b, in a fixed order
__global__ __launch_bounds__(256) void code_sw_dtb_reduce_kernel(const float* __restrict__ rec_b, float* __restrict__ dtbf,
                                                                 long long total, int MH, int nx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / MH, e = i % MH;
    const long long rec = B_DTB + MH;
    dtbf[i] = (float)strided_sum(rec_b + b * nx * rec + B_DTB + e, nx, rec);
}

// element ranges: [0, B*M*C) dcode = dtb W1c (plain store; skipped when dcode is NULL); then 64 * (C+3) parameter elements
// (j, c): c < C dW1c = sum_(b,m) dtb[b,m,j] code[b,m,c]; c = C, C+1 dW1p from the records; c = C+2: db1 = sum_(b,m) dtb
__global__ __launch_bounds__(256) void code_sw_finish_kernel(const float* __restrict__ code, const float* __restrict__ w1,
                                                             const float* __restrict__ dtbf, const float* __restrict__ rec_b,
                                                             float* __restrict__ dcode, float* __restrict__ dw1,
                                                             float* __restrict__ db1, int B, int M, int C, int nrec,
                                                             int accumulate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ncode = (long long)B * M * C;
    const int ldw = C + 2;
    if (i < ncode) {
        if (!dcode) return;
        const long long bm = i / C;
        const int c = (int)(i % C);
        double s = 0.0;
        for (int j = 0; j < HID; ++j) s = fma((double)dtbf[bm * HID + j], (double)w1[j * ldw + c], s);
        dcode[i] = (float)s;
        return;
    }
    const long long e = i - ncode;
    if (e >= (long long)HID * (C + 3)) return;
    const int j = (int)(e / (C + 3)), c = (int)(e % (C + 3));
    double s = 0.0;
    float* dst;
    if (c < C) {
        for (int bm = 0; bm < B * M; ++bm) s = fma((double)dtbf[(long long)bm * HID + j], (double)code[(long long)bm * C + c], s);
        dst = dw1 + j * ldw + c;
    } else if (c < C + 2) {
        const long long rec = B_DTB + (long long)M * HID;
        s = strided_sum(rec_b + 2 * j + (c - C), nrec, rec);
        dst = dw1 + j * ldw + c;
    } else {
        s = strided_sum(dtbf + j, B * M, HID);
        dst = db1 + j;
    }
    *dst = accumulate ? *dst + (float)s : (float)s;
}

// ------------------------------------------------------------------------------------------------ host side
int check_shape(int B, int N, int M, int C, int hidden, int depth) {
    if (C != 8 && C != 16 && C != 32 && C != 64) return PA2D_ERR_UNSUPPORTED;
    if (M < 1 || M > 128) return PA2D_ERR_UNSUPPORTED;
    if (hidden != HID || depth != 1) return PA2D_ERR_UNSUPPORTED;
    if (B < 0 || N < 1) return PA2D_ERR_ARG;
    if ((unsigned long long)B * N * M * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}

constexpr int FWD_TARGET = 2048, BWD_TARGET = 512;

size_t fwd_lds(int M) { return sizeof(float) * ((size_t)M * TS + FNT); }
size_t bwd_lds(int M) { return sizeof(float) * (2 * (size_t)HID * RS + (size_t)M * TS + (size_t)M * HID + 2 * BNT + 2 * NWACC); }

}  // namespace

extern "C" {

int pa2d_code_slice_weights_fwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, float* sw, int B, int N, int M, int C,
                                int hidden, int depth, void* stream, void* ev_start, void* ev_stop) {
    const int rc = check_shape(B, N, M, C, hidden, depth);
    if (rc) return rc;
    if (B == 0) return PA2D_OK;
    if (!code || !pos || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !sw) return PA2D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ppb = points_per_block(B, N, FNT / M, FWD_TARGET);
    const dim3 grid(ceil_div(N, ppb), B);
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
    hipLaunchKernelGGL(code_sw_fwd_kernel, grid, dim3(FNT), fwd_lds(M), st, code, pos, w1, b1, w2, b2, w3, b3, sw, N, M, C, ppb);
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

size_t pa2d_code_slice_weights_bwd_workspace(int B, int N, int M, int C) {
    if (check_shape(B, N, M, C, HID, 1) || B == 0) return 0;
    const int ppb = points_per_block(B, N, BNT / M, BWD_TARGET);
    const size_t nrec = (size_t)ceil_div(N, ppb) * B;
    return sizeof(float) * (nrec * (REC_A + B_DTB + (size_t)M * HID) + (size_t)B * M * HID);
}

int pa2d_code_slice_weights_bwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, const float* dsw, float* dcode,
                                float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ws_buf,
                                size_t ws_bytes, int B, int N, int M, int C, int hidden, int depth, int accumulate,
                                void* stream, void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, M, C, hidden, depth);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (accumulate) return PA2D_OK;
        if ((rc = pa2d_zero(dw1, sizeof(float) * HID * (C + 2), st))) return rc;
        if ((rc = pa2d_zero(db1, sizeof(float) * HID, st))) return rc;
        if ((rc = pa2d_zero(dw2, sizeof(float) * HID * HID, st))) return rc;
        if ((rc = pa2d_zero(db2, sizeof(float) * HID, st))) return rc;
        if ((rc = pa2d_zero(dw3, sizeof(float) * HID, st))) return rc;
        return pa2d_zero(db3, sizeof(float), st);
    }
    if (!code || !pos || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !dsw) return PA2D_ERR_ARG;
    if (!dw1 || !db1 || !dw2 || !db2 || !dw3 || !db3) return PA2D_ERR_ARG;
    if (ws_bytes < pa2d_code_slice_weights_bwd_workspace(B, N, M, C) || !ws_buf) return PA2D_ERR_WORKSPACE;
    const int ppb = points_per_block(B, N, BNT / M, BWD_TARGET);
    const int nx = ceil_div(N, ppb), nrec = nx * B;
    const int MH = M * HID;
    float* rec_a = (float*)ws_buf;
    float* rec_b = rec_a + (size_t)nrec * REC_A;
    float* dtbf = rec_b + (size_t)nrec * (B_DTB + MH);
    const size_t lds = bwd_lds(M);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&code_sw_bwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
    hipLaunchKernelGGL(code_sw_bwd_kernel, dim3(nx, B), dim3(BNT), lds, st, code, pos, w1, b1, w2, b2, w3, b3, dsw, rec_a,
                       rec_b, N, M, C, ppb);
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    const long long total = (long long)B * MH;
    hipLaunchKernelGGL(code_sw_dtb_reduce_kernel, dim3((unsigned)ceil_div_ll(total, 256)), dim3(256), 0, st, rec_b, dtbf,
                       total, MH, nx);
    PA2D_CHECK_LAUNCH();
    const long long nfin = (long long)B * M * C + (long long)HID * (C + 3);
    hipLaunchKernelGGL(code_sw_finish_kernel, dim3((unsigned)ceil_div_ll(nfin, 256)), dim3(256), 0, st, code, w1, dtbf, rec_b,
                       dcode, dw1, db1, B, M, C, nrec, accumulate);
    PA2D_CHECK_LAUNCH();
    ReduceSegs segs;
    segs.nseg = 4;
    segs.begin[0] = 0; segs.begin[1] = A_DB2; segs.begin[2] = A_DW3; segs.begin[3] = A_DB3; segs.begin[4] = A_END;
    segs.dst[0] = dw2; segs.dst[1] = db2; segs.dst[2] = dw3; segs.dst[3] = db3;
    return pa2d_launch_reduce_segs(rec_a, nrec, REC_A, segs, accumulate, st);
}

}  // extern "C"
