// Slice weights from the code and P point features: the one implementation behind pa2d_point_slice_weights_* (reference
// LearnSlice.py:41-153, class LearnSlice: `forward` runs weight_projection = MLP(C+P, 64, 1) on cat(code [M, C], point
// features expanded to [M, P]) with a softmax over the M slices, `get_slice_weight` calls it in a Python loop over the N
// points; train() (:477-526) sums F.mse_loss over the points) and pa2d_code_slice_weights_* (reference SequenSolver.py:159-170,
// the use_gt=False branch, which fills a [B, N, M, C+2] tensor in such a loop: the two point coordinates are P = 2 features):
//
//   a[n,m,:]  = W1 [code_m ; feat_n] + b1 = (W1c code_m + b1) + W1p feat_n      W1 = [W1c | W1p]  [64, C+P]
//   h = gelu(a),   u = h + gelu(W2 h + b2),   logit[n,m] = w3 . u + b3,   sw[b,0,n,:] = softmax_m(logit[n,:])
//
// P is 2 (coordinates), 64 (unified_pos distances), 74 (distances and T = 10 frames) or 12 in the reference; 1 <= P <= 128
// is served.  The concatenated tensor never exists: the first layer separates into a table tb[m, 64] = W1c code_m + b1 per
// sample (made by every workgroup in LDS: M*64*C FMAs, the work of C/67 points) and the point term.  A thread owns one
// (point, slice) row: its 64 hidden values live in registers, the 64x64 layer (the FLOPs: 2*64*64 per row) is 64 dot products
// against rows of W2 that every lane reads at the same address (scalar loads), the softmax over the M rows of a point goes
// through LDS, so any 1 <= M <= 128 is served without padding to a power of two.  The point term W1p feat_n is 64 P FMAs, at
// P = 74 more than the 64x64 layer of a row, so it is made ONCE PER POINT into a table pf[points of the tile][64] in LDS
// (every thread makes a few entries; 64 P FMAs per point, P / (64 M) of the tile's row work); rows then read
// a = tb[m] + pf[point].  The forward keeps W1p transposed in LDS ([P][64]: lane j reads column j without a bank conflict).
//
// Backward: a first small kernel makes the same table for all points into the workspace (pfw[b,n,:], 256 B per point; the
// main kernel's LDS and registers are taken by the h / z tiles and the dW2 block: with the table's dot products inlined it
// no longer compiles without a scratch reservation).  The main kernel recomputes the forward per tile of 128 rows; h and the
// pre-activations z = W2 h + b2 are kept in LDS as [64][rows] tiles, turned into dz = dl w3 gelu'(z) in place, and
//   dW2 += dz^T h          (every thread owns a 4 x 8 block of the 64 x 64 matrix and walks the rows of the tile)
//   dh = dl w3 + dz W2,  da = dh gelu'(a),   dtb[m, :] += da   (LDS table, each element owned by one thread)
//   db2, dw3, db3          wave butterfly sums, added to per-wave LDS accumulators by lane 0
// It copies its tile's rows of pfw to LDS and, at the end of the tile, overwrites the same rows with
// dpf[b,n,:] = sum_m da[n,m,:] (plain store; a workgroup owns its points).  A third kernel forms
// dW1p[64, P] = sum_(b,n) dpf[b,n,:]^T feat[b,n,:] over fixed ranges of points, one record per workgroup.  One partial-sum
// record per workgroup of the main kernel; all records are summed in a fixed order (fp64 in the small passes), then
// dcode = dtb W1c, dW1c = sum_(b,m) dtb^T code, db1 = sum_(b,m) dtb.  The features get no gradient.  No float atomics
// anywhere.  Exact fp32 FMA on the VALU on every engine: no engine argument.
//
// The loss stage (LearnSlice.py:499-510): loss = sum_(b,n) (1/M) sum_m (sw - target)^2, dsw = g 2/M (sw - target).
#include "pa2d_internal.h"

namespace {

constexpr int HID = 64;          // hidden width of weight_projection (the only one the reference builds)
constexpr int TS = HID + 1;      // pitch of the first-layer table: lanes read different rows at one column
constexpr int REC_A = 4228;      // record A: dW2 [64*64] | db2 [64] | dw3 [64] | db3 [1] | pad
constexpr int A_DB2 = 4096, A_DW3 = 4160, A_DB3 = 4224, A_END = 4225;

// GELU with a normal cdf that keeps its RELATIVE accuracy in the lower tail (0.5 erfc(-x / sqrt 2)): the gradient of a
// slice whose first-layer pre-activations sit at -3 and below is made of such tail values, and the rational erfc of
// pa2d_internal.h (absolute error 1.5e-7, the activation of the GEMM epilogues) is 1e-3 off in relative terms there.
__device__ __forceinline__ float cdf_tail(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }
__device__ __forceinline__ float gelu_tail(float x) { return x * cdf_tail(x); }
__device__ __forceinline__ float dgelu_tail(float x) {
    return fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), cdf_tail(x));
}
__device__ __forceinline__ void gelu_both(float x, float& g, float& dg) {
    const float c = cdf_tail(x);
    g = x * c;
    dg = fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), c);
}

// z = bias + w . h over the 64 hidden values, as four interleaved partial sums (the forward and the backward's recomputation
// share it, so both see the same bits); w is read at one address by every lane
__device__ __forceinline__ float hidden_dot(const float* __restrict__ w, float bias, const float (&h)[HID]) {
    float z0 = bias, z1 = 0.f, z2 = 0.f, z3 = 0.f;
#pragma unroll
    for (int j = 0; j < HID; j += 4) {
        z0 = fmaf(w[j], h[j], z0);
        z1 = fmaf(w[j + 1], h[j + 1], z1);
        z2 = fmaf(w[j + 2], h[j + 2], z2);
        z3 = fmaf(w[j + 3], h[j + 3], z3);
    }
    return (z0 + z1) + (z2 + z3);
}

// tb[m][j] = b1[j] + sum_c W1[j][c] code[b][m][c]; ldw = row pitch of W1 (C plus the width of the point part)
template <int NTH>
__device__ __forceinline__ void make_table(float* tb, const float* __restrict__ code_b, const float* __restrict__ w1,
                                           const float* __restrict__ b1, int M, int C, int ldw) {
    for (int e = threadIdx.x; e < M * HID; e += NTH) {
        const int m = e / HID, j = e % HID;
        const float* cr = code_b + m * C;
        const float* wr = w1 + j * ldw;
        float s0 = b1[j], s1 = 0.f, s2 = 0.f, s3 = 0.f;          // C % 8 == 0
        for (int c = 0; c < C; c += 4) {
            s0 = fmaf(wr[c], cr[c], s0);
            s1 = fmaf(wr[c + 1], cr[c + 1], s1);
            s2 = fmaf(wr[c + 2], cr[c + 2], s2);
            s3 = fmaf(wr[c + 3], cr[c + 3], s3);
        }
        tb[m * TS + j] = (s0 + s1) + (s2 + s3);
    }
}

// sum of n values at stride `st` in a fixed order, in fp64 (the second-stage sums are a few thousand additions in all)
__device__ __forceinline__ double strided_sum(const float* __restrict__ p, int n, long long st) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = 0;
    for (; c + 4 <= n; c += 4) {
        s0 += (double)p[c * st];
        s1 += (double)p[(c + 1) * st];
        s2 += (double)p[(c + 2) * st];
        s3 += (double)p[(c + 3) * st];
    }
    for (; c < n; ++c) s0 += (double)p[c * st];
    return (s0 + s1) + (s2 + s3);
}

constexpr int FNT = 256;         // forward: threads = rows per tile
constexpr int BNT = 128;         // backward: threads = rows per tile
constexpr int RS = BNT + 4;      // pitch of the [64][rows] tiles (16-byte aligned rows)
constexpr int NWACC = 2 * HID + 1;   // per-wave accumulators: dw3 [64] | db2 [64] | db3
constexpr int PMAX = 128;        // widest point feature row
constexpr int WNT = 256;         // dW1p kernel: threads
constexpr int WCOLS = PMAX / (WNT / HID);      // feature columns per thread of the dW1p kernel (32)
constexpr int WBLK = 64;         // dW1p kernel: points per inner fp32 chain
constexpr int W_TARGET = 512;    // dW1p kernel: about this many records
constexpr int TBL_CHUNK = 64;    // backward table kernel: points per workgroup
constexpr int MSE_NT = 256, MSE_MAXB = 256;

// out[p * pitch + j] = sum_c W1p[j][c] rows[p][c] for npt table rows, of which the first nvalid are consecutive rows of the
// features and the others repeat the last of them (finite values that no output depends on), four interleaved partial sums
// over c; W1p is read transposed from LDS (wt[c * HID + j]: lane j reads column j without a bank conflict).  The forward and
// the backward's table kernel share it, so both see the same bits.
template <int NTH>
__device__ __forceinline__ void make_point_table(float* out, int pitch, const float* __restrict__ rows, const float* wt, int P,
                                                 int npt, int nvalid) {
    for (int e = threadIdx.x; e < npt * HID; e += NTH) {
        const int p = e / HID, j = e % HID;
        const float* fr = rows + (long long)min(p, nvalid - 1) * P;
        const float* wr = wt + j;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int c = 0;
        for (; c + 4 <= P; c += 4) {
            s0 = fmaf(wr[c * HID], fr[c], s0);
            s1 = fmaf(wr[(c + 1) * HID], fr[c + 1], s1);
            s2 = fmaf(wr[(c + 2) * HID], fr[c + 2], s2);
            s3 = fmaf(wr[(c + 3) * HID], fr[c + 3], s3);
        }
        for (; c < P; ++c) s0 = fmaf(wr[c * HID], fr[c], s0);
        out[p * pitch + j] = (s0 + s1) + (s2 + s3);
    }
}

// wt[c][j] = W1[j][C + c]: consecutive threads read consecutive addresses of a row of W1
template <int NTH>
__device__ __forceinline__ void stage_w1p(float* wt, const float* __restrict__ w1, int C, int P) {
    for (int e = threadIdx.x; e < P * HID; e += NTH) {
        const int j = e / P, c = e % P;
        wt[c * HID + j] = w1[j * (C + P) + C + c];
    }
}

// grid (chunks, B): the workgroup walks points [n0, n1) of sample b, NTH / M points per tile, one (point, slice) per thread
__global__ __launch_bounds__(FNT) void point_sw_fwd_kernel(const float* __restrict__ code, const float* __restrict__ feat,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ w3, const float* __restrict__ b3,
                                                           float* __restrict__ sw, int N, int M, int C, int P, int ppb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int PT = FNT / M;
    float* tb = smem;                  // [M][TS]
    float* lg = tb + M * TS;           // [FNT]
    float* pf = lg + FNT;              // [PT][TS]
    float* wt = pf + PT * TS;          // [P][HID]   W1p transposed
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n0 = blockIdx.x * ppb, n1 = min(N, n0 + ppb);
    const int ldw = C + P;
    make_table<FNT>(tb, code + (long long)b * M * C, w1, b1, M, C, ldw);
    stage_w1p<FNT>(wt, w1, C, P);
    const float* feat_b = feat + (long long)b * N * P;
    const bool active = tid < PT * M;
    const int pl = active ? tid / M : 0, m = active ? tid % M : 0;
    for (int t0 = n0; t0 < n1; t0 += PT) {
        __syncthreads();               // the previous tile's readers of pf and lg are done (first tile: tb and wt are staged)
        make_point_table<FNT>(pf, TS, feat_b + (long long)t0 * P, wt, P, PT, n1 - t0);
        __syncthreads();
        const int n = t0 + pl;
        const bool valid = active && n < n1;
        float h[HID];
        float lp[4] = {b3[0], 0.f, 0.f, 0.f};        // four partial sums of the logit: short fp32 chains
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + pf[pl * TS + j];
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
    }
}

// backward, first pass: pfw[r, :] = W1p feat[r, :] for the flat rows r = b * N + n of [r0, r1) (the buffer that the main
// kernel later overwrites row by row with dpf)
__global__ __launch_bounds__(FNT) void point_sw_table_kernel(const float* __restrict__ feat, const float* __restrict__ w1,
                                                             float* __restrict__ pfw, long long total, int C, int P, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [P][HID]   W1p transposed
    stage_w1p<FNT>(smem, w1, C, P);
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * chunk;
    const int npt = (int)(r0 + chunk < total ? chunk : total - r0);
    make_point_table<FNT>(pfw + r0 * HID, HID, feat + r0 * P, smem, P, npt, npt);
}

__global__ __launch_bounds__(BNT) void point_sw_bwd_kernel(const float* __restrict__ code,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ w3, const float* __restrict__ b3,
                                                           const float* __restrict__ dsw, float* __restrict__ rec_a,
                                                           float* __restrict__ rec_b, float* dpf, int N, int M, int C, int P,
                                                           int ppb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int PT = BNT / M;
    float* hs = smem;                          // [HID][RS]   h of the tile's rows
    float* zs = hs + HID * RS;                 // [HID][RS]   z, then dz, then da
    float* tb = zs + HID * RS;                 // [M][TS]
    float* dtb = tb + M * TS;                  // [M][HID]
    float* lg = dtb + M * HID;                 // [BNT]
    float* dsl = lg + BNT;                     // [BNT]
    float* wacc = dsl + BNT;                   // [2 waves][NWACC]
    float* pf = wacc + 2 * NWACC;              // [PT][TS]
    const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * ppb, n1 = min(N, n0 + ppb);
    const int ldw = C + P;
    make_table<BNT>(tb, code + (long long)b * M * C, w1, b1, M, C, ldw);
    for (int e = tid; e < M * HID; e += BNT) dtb[e] = 0.f;
    for (int e = tid; e < 2 * NWACC; e += BNT) wacc[e] = 0.f;
    float* dpf_b = dpf + (long long)b * N * HID;        // in: W1p feat_n (point_sw_table_kernel); out: dpf
    const bool active = tid < PT * M;
    const int pl = active ? tid / M : 0, m = active ? tid % M : 0;
    const int kb = (tid / 8) * 4, jb = (tid % 8) * 8;      // this thread's 4 x 8 block of dW2
    float* wa = wacc + wave * NWACC;
    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int t0 = n0; t0 < n1; t0 += PT) {
        __syncthreads();                       // the previous tile's readers are done (first tile: tb, dtb, wacc are staged)
        for (int e = tid; e < PT * HID; e += BNT) {         // rows past the range repeat its last point: finite, never used
            const int p = e / HID, j = e % HID;
            pf[p * TS + j] = dpf_b[(long long)min(t0 + p, n1 - 1) * HID + j];
        }
        __syncthreads();
        const int n = t0 + pl;
        const bool valid = active && n < n1;
        float dh[HID];                         // h, later dh and da
        float lp[4] = {b3[0], 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + pf[pl * TS + j];
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
            if (lane == 0) wa[2 * HID] += s3;
        }
#pragma unroll
        for (int j = 0; j < HID; ++j) {
            const float a = tb[m * TS + j] + pf[pl * TS + j];
            dh[j] *= dgelu_tail(a);
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
        // dpf[n, :] = sum_m da[n, m, :], the point's M rows in order (rows of points past the range hold da = 0, not stored)
        for (int e = tid; e < PT * HID; e += BNT) {
            const int p = e / HID, j = e % HID;
            if (t0 + p < n1) {
                float s = 0.f;
                for (int mm = 0; mm < M; ++mm) s += zs[j * RS + p * M + mm];
                dpf_b[(long long)(t0 + p) * HID + j] = s;
            }
        }
    }
    __syncthreads();
    const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    float* ra = rec_a + blk * REC_A;
    float* rb = rec_b + blk * ((long long)M * HID);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) ra[(kb + i) * HID + jb + j] = acc[i][j];
    if (tid < HID) {
        ra[A_DW3 + tid] = wacc[tid] + wacc[NWACC + tid];
        ra[A_DB2 + tid] = wacc[HID + tid] + wacc[NWACC + HID + tid];
    }
    if (tid == 0) {
        ra[A_DB3] = wacc[2 * HID] + wacc[NWACC + 2 * HID];
        ra[A_END] = ra[A_END + 1] = ra[A_END + 2] = 0.f;
    }
    for (int e = tid; e < M * HID; e += BNT) rb[e] = dtb[e];
}

// record r [64][P] = sum over points [r * chunk, min(total, (r+1) * chunk)) of dpf[n, :]^T feat[n, :]; thread (j, g) owns
// columns g, g + 4, ... of row j.  fp32 chains of WBLK points, added to the running sum block by block.
__global__ __launch_bounds__(WNT) void point_sw_dw1p_kernel(const float* __restrict__ dpf, const float* __restrict__ feat,
                                                            float* __restrict__ rec_w, long long total, int P, int chunk) {
    const int j = threadIdx.x % HID, g = threadIdx.x / HID;
    const long long p0 = (long long)blockIdx.x * chunk;
    const long long p1 = p0 + chunk < total ? p0 + chunk : total;
    float acc[WCOLS];
#pragma unroll
    for (int i = 0; i < WCOLS; ++i) acc[i] = 0.f;
    for (long long q0 = p0; q0 < p1; q0 += WBLK) {
        const long long q1 = q0 + WBLK < p1 ? q0 + WBLK : p1;
        float part[WCOLS];
#pragma unroll
        for (int i = 0; i < WCOLS; ++i) part[i] = 0.f;
        for (long long n = q0; n < q1; ++n) {
            const float d = dpf[n * HID + j];
            const float* fr = feat + n * P;
#pragma unroll
            for (int i = 0; i < WCOLS; ++i) {
                const int c = g + 4 * i;
                if (c < P) part[i] = fmaf(d, fr[c], part[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < WCOLS; ++i) acc[i] += part[i];
    }
    float* r = rec_w + (long long)blockIdx.x * HID * P + j * P;
#pragma unroll
    for (int i = 0; i < WCOLS; ++i) {
        const int c = g + 4 * i;
        if (c < P) r[c] = acc[i];
    }
}

// dtbf[b][e] = sum over the nx records of sample b, in a fixed order
__global__ __launch_bounds__(256) void point_sw_dtb_reduce_kernel(const float* __restrict__ rec_b, float* __restrict__ dtbf,
                                                                  long long total, int MH, int nx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / MH, e = i % MH;
    dtbf[i] = (float)strided_sum(rec_b + b * nx * MH + e, nx, MH);
}

// element ranges: [0, B*M*C) dcode = dtb W1c (plain store; skipped when dcode is NULL); then 64 * (C+P+1) parameter elements
// (j, c): c < C dW1c = sum_(b,m) dtb[b,m,j] code[b,m,c]; C <= c < C+P dW1p from the records; c = C+P: db1 = sum_(b,m) dtb
__global__ __launch_bounds__(256) void point_sw_finish_kernel(const float* __restrict__ code, const float* __restrict__ w1,
                                                              const float* __restrict__ dtbf, const float* __restrict__ rec_w,
                                                              float* __restrict__ dcode, float* __restrict__ dw1,
                                                              float* __restrict__ db1, int B, int M, int C, int P, int nrec_w,
                                                              int accumulate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ncode = (long long)B * M * C;
    const int ldw = C + P;
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
    if (e >= (long long)HID * (ldw + 1)) return;
    const int j = (int)(e / (ldw + 1)), c = (int)(e % (ldw + 1));
    double s = 0.0;
    float* dst;
    if (c < C) {
        for (int bm = 0; bm < B * M; ++bm) s = fma((double)dtbf[(long long)bm * HID + j], (double)code[(long long)bm * C + c], s);
        dst = dw1 + j * ldw + c;
    } else if (c < ldw) {
        s = strided_sum(rec_w + j * P + (c - C), nrec_w, (long long)HID * P);
        dst = dw1 + j * ldw + c;
    } else {
        s = strided_sum(dtbf + j, B * M, HID);
        dst = db1 + j;
    }
    *dst = accumulate ? *dst + (float)s : (float)s;
}

// ------------------------------------------------------------------------------------------------ loss stage
// partial[blk] = sum over the workgroup's fixed range of (sw - target)^2.  The differences and their squares are taken in
// fp64 (exact for fp32 operands up to the final rounding of each square), so the loss carries one fp32 rounding in all: a
// streaming kernel has the issue slots for it.  Strided sum per thread, wave butterfly, the four wave sums in order.
__global__ __launch_bounds__(MSE_NT) void slice_mse_partial_kernel(const float* __restrict__ sw, const float* __restrict__ tg,
                                                                   long long n, long long per, double* __restrict__ partial) {
    __shared__ double red[MSE_NT / 64];
    const long long i0 = (long long)blockIdx.x * per;
    const long long i1 = i0 + per < n ? i0 + per : n;
    double s = 0.0;
    for (long long i = i0 + threadIdx.x; i < i1; i += MSE_NT) {
        const double d = (double)sw[i] - (double)tg[i];
        s = fma(d, d, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void slice_mse_final_kernel(const double* __restrict__ partial, int nb, int M,
                                                             float* __restrict__ loss) {
    if (threadIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += partial[i];
    loss[0] = (float)(s / (double)M);
}

__global__ __launch_bounds__(256) void slice_mse_bwd_kernel(const float* __restrict__ sw, const float* __restrict__ tg,
                                                            const float* __restrict__ gout, float* __restrict__ dsw,
                                                            long long n, float two_over_m) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dsw[i] = gout[0] * two_over_m * (sw[i] - tg[i]);
}

// ------------------------------------------------------------------------------------------------ host side
int check_shape(int B, int N, int M, int C, int P, int hidden, int depth) {
    if (C != 8 && C != 16 && C != 32 && C != 64) return PA2D_ERR_UNSUPPORTED;
    if (M < 1 || M > 128 || P < 1 || P > PMAX) return PA2D_ERR_UNSUPPORTED;
    if (hidden != HID || depth != 1) return PA2D_ERR_UNSUPPORTED;
    if (B < 0 || N < 1) return PA2D_ERR_ARG;
    const int widest = M > P ? (M > HID ? M : HID) : (P > HID ? P : HID);      // rows of sw, feat and dpf
    if ((unsigned long long)B * N * widest * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}

constexpr int FWD_TARGET = 2048, BWD_TARGET = 512;

// points per workgroup: a multiple of the points per tile, about `target` workgroups in all
int points_per_block(int B, int N, int pt, int target) {
    int nx = ceil_div(target, B);
    const int maxc = ceil_div(N, pt);
    if (nx > maxc) nx = maxc;
    if (nx < 1) nx = 1;
    return ceil_div(ceil_div(N, nx), pt) * pt;
}

size_t fwd_lds(int M, int P) { return sizeof(float) * ((size_t)M * TS + FNT + (size_t)(FNT / M) * TS + (size_t)P * HID); }
size_t bwd_lds(int M) {
    return sizeof(float) * (2 * (size_t)HID * RS + (size_t)M * TS + (size_t)M * HID + 2 * BNT + 2 * NWACC + (size_t)(BNT / M) * TS);
}

// points per record of the dW1p kernel: a multiple of WBLK, about W_TARGET records
int dw1p_chunk(long long total) { return (int)(ceil_div_ll(ceil_div_ll(total, W_TARGET), WBLK) * WBLK); }

int mse_blocks(long long n) {
    const long long nb = ceil_div_ll(n, 4 * MSE_NT);
    return (int)(nb < MSE_MAXB ? nb : MSE_MAXB);
}

}  // namespace

extern "C" {

int pa2d_point_slice_weights_fwd(const float* code, const float* feat, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* w3, const float* b3, float* sw, int B, int N, int M, int C,
                                 int P, int hidden, int depth, void* stream, void* ev_start, void* ev_stop) {
    const int rc = check_shape(B, N, M, C, P, hidden, depth);
    if (rc) return rc;
    if (B == 0) return PA2D_OK;
    if (!code || !feat || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !sw) return PA2D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ppb = points_per_block(B, N, FNT / M, FWD_TARGET);
    const dim3 grid(ceil_div(N, ppb), B);
    const size_t lds = fwd_lds(M, P);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&point_sw_fwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
    hipLaunchKernelGGL(point_sw_fwd_kernel, grid, dim3(FNT), lds, st, code, feat, w1, b1, w2, b2, w3, b3, sw, N, M, C, P, ppb);
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

size_t pa2d_point_slice_weights_bwd_workspace(int B, int N, int M, int C, int P) {
    if (check_shape(B, N, M, C, P, HID, 1) || B == 0) return 0;
    const int ppb = points_per_block(B, N, BNT / M, BWD_TARGET);
    const size_t nrec = (size_t)ceil_div(N, ppb) * B;
    const long long total = (long long)B * N;
    const size_t nrec_w = (size_t)ceil_div_ll(total, dw1p_chunk(total));
    return sizeof(float) * (nrec * (REC_A + (size_t)M * HID) + (size_t)B * M * HID + (size_t)total * HID + nrec_w * HID * P);
}

int pa2d_point_slice_weights_bwd(const float* code, const float* feat, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* w3, const float* b3, const float* dsw, float* dcode,
                                 float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ws_buf,
                                 size_t ws_bytes, int B, int N, int M, int C, int P, int hidden, int depth, int accumulate,
                                 void* stream, void* ev_start, void* ev_stop) {
    int rc = check_shape(B, N, M, C, P, hidden, depth);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (accumulate) return PA2D_OK;
        if ((rc = pa2d_zero(dw1, sizeof(float) * HID * (C + P), st))) return rc;
        if ((rc = pa2d_zero(db1, sizeof(float) * HID, st))) return rc;
        if ((rc = pa2d_zero(dw2, sizeof(float) * HID * HID, st))) return rc;
        if ((rc = pa2d_zero(db2, sizeof(float) * HID, st))) return rc;
        if ((rc = pa2d_zero(dw3, sizeof(float) * HID, st))) return rc;
        return pa2d_zero(db3, sizeof(float), st);
    }
    if (!code || !feat || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !dsw) return PA2D_ERR_ARG;
    if (!dw1 || !db1 || !dw2 || !db2 || !dw3 || !db3) return PA2D_ERR_ARG;
    if (ws_bytes < pa2d_point_slice_weights_bwd_workspace(B, N, M, C, P) || !ws_buf) return PA2D_ERR_WORKSPACE;
    const int ppb = points_per_block(B, N, BNT / M, BWD_TARGET);
    const int nx = ceil_div(N, ppb), nrec = nx * B;
    const int MH = M * HID;
    const long long total_pts = (long long)B * N;
    const int chunk = dw1p_chunk(total_pts);
    const int nrec_w = (int)ceil_div_ll(total_pts, chunk);
    float* rec_a = (float*)ws_buf;
    float* rec_b = rec_a + (size_t)nrec * REC_A;
    float* dtbf = rec_b + (size_t)nrec * MH;
    float* dpf = dtbf + (size_t)B * MH;
    float* rec_w = dpf + (size_t)total_pts * HID;
    const size_t lds = bwd_lds(M);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&point_sw_bwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
    hipLaunchKernelGGL(point_sw_table_kernel, dim3((unsigned)ceil_div_ll(total_pts, TBL_CHUNK)), dim3(FNT),
                       sizeof(float) * P * HID, st, feat, w1, dpf, total_pts, C, P, TBL_CHUNK);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(point_sw_bwd_kernel, dim3(nx, B), dim3(BNT), lds, st, code, w1, b1, w2, b2, w3, b3, dsw, rec_a, rec_b, dpf,
                       N, M, C, P, ppb);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(point_sw_dw1p_kernel, dim3(nrec_w), dim3(WNT), 0, st, dpf, feat, rec_w, total_pts, P, chunk);
    PA2D_CHECK_LAUNCH();
    // the three kernels whose work grows with N and P lie between the events; the small fixed-order reductions follow
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    const long long total = (long long)B * MH;
    hipLaunchKernelGGL(point_sw_dtb_reduce_kernel, dim3((unsigned)ceil_div_ll(total, 256)), dim3(256), 0, st, rec_b, dtbf,
                       total, MH, nx);
    PA2D_CHECK_LAUNCH();
    const long long nfin = (long long)B * M * C + (long long)HID * (C + P + 1);
    hipLaunchKernelGGL(point_sw_finish_kernel, dim3((unsigned)ceil_div_ll(nfin, 256)), dim3(256), 0, st, code, w1, dtbf, rec_w,
                       dcode, dw1, db1, B, M, C, P, nrec_w, accumulate);
    PA2D_CHECK_LAUNCH();
    ReduceSegs segs;
    segs.nseg = 4;
    segs.begin[0] = 0; segs.begin[1] = A_DB2; segs.begin[2] = A_DW3; segs.begin[3] = A_DB3; segs.begin[4] = A_END;
    segs.dst[0] = dw2; segs.dst[1] = db2; segs.dst[2] = dw3; segs.dst[3] = db3;
    return pa2d_launch_reduce_segs(rec_a, nrec, REC_A, segs, accumulate, st);
}

// The two point coordinates of SequenSolver.py:159-170 are P = 2 point features: pos [B, N, 2], w1 [hidden, C+2].
int pa2d_code_slice_weights_fwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, float* sw, int B, int N, int M, int C,
                                int hidden, int depth, void* stream, void* ev_start, void* ev_stop) {
    return pa2d_point_slice_weights_fwd(code, pos, w1, b1, w2, b2, w3, b3, sw, B, N, M, C, 2, hidden, depth, stream, ev_start,
                                        ev_stop);
}

size_t pa2d_code_slice_weights_bwd_workspace(int B, int N, int M, int C) {
    return pa2d_point_slice_weights_bwd_workspace(B, N, M, C, 2);
}

int pa2d_code_slice_weights_bwd(const float* code, const float* pos, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, const float* dsw, float* dcode,
                                float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ws_buf,
                                size_t ws_bytes, int B, int N, int M, int C, int hidden, int depth, int accumulate,
                                void* stream, void* ev_start, void* ev_stop) {
    return pa2d_point_slice_weights_bwd(code, pos, w1, b1, w2, b2, w3, b3, dsw, dcode, dw1, db1, dw2, db2, dw3, db3, ws_buf,
                                        ws_bytes, B, N, M, C, 2, hidden, depth, accumulate, stream, ev_start, ev_stop);
}

size_t pa2d_slice_mse_workspace(long long rows, int M) {
    if (rows <= 0 || M < 1) return 0;
    return sizeof(double) * (size_t)mse_blocks(rows * M);
}

int pa2d_slice_mse_fwd(const float* sw, const float* target, float* loss, void* ws, size_t ws_bytes, long long rows, int M,
                       void* stream) {
    if (rows < 0 || M < 1) return PA2D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) return pa2d_zero(loss, sizeof(float), st);
    if (!sw || !target || !loss) return PA2D_ERR_ARG;
    if (ws_bytes < pa2d_slice_mse_workspace(rows, M) || !ws || (((uintptr_t)ws) & 7)) return PA2D_ERR_WORKSPACE;
    const long long n = rows * M;
    const int nb = mse_blocks(n);
    const long long per = ceil_div_ll(n, nb);
    hipLaunchKernelGGL(slice_mse_partial_kernel, dim3(nb), dim3(MSE_NT), 0, st, sw, target, n, per, (double*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_mse_final_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nb, M, loss);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

int pa2d_slice_mse_bwd(const float* sw, const float* target, const float* gout, float* dsw, long long rows, int M,
                       void* stream) {
    if (rows < 0 || M < 1) return PA2D_ERR_ARG;
    if (rows == 0) return PA2D_OK;
    if (!sw || !target || !gout || !dsw) return PA2D_ERR_ARG;
    const long long n = rows * M;
    hipLaunchKernelGGL(slice_mse_bwd_kernel, dim3((unsigned)ceil_div_ll(n, 256)), dim3(256), 0, (hipStream_t)stream, sw, target,
                       gout, dsw, n, 2.0f / (float)M);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
