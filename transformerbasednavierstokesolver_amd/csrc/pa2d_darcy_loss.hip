// The loss of one exp_darcy iteration (exp_darcy.py:213-226) on the normalised head output, in two stencil kernels:
//   o = out_n * std + mean, y = y_n * std + mean            (UnitTransformer.decode, utils/normalizer.py)
//   l2_b  = ||o - y|| / ||y||
//   o~    = o with its one-pixel border set to 0            (exp_darcy.py:219-222)
//   gx(f)[i,j] = (f[i,j+1] - f[i,j-1]) / (2 dx), gy(f)[i,j] = (f[i+1,j] - f[i-1,j]) / (2 dx), zeros outside the image
//   dxr_b = ||gx(o~) - gx(y)|| / ||gx(y)||, dyr_b likewise   (central_diff, exp_darcy.py:59-68)
//   loss  = sum_b l2_b + 0.1 sum_b (dxr_b + dyr_b)
//   * pa2d_darcy_loss_fwd : workgroups over (row tiles, B).  A tile stages its rows plus a one-row halo of o and y in
//                           LDS (each element read once), accumulates the six sums of squares and writes them as one
//                           partial record; a one-wave pass adds the records of a sample in tile order (double), takes
//                           the six norms and adds the per-sample ratios in a fixed order -> the same bits every call.
//   * pa2d_darcy_loss_bwd : d loss / d out_n in one kernel: the l2 term plus the two transposed-stencil terms of
//                           d = o~ - y (two-row halo of d in LDS), zero on the border ring that o~ masks, times std.
// mean / std are device scalars (the normaliser's tensors): nothing here reads them on the host.
#include "pa2d_internal.h"

#define DL_THREADS 256
#define DL_ROWS 8                    // rows of a tile (fewer when the LDS budget asks for it)
#define DL_LDS_BYTES (48 * 1024)

static __device__ __forceinline__ float dl_block_sum(float v, float* red /* [4] */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial: [B][ntiles][6] = sums of squares of (o - y, y, gx(o~) - gx(y), gx(y), gy(o~) - gy(y), gy(y)) over the tile
__global__ __launch_bounds__(DL_THREADS) void darcy_loss_fwd_kernel(const float* __restrict__ out_n,
                                                                    const float* __restrict__ y_n,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ stdv, int s, int R,
                                                                    float inv2dx, float* __restrict__ partial) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    const int r0 = blockIdx.x * R;
    const int rows = min(R, s - r0);
    float* lo = lds;                         // o (unmasked; the border mask is applied where o~ is read)
    float* ly = lds + (size_t)(R + 2) * s;
    const float mu = *mean, sd = *stdv;
    const size_t base = (size_t)blockIdx.y * s * s;
    const int nstage = (rows + 2) * s;       // image rows r0 - 1 .. r0 + rows; rows outside the image hold 0
    for (int idx = threadIdx.x; idx < nstage; idx += DL_THREADS) {
        const int lr = idx / s, j = idx - lr * s, i = r0 - 1 + lr;
        float o = 0.f, y = 0.f;
        if (i >= 0 && i < s) {
            const size_t g = base + (size_t)i * s + j;
            o = fmaf(out_n[g], sd, mu);
            y = fmaf(y_n[g], sd, mu);
        }
        lo[idx] = o;
        ly[idx] = y;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f;
    const int n = rows * s;
    for (int idx = threadIdx.x; idx < n; idx += DL_THREADS) {
        const int lr = idx / s, j = idx - lr * s, i = r0 + lr;
        const int c = (lr + 1) * s + j;
        const float y = ly[c], e = lo[c] - y;
        a0 += e * e;
        a1 += y * y;
        const bool rowin = i >= 1 && i <= s - 2, colin = j >= 1 && j <= s - 2;
        // d/dx: neighbours (i, j -+ 1); o~ is o on interior pixels, 0 on the border ring and outside
        const float ol = (rowin && j >= 2) ? lo[c - 1] : 0.f;
        const float orr = (rowin && j <= s - 3) ? lo[c + 1] : 0.f;
        const float yl = j > 0 ? ly[c - 1] : 0.f;
        const float yr = j < s - 1 ? ly[c + 1] : 0.f;
        const float gx = (yr - yl) * inv2dx, ex = (orr - ol) * inv2dx - gx;
        a2 += ex * ex;
        a3 += gx * gx;
        // d/dy: neighbours (i -+ 1, j); the halo rows outside the image are zero
        const float ou = (colin && i >= 2) ? lo[c - s] : 0.f;
        const float od = (colin && i <= s - 3) ? lo[c + s] : 0.f;
        const float gy = (ly[c + s] - ly[c - s]) * inv2dx, ey = (od - ou) * inv2dx - gy;
        a4 += ey * ey;
        a5 += gy * gy;
    }
    a0 = dl_block_sum(a0, red);
    a1 = dl_block_sum(a1, red);
    a2 = dl_block_sum(a2, red);
    a3 = dl_block_sum(a3, red);
    a4 = dl_block_sum(a4, red);
    a5 = dl_block_sum(a5, red);
    if (threadIdx.x == 0) {
        float* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
        p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3; p[4] = a4; p[5] = a5;
    }
}

// one wave: norms[k][b] = sqrt(sum over the tiles, in tile order), sums = (loss, sum l2, sum (dxr + dyr))
__global__ __launch_bounds__(64) void darcy_loss_finish_kernel(const float* __restrict__ partial, int B, int ntiles,
                                                               float* __restrict__ norms, float* __restrict__ sums) {
    float l2 = 0.f, dv = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) {
        const float* p = partial + (size_t)b * ntiles * 6;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0., s5 = 0.;
        for (int t = 0; t < ntiles; ++t) {
            s0 += p[t * 6 + 0]; s1 += p[t * 6 + 1]; s2 += p[t * 6 + 2];
            s3 += p[t * 6 + 3]; s4 += p[t * 6 + 4]; s5 += p[t * 6 + 5];
        }
        const float n0 = sqrtf((float)s0), n1 = sqrtf((float)s1), n2 = sqrtf((float)s2), n3 = sqrtf((float)s3),
                    n4 = sqrtf((float)s4), n5 = sqrtf((float)s5);
        norms[0 * (size_t)B + b] = n0; norms[1 * (size_t)B + b] = n1; norms[2 * (size_t)B + b] = n2;
        norms[3 * (size_t)B + b] = n3; norms[4 * (size_t)B + b] = n4; norms[5 * (size_t)B + b] = n5;
        l2 += n0 / n1;
        dv += n2 / n3 + n4 / n5;
    }
    l2 = wave_sum(l2);
    dv = wave_sum(dv);
    if (threadIdx.x == 0) {
        sums[0] = fmaf(0.1f, dv, l2);
        sums[1] = l2;
        sums[2] = dv;
    }
}

// dout[b][i][j] = std * ( coef[0] (o - y) / (n0 n1)
//                       + interior(i,j) coef[1] / (2 dx) * ( (rx[i,j-1] - rx[i,j+1]) / (n2 n3) + (ry[i-1,j] - ry[i+1,j]) / (n4 n5) ) )
// with rx = gx(o~) - gx(y) = (d[i,j+1] - d[i,j-1]) / (2 dx), d = o~ - y (zero outside the image), ry likewise;
// coef = (d L / d sum l2, d L / d sum (dxr + dyr)) of the caller's upstream gradients (device, 2 floats).
// A zero difference norm (n0, n2 or n4) gives that term the zero sub-gradient, as pa2d_rel_l2_bwd does.
__global__ __launch_bounds__(DL_THREADS) void darcy_loss_bwd_kernel(const float* __restrict__ out_n,
                                                                    const float* __restrict__ y_n,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ stdv,
                                                                    const float* __restrict__ norms,
                                                                    const float* __restrict__ coef, int B, int s, int R,
                                                                    float inv2dx, float* __restrict__ dout) {
    extern __shared__ float ld[];            // d on image rows r0 - 2 .. r0 + rows + 1
    const int r0 = blockIdx.x * R;
    const int rows = min(R, s - r0);
    const int b = blockIdx.y;
    const float mu = *mean, sd = *stdv;
    const size_t base = (size_t)b * s * s;
    const int nstage = (rows + 4) * s;
    for (int idx = threadIdx.x; idx < nstage; idx += DL_THREADS) {
        const int lr = idx / s, j = idx - lr * s, i = r0 - 2 + lr;
        float d = 0.f;
        if (i >= 0 && i < s) {
            const size_t g = base + (size_t)i * s + j;
            const bool interior = i >= 1 && i <= s - 2 && j >= 1 && j <= s - 2;
            const float o = interior ? fmaf(out_n[g], sd, mu) : 0.f;
            d = o - fmaf(y_n[g], sd, mu);
        }
        ld[idx] = d;
    }
    __syncthreads();
    const float n0 = norms[0 * (size_t)B + b], n1 = norms[1 * (size_t)B + b], n2 = norms[2 * (size_t)B + b],
                n3 = norms[3 * (size_t)B + b], n4 = norms[4 * (size_t)B + b], n5 = norms[5 * (size_t)B + b];
    const float c0 = n0 > 0.f ? coef[0] * sd / (n0 * n1) : 0.f;
    const float cx = n2 > 0.f ? coef[1] * sd * inv2dx / (n2 * n3) : 0.f;
    const float cy = n4 > 0.f ? coef[1] * sd * inv2dx / (n4 * n5) : 0.f;
    const int n = rows * s;
    for (int idx = threadIdx.x; idx < n; idx += DL_THREADS) {
        const int lr = idx / s, j = idx - lr * s, i = r0 + lr;
        const int c = (lr + 2) * s + j;
        const size_t g = base + (size_t)i * s + j;
        const float dc = ld[c];
        float grad;
        if (i >= 1 && i <= s - 2 && j >= 1 && j <= s - 2) {
            const float dl = j >= 2 ? ld[c - 2] : 0.f, dr = j <= s - 3 ? ld[c + 2] : 0.f;
            const float du = ld[c - 2 * s], dd = ld[c + 2 * s];       // rows outside the image hold 0
            const float tx = ((dc - dl) - (dr - dc)) * inv2dx;        // rx[i,j-1] - rx[i,j+1]
            const float ty = ((dc - du) - (dd - dc)) * inv2dx;        // ry[i-1,j] - ry[i+1,j]
            grad = c0 * dc + cx * tx + cy * ty;
        } else {
            grad = c0 * (fmaf(out_n[g], sd, mu) + dc);                // d = -y on the border ring
        }
        dout[g] = grad;
    }
}

static int dl_tile_rows(int s, int arrays, int halo) {
    const long long fit = (long long)DL_LDS_BYTES / ((long long)s * 4 * arrays) - 2 * halo;
    return (int)(fit < DL_ROWS ? fit : DL_ROWS);       // < 1: the rows of this image do not fit
}

extern "C" {

size_t pa2d_darcy_loss_workspace(int B, int s) {
    if (B <= 0 || s <= 0) return 0;
    const int R = dl_tile_rows(s, 2, 1);
    if (R < 1) return 0;
    return sizeof(float) * 6 * (size_t)B * (size_t)ceil_div(s, R);
}

// norms: [6][B], sums: [3]; ws: pa2d_darcy_loss_workspace(B, s) bytes
int pa2d_darcy_loss_fwd(const float* out_n, const float* y_n, const float* mean, const float* stdv, float* norms,
                        float* sums, void* ws, size_t ws_bytes, int B, int s, float dx, hipStream_t st) {
    if (s < 1 || !(dx > 0.f)) return PA2D_ERR_ARG;
    if (B <= 0) return pa2d_zero(sums, 3 * sizeof(float), st);
    const int R = dl_tile_rows(s, 2, 1);
    if (R < 1 || B > 65535) return PA2D_ERR_UNSUPPORTED;
    if (ws_bytes < pa2d_darcy_loss_workspace(B, s)) return PA2D_ERR_WORKSPACE;
    const int ntiles = ceil_div(s, R);
    const float inv2dx = (float)(1.0 / (2.0 * (double)dx));
    const size_t lds = sizeof(float) * 2 * (size_t)(R + 2) * s;
    hipLaunchKernelGGL(darcy_loss_fwd_kernel, dim3(ntiles, B), dim3(DL_THREADS), lds, st, out_n, y_n, mean, stdv, s, R,
                       inv2dx, (float*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(darcy_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)ws, B, ntiles, norms, sums);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// coef: 2 floats on the device (see the kernel); dout: [B, s*s]
int pa2d_darcy_loss_bwd(const float* out_n, const float* y_n, const float* mean, const float* stdv, const float* norms,
                        const float* coef, float* dout, int B, int s, float dx, hipStream_t st) {
    if (s < 1 || !(dx > 0.f)) return PA2D_ERR_ARG;
    if (B <= 0) return PA2D_OK;
    const int R = dl_tile_rows(s, 1, 2);
    if (R < 1 || B > 65535) return PA2D_ERR_UNSUPPORTED;
    const float inv2dx = (float)(1.0 / (2.0 * (double)dx));
    const size_t lds = sizeof(float) * (size_t)(R + 4) * s;
    hipLaunchKernelGGL(darcy_loss_bwd_kernel, dim3(ceil_div(s, R), B), dim3(DL_THREADS), lds, st, out_n, y_n, mean, stdv,
                       norms, coef, B, s, R, inv2dx, dout);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
