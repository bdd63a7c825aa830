// The step tail of the velocity-field trainers (ns_velocity.py, ns_velocity_unrolling.py, ns_unrolling2_with_t.py), where one
// prediction is k = `step` columns (vel_x, vel_y) of a [B, N, T] trajectory:
//   * pa2d_rel_l2_window_fwd / _bwd : per-sample ||pred - y|| / ||y|| of pred [B, N, k] against the column window
//                                     yy[..., c:c+k] of a wider tensor, read where it lies (a two-dimensional strided view:
//                                     row stride and batch stride), and its gradient w.r.t. pred.  The reduction is that of
//                                     pa2d_rel_l2_affine_fwd: a sample is spread over up to PA2D_WINDOW_SPLIT workgroups, each
//                                     writes one (sum d^2, sum y^2) record, a one-wave pass adds a sample's records in split
//                                     order (double): the same bits every call, no float atomics.
//   * pa2d_rollout_tail             : ONE launch after each model call of a no-grad prediction-feedback rollout: the input
//                                     window [B, N, F] is shifted by k columns in place and pred appended; pred goes into
//                                     columns [c, c+k) of the trajectory buffer (optional); the step's partial sums of
//                                     (pred - y)^2 and y^2 go into slot s of a record [S, B, PA2D_WINDOW_SPLIT, 2] (optional).
//   * pa2d_rollout_score            : one launch after the last step: the record -> step_ratio [S, B], full_ratio [B].
// A window row is F dwords (40 bytes at F = 10): nothing here assumes more than 4-byte alignment.  A tile of WIN_ROWS
// consecutive rows of a sample is one contiguous run of dwords: it is read into LDS with lane i on dword i (coalesced), the
// workgroup synchronises, and the shifted rows are written back the same way, each dword taken from LDS (column + k) or from
// the staged pred rows.  Every row of a tile is read before any is written and tiles own disjoint rows, so the in-place
// shift has no hazard.
#include "pa2d_internal.h"

#define WIN_THREADS 256
#define WIN_SPLIT 64                 // == PA2D_WINDOW_SPLIT (include/pa2d.h)
#define WIN_CHUNK 1024               // elements of a sample that one workgroup of the loss kernels covers per pass
#define WIN_ROWS 64                  // rows of one LDS tile of the rollout tail
#define WIN_MAX_K 8                  // == PA2D_WINDOW_MAX_K
#define WIN_MAX_F 64                 // == PA2D_WINDOW_MAX_F

static __device__ __forceinline__ float win_block_sum(float v, float* red /* [4] */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial: [B][nsplit][2] = (sum (pred - y)^2, sum y^2) of the elements this workgroup covers; element i of a sample is
// (row i / k, column i % k)
__global__ __launch_bounds__(WIN_THREADS) void rel_l2_window_fwd_kernel(const float* __restrict__ pred,
                                                                        const float* __restrict__ y, long long yrs,
                                                                        long long ybs, long long L, int k,
                                                                        float* __restrict__ partial) {
    __shared__ float red[4];
    const int sp = blockIdx.x, nsplit = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const float* pb = pred + (size_t)b * L;
    const float* yb = y + (long long)b * ybs;
    float sdq = 0.f, syq = 0.f;
    for (long long i = (long long)sp * WIN_THREADS + tid; i < L; i += (long long)nsplit * WIN_THREADS) {
        const long long row = i / k;
        const int j = (int)(i - row * k);
        const float t = yb[row * yrs + j];
        const float d = pb[i] - t;
        sdq += d * d;
        syq += t * t;
    }
    const float td = win_block_sum(sdq, red);
    const float ty = win_block_sum(syq, red);
    if (tid == 0) {
        float* p = partial + ((size_t)b * nsplit + sp) * 2;
        p[0] = td;
        p[1] = ty;
    }
}

// one wave: a lane adds the records of its samples in split order
__global__ __launch_bounds__(64) void rel_l2_window_finish_kernel(const float* __restrict__ partial, int B, int nsplit,
                                                                  float* __restrict__ dnorm, float* __restrict__ ynorm,
                                                                  float* __restrict__ ratio) {
    for (int b = threadIdx.x; b < B; b += 64) {
        const float* p = partial + (size_t)b * nsplit * 2;
        double s0 = 0., s1 = 0.;
        for (int i = 0; i < nsplit; ++i) {
            s0 += p[2 * i];
            s1 += p[2 * i + 1];
        }
        const float d = sqrtf((float)s0), n = sqrtf((float)s1);
        dnorm[b] = d;
        ynorm[b] = n;
        ratio[b] = d / n;
    }
}

__global__ __launch_bounds__(WIN_THREADS) void rel_l2_window_bwd_kernel(const float* __restrict__ pred,
                                                                        const float* __restrict__ y, long long yrs,
                                                                        long long ybs, const float* __restrict__ dnorm,
                                                                        const float* __restrict__ ynorm,
                                                                        const float* __restrict__ gout, long long L, int k,
                                                                        float* __restrict__ dpred) {
    const int sp = blockIdx.x, nsplit = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const float dn = dnorm[b];
    const float s = dn > 0.f ? gout[b] / (dn * ynorm[b]) : 0.f;
    const float* pb = pred + (size_t)b * L;
    const float* yb = y + (long long)b * ybs;
    float* gb = dpred + (size_t)b * L;
    for (long long i = (long long)sp * WIN_THREADS + tid; i < L; i += (long long)nsplit * WIN_THREADS) {
        const long long row = i / k;
        const int j = (int)(i - row * k);
        gb[i] = s * (pb[i] - yb[row * yrs + j]);
    }
}

// grid (nsplit, B); workgroup sp of a sample takes the row tiles sp, sp + nsplit, ...
__global__ __launch_bounds__(WIN_THREADS) void rollout_tail_kernel(const float* __restrict__ pred, float* window,
                                                                   float* __restrict__ traj, long long T, long long c,
                                                                   const float* __restrict__ y, long long yrs, long long ybs,
                                                                   float* __restrict__ rec, int N, int k, int F) {
    __shared__ float tile[WIN_ROWS * WIN_MAX_F];
    __shared__ float ptile[WIN_ROWS * WIN_MAX_K];
    __shared__ float red[4];
    const int sp = blockIdx.x, nsplit = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const int ntiles = (N + WIN_ROWS - 1) / WIN_ROWS;
    const int keep = F - k;                          // columns of the old window that stay (shifted to the front)
    float sdq = 0.f, syq = 0.f;
    for (int t = sp; t < ntiles; t += nsplit) {
        const int r0 = t * WIN_ROWS;
        const int nr = N - r0 < WIN_ROWS ? N - r0 : WIN_ROWS;
        const size_t row0 = (size_t)b * N + r0;      // first row of the tile among all B N rows
        float* wt = window + row0 * F;
        const float* pt = pred + row0 * k;
        const int nw = nr * F, np = nr * k;
        __syncthreads();                             // the previous tile's LDS reads are done
        for (int i = tid; i < nw; i += WIN_THREADS) tile[i] = wt[i];
        for (int i = tid; i < np; i += WIN_THREADS) ptile[i] = pt[i];
        __syncthreads();                             // every row of the tile is in LDS before one is overwritten
        for (int i = tid; i < nw; i += WIN_THREADS) {
            const int row = i / F, col = i - row * F;
            wt[i] = col < keep ? tile[i + k] : ptile[row * k + (col - keep)];
        }
        for (int i = tid; i < np; i += WIN_THREADS) {
            const int row = i / k, j = i - row * k;
            const float p = ptile[i];
            if (traj) traj[(row0 + row) * T + c + j] = p;
            if (y) {
                const float v = y[(long long)b * ybs + (long long)(r0 + row) * yrs + j];
                const float d = p - v;
                sdq += d * d;
                syq += v * v;
            }
        }
    }
    if (y) {                                         // (uniform over the workgroup)
        const float td = win_block_sum(sdq, red);
        const float ty = win_block_sum(syq, red);
        if (tid == 0) {
            float* p = rec + ((size_t)b * WIN_SPLIT + sp) * 2;
            p[0] = td;
            p[1] = ty;
        }
    }
}

// one wave: lane b adds step s's records in split order (double), then the steps in step order
__global__ __launch_bounds__(64) void rollout_score_kernel(const float* __restrict__ rec, int S, int B, int nsplit,
                                                           float* __restrict__ step_ratio, float* __restrict__ full_ratio) {
    for (int b = threadIdx.x; b < B; b += 64) {
        double fd = 0., fy = 0.;
        for (int s = 0; s < S; ++s) {
            const float* p = rec + ((size_t)s * B + b) * WIN_SPLIT * 2;
            double s0 = 0., s1 = 0.;
            for (int i = 0; i < nsplit; ++i) {
                s0 += p[2 * i];
                s1 += p[2 * i + 1];
            }
            step_ratio[(size_t)s * B + b] = sqrtf((float)s0) / sqrtf((float)s1);
            fd += s0;
            fy += s1;
        }
        full_ratio[b] = sqrtf((float)fd) / sqrtf((float)fy);
    }
}

static int win_nsplit(long long L) {
    const long long n = ceil_div_ll(L, WIN_CHUNK);
    return n > WIN_SPLIT ? WIN_SPLIT : (int)n;
}
static int win_tail_nsplit(int N) {
    const int n = ceil_div(N, WIN_ROWS);
    return n > WIN_SPLIT ? WIN_SPLIT : n;
}
static bool win_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 3) != 0;
}

extern "C" {

// dnorm, ynorm, ratio: [B]; ws: at least 2 * B * PA2D_WINDOW_SPLIT floats
int pa2d_rel_l2_window_fwd(const float* pred, const float* y, long long y_row_stride, long long y_batch_stride,
                           float* dnorm, float* ynorm, float* ratio, void* ws, size_t ws_bytes, int B, int N, int k,
                           hipStream_t st) {
    if (B < 0 || N < 0) return PA2D_ERR_ARG;
    if (k < 1 || k > WIN_MAX_K || B > 65535) return PA2D_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return PA2D_OK;
    if (win_misaligned(pred, y, ws) || y_row_stride < 0) return PA2D_ERR_ARG;
    if (ws_bytes < sizeof(float) * 2 * (size_t)B * WIN_SPLIT) return PA2D_ERR_WORKSPACE;
    const long long L = (long long)N * k;
    const int nsplit = win_nsplit(L);
    hipLaunchKernelGGL(rel_l2_window_fwd_kernel, dim3(nsplit, B), dim3(WIN_THREADS), 0, st, pred, y, y_row_stride,
                       y_batch_stride, L, k, (float*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(rel_l2_window_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)ws, B, nsplit, dnorm, ynorm,
                       ratio);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// gout: the per-sample upstream gradient [B]; dpred: [B, N, k]
int pa2d_rel_l2_window_bwd(const float* pred, const float* y, long long y_row_stride, long long y_batch_stride,
                           const float* dnorm, const float* ynorm, const float* gout, float* dpred, int B, int N, int k,
                           hipStream_t st) {
    if (B < 0 || N < 0) return PA2D_ERR_ARG;
    if (k < 1 || k > WIN_MAX_K || B > 65535) return PA2D_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return PA2D_OK;
    if (win_misaligned(pred, y, dpred) || y_row_stride < 0) return PA2D_ERR_ARG;
    const long long L = (long long)N * k;
    long long nb = ceil_div_ll(L, WIN_CHUNK);
    if (nb > 256) nb = 256;
    hipLaunchKernelGGL(rel_l2_window_bwd_kernel, dim3((int)nb, B), dim3(WIN_THREADS), 0, st, pred, y, y_row_stride,
                       y_batch_stride, dnorm, ynorm, gout, L, k, dpred);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// window [B, N, F] in place; traj [B, N, T] or NULL (columns [c, c + k) are written); y or NULL: element (b, n, j) of the
// target at y[b * y_batch_stride + n * y_row_stride + j]; record [S, B, PA2D_WINDOW_SPLIT, 2], slot s is written
int pa2d_rollout_tail(const float* pred, float* window, float* traj, long long T, long long c, const float* y,
                      long long y_row_stride, long long y_batch_stride, float* record, int s, int S, int B, int N, int k,
                      int F, hipStream_t st) {
    if (B < 0 || N < 0) return PA2D_ERR_ARG;
    if (k < 1 || k > WIN_MAX_K || F < k || F > WIN_MAX_F || B > 65535) return PA2D_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return PA2D_OK;
    if (win_misaligned(pred, window, traj, y) || win_misaligned(record)) return PA2D_ERR_ARG;
    if (traj && (c < 0 || c + k > T)) return PA2D_ERR_ARG;
    if (y && (record == nullptr || s < 0 || s >= S || y_row_stride < 0)) return PA2D_ERR_ARG;
    float* rec = y ? record + (size_t)s * B * WIN_SPLIT * 2 : nullptr;
    hipLaunchKernelGGL(rollout_tail_kernel, dim3(win_tail_nsplit(N), B), dim3(WIN_THREADS), 0, st, pred, window, traj, T, c,
                       y, y_row_stride, y_batch_stride, rec, N, k, F);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// record as the S calls of pa2d_rollout_tail on [B, N, .] left it; step_ratio [S, B], full_ratio [B]
int pa2d_rollout_score(const float* record, float* step_ratio, float* full_ratio, int S, int B, int N, hipStream_t st) {
    if (S < 0 || B < 0 || N < 0) return PA2D_ERR_ARG;
    if (S == 0 || B == 0 || N == 0) return PA2D_OK;
    if (win_misaligned(record, step_ratio, full_ratio)) return PA2D_ERR_ARG;
    hipLaunchKernelGGL(rollout_score_kernel, dim3(1), dim3(64), 0, st, record, S, B, win_tail_nsplit(N), step_ratio,
                       full_ratio);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
