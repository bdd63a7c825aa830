// Stages of the conv slice predictors (reference SliceLearner.py, class SliceLearner; LearnSlice.forward_from_vorticity;
// SequenSolverMerged.SequenSolver.forward_slice) that the other translation units do not have:
//   - the z-score over a WHOLE tensor (mean and population std over every element, batch included), and
//   - the wide slice weights softmax_m((x . Ws^T + bs) / t) for D up to 512 features per row.
// Both are exact fp32 on every engine (fp32 FMAs on the VALU; every global sum in fp64 in a fixed order), keep no state and
// use no atomics: runs are bitwise repeatable.  The single 3x3 conv of these models lives in pa2d_gemm.hip.
#include "pa2d_internal.h"

extern "C" size_t pa2d_gemm_bwd_weight_workspace(int M, int N, int K, int engine);
extern "C" int pa2d_gemm_bwd_weight(const float* dy, long long lddy, const float* x, long long ldx, float* dw, float* db,
                                    void* ws, size_t ws_bytes, int M, int N, int K, int accumulate, int engine,
                                    hipStream_t stream);

namespace {

constexpr int NT = 256;

// fixed-order sum of one double per thread over the 256 threads of a workgroup; every thread returns the total
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // red may still be read from a previous call
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------
// z-score.  Pass 1: workgroup b sums its fixed range of float4 elements in fp64 (products of two floats are exact there):
// forward (sum x, sum x^2), backward (sum dy, sum dy*y) -> part[b][2].  Pass 2: every workgroup adds the partial records in
// the same fixed order, so all of them hold the same statistics, and maps its own range.
// Grouped form: blockIdx.y is a group of `rows` consecutive rows with its own partial records, statistics and ranges; every
// base below is moved to the group once, so a group runs the arithmetic of an ungrouped launch on its rows alone.
constexpr int Z_V4_PER_BLOCK = NT * 16;      // pass 1: float4 elements per workgroup (until 1024 workgroups)
constexpr int Z_MAP_V4 = NT * 8;             // pass 2: float4 elements per workgroup
static int zscore_blocks(long long n4) {
    long long b = ceil_div_ll(n4, Z_V4_PER_BLOCK);
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

template <bool BWD>
__global__ __launch_bounds__(NT) void zscore_partial_kernel(const float* __restrict__ a, long long lda,
                                                           const float* __restrict__ b, long long n4, int q4,
                                                           long long per, double* __restrict__ part) {
    __shared__ double red[4];
    a += (long long)blockIdx.y * (n4 / q4) * lda;
    if (BWD) b += (long long)blockIdx.y * n4 * 4;
    part += 2 * (size_t)blockIdx.y * gridDim.x;
    const long long begin = (long long)blockIdx.x * per;
    const long long end = begin + per < n4 ? begin + per : n4;
    double s = 0.0, q = 0.0;
    for (long long i = begin + threadIdx.x; i < end; i += NT) {
        const long long row = i / q4;
        const int c4 = (int)(i - row * q4);
        const float4 v = *reinterpret_cast<const float4*>(a + row * lda + c4 * 4);
        float4 w = v;
        if (BWD) w = *reinterpret_cast<const float4*>(b + i * 4);
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        q += ((double)v.x * (double)w.x + (double)v.y * (double)w.y) + ((double)v.z * (double)w.z + (double)v.w * (double)w.w);
    }
    s = block_sum_f64(s, red);
    q = block_sum_f64(q, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s;
        part[2 * blockIdx.x + 1] = q;
    }
}

__device__ __forceinline__ void zscore_totals(const double* __restrict__ part, int nb, double* red, double& S, double& Q) {
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) {
        s += part[2 * i];
        q += part[2 * i + 1];
    }
    S = block_sum_f64(s, red);
    Q = block_sum_f64(q, red);
}

__global__ __launch_bounds__(NT) void zscore_fwd_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ y,
                                                       double* __restrict__ stats, const double* __restrict__ part, int nb,
                                                       long long n4, int q4) {
    __shared__ double red[4];
    x += (long long)blockIdx.y * (n4 / q4) * ldx;
    y += (long long)blockIdx.y * n4 * 4;
    stats += 2 * blockIdx.y;
    part += 2 * (size_t)blockIdx.y * nb;
    double S, Q;
    zscore_totals(part, nb, red, S, Q);
    const double n = (double)n4 * 4.0;
    const double mu = S / n;
    // n*Q - S*S is zero for a constant input in exact arithmetic, but Q (sums of 48-bit squares) is rounded at every add:
    // a remainder within 64 parts in 2^52 of n*Q is rounding, not a variance (data with mean = 10^6 std leaves 10^-12).
    const double sq = S * S, nq = n * Q;
    const double var = (nq - sq > 64.0 * 2.220446049250313e-16 * nq) ? (nq - sq) / (n * n) : 0.0;
    const double sigma = sqrt(var);
    const double inv = 1.0 / (sigma + 1e-8);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = mu;
        stats[1] = sigma;
    }
    const long long begin = (long long)blockIdx.x * Z_MAP_V4;
    const long long end = begin + Z_MAP_V4 < n4 ? begin + Z_MAP_V4 : n4;
    for (long long i = begin + threadIdx.x; i < end; i += NT) {
        const long long row = i / q4;
        const int c4 = (int)(i - row * q4);
        const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + c4 * 4);
        float4 o;
        o.x = (float)(((double)v.x - mu) * inv);
        o.y = (float)(((double)v.y - mu) * inv);
        o.z = (float)(((double)v.z - mu) * inv);
        o.w = (float)(((double)v.w - mu) * inv);
        *reinterpret_cast<float4*>(y + i * 4) = o;
    }
}

// dx = (dy - mean(dy) - y * mean(dy*y) * (sigma + eps) / sigma) / (sigma + eps)
__global__ __launch_bounds__(NT) void zscore_bwd_kernel(const float* __restrict__ dy, long long lddy,
                                                       const float* __restrict__ y, const double* __restrict__ stats,
                                                       float* __restrict__ dx, long long lddx,
                                                       const double* __restrict__ part, int nb, long long n4, int q4) {
    __shared__ double red[4];
    dy += (long long)blockIdx.y * (n4 / q4) * lddy;
    y += (long long)blockIdx.y * n4 * 4;
    dx += (long long)blockIdx.y * (n4 / q4) * lddx;
    stats += 2 * blockIdx.y;
    part += 2 * (size_t)blockIdx.y * nb;
    double S, Q;
    zscore_totals(part, nb, red, S, Q);
    const double n = (double)n4 * 4.0;
    const double sigma = stats[1], se = sigma + 1e-8;
    const double m1 = S / n, c2 = (Q / n) * (se / sigma), inv = 1.0 / se;
    const long long begin = (long long)blockIdx.x * Z_MAP_V4;
    const long long end = begin + Z_MAP_V4 < n4 ? begin + Z_MAP_V4 : n4;
    for (long long i = begin + threadIdx.x; i < end; i += NT) {
        const long long row = i / q4;
        const int c4 = (int)(i - row * q4);
        const float4 g = *reinterpret_cast<const float4*>(dy + row * lddy + c4 * 4);
        const float4 v = *reinterpret_cast<const float4*>(y + i * 4);
        float4 o;
        o.x = (float)(((double)g.x - m1 - (double)v.x * c2) * inv);
        o.y = (float)(((double)g.y - m1 - (double)v.y * c2) * inv);
        o.z = (float)(((double)g.z - m1 - (double)v.z * c2) * inv);
        o.w = (float)(((double)g.w - m1 - (double)v.w * c2) * inv);
        *reinterpret_cast<float4*>(dx + row * lddx + c4 * 4) = o;
    }
}

static int zscore_check(long long rows, int C, long long ld) {
    if (C <= 0 || (C & 3)) return PA2D_ERR_UNSUPPORTED;
    if (rows <= 0) return PA2D_OK;
    if (ld < C || (ld & 3)) return PA2D_ERR_ARG;
    if (((unsigned long long)(rows - 1) * ld + C) * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}

constexpr int Z_MAX_GROUPS = 65535;           // the group is a grid axis
// `groups` groups of `rpg` rows in one tensor of pitch ld: the shape contract of zscore_check, the extent over ALL rows
static int zscore_grouped_check(int groups, long long rpg, int C, long long ld) {
    if (C <= 0 || (C & 3)) return PA2D_ERR_UNSUPPORTED;
    if (groups < 1 || rpg < 0) return PA2D_ERR_ARG;
    if (groups > Z_MAX_GROUPS || rpg > (long long)0x7FFFFFFF) return PA2D_ERR_UNSUPPORTED;
    return zscore_check((long long)groups * rpg, C, ld);
}

// ---------------------------------------------------------------------------------------------
// wide slice weights.  A workgroup owns 32 rows; a row pair belongs to a group of 16 lanes, lane g of it holds the logits
// of the slices m = g, g + 16, ... (MPL of them, so any M <= 16 * MPL is served; absent slices are masked) in registers.
// x tiles [32][32] and Ws chunks [M][32] go through LDS (Ws is up to 256 KB: chunked over D); the softmax runs inside the
// lane group with four butterfly steps.  Row pitch 36 floats: an odd number of 16-byte slots, conflict-free float4 reads
// of 16 consecutive Ws rows.
constexpr int W_ROWS = 32, W_DC = 32, W_P = W_DC + 4;

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wide_temperature(const float* temperature, int clamp) {
    const float tv = temperature[0];
    return clamp ? fminf(fmaxf(tv, 0.1f), 5.0f) : tv;
}

__device__ __forceinline__ void wide_stage_ws(const float* __restrict__ Ws, float (*wsm)[W_P], int M, int D, int d0, int mrows) {
    for (int i = threadIdx.x; i < mrows * (W_DC / 4); i += NT) {
        const int m = i >> 3, c4 = i & 7, col = d0 + c4 * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < M && col < D) v = *reinterpret_cast<const float4*>(Ws + (size_t)m * D + col);
        *reinterpret_cast<float4*>(&wsm[m][c4 * 4]) = v;
    }
}

template <int MPL, bool BWD>
__global__ __launch_bounds__(NT) void wide_sw_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ Ws,
                                                    const float* __restrict__ bs, const float* __restrict__ temperature,
                                                    float* __restrict__ sw, const float* __restrict__ dsw,
                                                    float* __restrict__ dx, long long lddx, float* __restrict__ dlbuf,
                                                    double* __restrict__ dtpart, int rows, int D, int M, int Mp, int clamp) {
    constexpr int MR = MPL * 16;              // slice rows staged per chunk
    constexpr int DLP = MR + 1;               // pitch of the dl tile (odd: the eight rows of a wave on distinct banks)
    __shared__ __attribute__((aligned(16))) float xs[W_ROWS][W_P];
    __shared__ __attribute__((aligned(16))) float wsm[MR][W_P];
    __shared__ float dls[BWD ? W_ROWS * DLP : 1];
    __shared__ double red[4];
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const int row0 = blockIdx.x * W_ROWS;

    float acc[2][MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) acc[0][j] = acc[1][j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += W_DC) {
        __syncthreads();
        {
            const int r = tid >> 3, c4 = tid & 7, row = row0 + r, col = d0 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < rows && col < D) v = *reinterpret_cast<const float4*>(x + (size_t)row * ldx + col);
            *reinterpret_cast<float4*>(&xs[r][c4 * 4]) = v;
        }
        wide_stage_ws(Ws, wsm, M, D, d0, MR);
        __syncthreads();
        // two-level sum: each 32-feature chunk on its own, then added to the total (a third of the rounding error of one
        // D-long chain at D = 384)
        float part[2][MPL];
#pragma unroll
        for (int j = 0; j < MPL; ++j) part[0][j] = part[1][j] = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < W_DC / 4; ++k4) {
            const float4 xa = *reinterpret_cast<const float4*>(&xs[grp * 2][k4 * 4]);
            const float4 xb = *reinterpret_cast<const float4*>(&xs[grp * 2 + 1][k4 * 4]);
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const float4 w = *reinterpret_cast<const float4*>(&wsm[g + 16 * j][k4 * 4]);
                part[0][j] = fmaf(xa.w, w.w, fmaf(xa.z, w.z, fmaf(xa.y, w.y, fmaf(xa.x, w.x, part[0][j]))));
                part[1][j] = fmaf(xb.w, w.w, fmaf(xb.z, w.z, fmaf(xb.y, w.y, fmaf(xb.x, w.x, part[1][j]))));
            }
        }
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            acc[0][j] += part[0][j];
            acc[1][j] += part[1][j];
        }
    }

    const float t = wide_temperature(temperature, clamp);
    // BWD: this lane's part of sum dl * (logit - the row's largest logit), in fp64.  sum_m dl_m = 0 in every row, so the
    // shift leaves dt as it is; it takes the common part of the logits, which only cancels, out of the products.
    double dtl = 0.0;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = grp * 2 + rr, row = row0 + r;
        float l[MPL], p[MPL];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = g + 16 * j;
            l[j] = m < M ? acc[rr][j] + bs[m] : 0.f;
            p[j] = m < M ? l[j] / t : -INFINITY;
            mx = fmaxf(mx, p[j]);
        }
        mx = group16_max(mx);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            p[j] = expf(p[j] - mx);      // absent slices: exp(-inf) = 0
            s += p[j];
        }
        s = group16_sum(s);
#pragma unroll
        for (int j = 0; j < MPL; ++j) p[j] = p[j] / s;
        if (!BWD) {
            if (row < rows) {
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = g + 16 * j;
                    if (m < M) sw[(size_t)row * M + m] = p[j];
                }
            }
        } else {
            float gsw[MPL];
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = g + 16 * j;
                gsw[j] = (row < rows && m < M) ? dsw[(size_t)row * M + m] : 0.f;
                dot = fmaf(p[j], gsw[j], dot);
            }
            dot = group16_sum(dot);
            float lmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < MPL; ++j)
                if (g + 16 * j < M) lmax = fmaxf(lmax, l[j]);
            lmax = group16_max(lmax);
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = g + 16 * j;
                const float dl = p[j] * (gsw[j] - dot) / t;      // 0 for absent slices and rows (p or dsw is 0)
                dtl += (double)dl * ((double)l[j] - (double)lmax);
                dls[r * DLP + m] = dl;
                if (row < rows && m < Mp) dlbuf[(size_t)row * Mp + m] = dl;
            }
        }
    }
    if (!BWD) return;

    {   // per-workgroup partial of sum dl * logit, added in a fixed order
        const double w = block_sum_f64(dtl, red);      // its barriers also complete the dl tile
        if (tid == 0) dtpart[blockIdx.x] = w;
    }
    if (!dx) return;
    // dx[32][D] = dl[32][M] . Ws[M][D]: thread = (row, four columns) of each 32-column chunk
    const int r = tid >> 3, c4 = tid & 7, row = row0 + r;
    for (int d0 = 0; d0 < D; d0 += W_DC) {
        __syncthreads();
        wide_stage_ws(Ws, wsm, M, D, d0, MR);
        __syncthreads();
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int m = 0; m < M; ++m) {
            const float dl = dls[r * DLP + m];
            const float4 w = *reinterpret_cast<const float4*>(&wsm[m][c4 * 4]);
            o.x = fmaf(dl, w.x, o.x);
            o.y = fmaf(dl, w.y, o.y);
            o.z = fmaf(dl, w.z, o.z);
            o.w = fmaf(dl, w.w, o.w);
        }
        const int col = d0 + c4 * 4;
        if (row < rows && col < D) *reinterpret_cast<float4*>(dx + (size_t)row * lddx + col) = o;
    }
}

// last pass of the backward: dt = -(1/t) * sum of the per-workgroup partials (fp64, fixed order; zero where the clamp is
// active), and, where M is not a multiple of 4, the first M rows of the padded weight / bias gradients to their places
__global__ __launch_bounds__(NT) void wide_sw_finish_kernel(const double* __restrict__ dtpart, int nblk,
                                                           const float* __restrict__ temperature, int clamp,
                                                           float* __restrict__ dt, const float* __restrict__ padded,
                                                           float* __restrict__ dws, float* __restrict__ dbs, int M, int Mp,
                                                           int D, int accumulate) {
    __shared__ double red[4];
    if (blockIdx.x == 0) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nblk; i += NT) s += dtpart[i];
        s = block_sum_f64(s, red);
        if (threadIdx.x == 0) {
            const float tv = temperature[0];
            const bool off = clamp && (tv < 0.1f || tv > 5.0f);
            const float t = wide_temperature(temperature, clamp);
            const float v = off ? 0.f : (float)(-s / (double)t);
            dt[0] = accumulate ? dt[0] + v : v;
        }
        return;
    }
    if (!padded) return;
    const long long idx = (long long)(blockIdx.x - 1) * NT + threadIdx.x, MD = (long long)M * D;
    if (idx < MD) dws[idx] = accumulate ? dws[idx] + padded[idx] : padded[idx];
    else if (idx < MD + M) {
        const float v = padded[(size_t)Mp * D + (idx - MD)];
        dbs[idx - MD] = accumulate ? dbs[idx - MD] + v : v;
    }
}

static int wide_check(int rows, int D, int M) {
    if (D < 16 || D > 512 || (D & 3) || M < 1 || M > 128) return PA2D_ERR_UNSUPPORTED;
    return rows < 0 ? PA2D_ERR_ARG : PA2D_OK;
}
static bool wide_too_big(int rows, long long ld, int D) {
    return ((unsigned long long)(rows - 1) * ld + D) * 4ull >= 0xFFFFFFF0ull;
}
static int wide_mpl(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : (M <= 64 ? 4 : 8)); }
static size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace

extern "C" {

size_t pa2d_zscore_workspace(long long rows, int C) {
    if (rows <= 0 || C <= 0 || (C & 3)) return 0;
    return sizeof(double) * 2 * zscore_blocks(rows * (C / 4));
}

int pa2d_zscore_fwd(const float* x, long long ldx, float* y, double* stats, void* ws, size_t ws_bytes, long long rows, int C,
                    void* stream) {
    const int rc = zscore_check(rows, C, ldx);
    if (rc) return rc;
    if (rows <= 0) return PA2D_OK;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || !stats) return PA2D_ERR_ARG;
    if (!ws || ws_bytes < pa2d_zscore_workspace(rows, C)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int q4 = C / 4;
    const long long n4 = rows * q4;
    const int nb = zscore_blocks(n4);
    hipLaunchKernelGGL((zscore_partial_kernel<false>), dim3(nb), dim3(NT), 0, st, x, ldx, (const float*)nullptr, n4, q4,
                       ceil_div_ll(n4, nb), (double*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_fwd_kernel, dim3((unsigned)ceil_div_ll(n4, Z_MAP_V4)), dim3(NT), 0, st, x, ldx, y, stats,
                       (const double*)ws, nb, n4, q4);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

int pa2d_zscore_bwd(const float* dy, long long lddy, const float* y, const double* stats, float* dx, long long lddx, void* ws,
                    size_t ws_bytes, long long rows, int C, void* stream) {
    int rc = zscore_check(rows, C, lddy);
    if (!rc) rc = zscore_check(rows, C, lddx);
    if (rc) return rc;
    if (rows <= 0) return PA2D_OK;
    if (((uintptr_t)dy & 15) || ((uintptr_t)y & 15) || ((uintptr_t)dx & 15) || !stats) return PA2D_ERR_ARG;
    if (!ws || ws_bytes < pa2d_zscore_workspace(rows, C)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int q4 = C / 4;
    const long long n4 = rows * q4;
    const int nb = zscore_blocks(n4);
    hipLaunchKernelGGL((zscore_partial_kernel<true>), dim3(nb), dim3(NT), 0, st, dy, lddy, y, n4, q4, ceil_div_ll(n4, nb),
                       (double*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_bwd_kernel, dim3((unsigned)ceil_div_ll(n4, Z_MAP_V4)), dim3(NT), 0, st, dy, lddy, y, stats, dx,
                       lddx, (const double*)ws, nb, n4, q4);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

size_t pa2d_zscore_grouped_workspace(int groups, long long rows_per_group, int C) {
    if (groups < 1 || groups > Z_MAX_GROUPS) return 0;
    return (size_t)groups * pa2d_zscore_workspace(rows_per_group, C);
}

int pa2d_zscore_grouped_fwd(const float* x, long long ldx, float* y, double* stats, void* ws, size_t ws_bytes, int groups,
                            long long rows_per_group, int C, void* stream) {
    const int rc = zscore_grouped_check(groups, rows_per_group, C, ldx);
    if (rc) return rc;
    if (rows_per_group <= 0) return PA2D_OK;
    if (!x || !y || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || !stats) return PA2D_ERR_ARG;
    if (!ws || ws_bytes < pa2d_zscore_grouped_workspace(groups, rows_per_group, C)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int q4 = C / 4;
    const long long n4 = rows_per_group * q4;      // per group: the partition of an ungrouped call on its rows
    const int nb = zscore_blocks(n4);
    hipLaunchKernelGGL((zscore_partial_kernel<false>), dim3(nb, groups), dim3(NT), 0, st, x, ldx, (const float*)nullptr, n4,
                       q4, ceil_div_ll(n4, nb), (double*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_fwd_kernel, dim3((unsigned)ceil_div_ll(n4, Z_MAP_V4), groups), dim3(NT), 0, st, x, ldx, y,
                       stats, (const double*)ws, nb, n4, q4);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

int pa2d_zscore_grouped_bwd(const float* dy, long long lddy, const float* y, const double* stats, float* dx, long long lddx,
                            void* ws, size_t ws_bytes, int groups, long long rows_per_group, int C, void* stream) {
    int rc = zscore_grouped_check(groups, rows_per_group, C, lddy);
    if (!rc) rc = zscore_grouped_check(groups, rows_per_group, C, lddx);
    if (rc) return rc;
    if (rows_per_group <= 0) return PA2D_OK;
    if (!dy || !y || !dx || ((uintptr_t)dy & 15) || ((uintptr_t)y & 15) || ((uintptr_t)dx & 15) || !stats)
        return PA2D_ERR_ARG;
    if (!ws || ws_bytes < pa2d_zscore_grouped_workspace(groups, rows_per_group, C)) return PA2D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int q4 = C / 4;
    const long long n4 = rows_per_group * q4;
    const int nb = zscore_blocks(n4);
    hipLaunchKernelGGL((zscore_partial_kernel<true>), dim3(nb, groups), dim3(NT), 0, st, dy, lddy, y, n4, q4,
                       ceil_div_ll(n4, nb), (double*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_bwd_kernel, dim3((unsigned)ceil_div_ll(n4, Z_MAP_V4), groups), dim3(NT), 0, st, dy, lddy, y,
                       stats, dx, lddx, (const double*)ws, nb, n4, q4);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

int pa2d_wide_slice_weights_fwd(const float* x, long long ldx, const float* ws, const float* bs, const float* temperature,
                                float* sw, int rows, int D, int M, int clamp_temperature, void* stream, void* ev_start,
                                void* ev_stop) {
    const int rc = wide_check(rows, D, M);
    if (rc) return rc;
    if (rows == 0) return PA2D_OK;
    if (ldx < D || (ldx & 3) || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return PA2D_ERR_ARG;
    if (wide_too_big(rows, ldx, D) || wide_too_big(rows, M, M)) return PA2D_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(rows, W_ROWS));
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_WF(MPL_)                                                                                                    \
    hipLaunchKernelGGL((wide_sw_kernel<MPL_, false>), grid, dim3(NT), 0, st, x, ldx, ws, bs, temperature, sw,            \
                       (const float*)nullptr, (float*)nullptr, 0LL, (float*)nullptr, (double*)nullptr, rows, D, M, 0,     \
                       clamp_temperature)
    switch (wide_mpl(M)) {
        case 1: CALL_WF(1); break;
        case 2: CALL_WF(2); break;
        case 4: CALL_WF(4); break;
        default: CALL_WF(8); break;
    }
#undef CALL_WF
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    return PA2D_OK;
}

// workspace: [dl rows x Mp | per-workgroup dt partials (fp64) | padded dWs, dbs (M % 4 != 0 only) | weight-gradient GEMM scratch]
size_t pa2d_wide_slice_weights_bwd_workspace(int rows, int D, int M) {
    if (wide_check(rows, D, M) || rows == 0) return 0;
    const size_t Mp = round4(M);
    const size_t pad = (M & 3) ? Mp * D + Mp : 0;
    return sizeof(float) * ((size_t)rows * Mp + round4(2 * (size_t)ceil_div(rows, W_ROWS)) + pad) +
           pa2d_gemm_bwd_weight_workspace(rows, (int)Mp, D, 0);
}

int pa2d_wide_slice_weights_bwd(const float* x, long long ldx, const float* ws, const float* bs, const float* temperature,
                                const float* dsw, float* dx, long long lddx, float* dws, float* dbs, float* dtemperature,
                                void* ws_buf, size_t ws_bytes, int rows, int D, int M, int clamp_temperature, int accumulate,
                                void* stream, void* ev_start, void* ev_stop) {
    int rc = wide_check(rows, D, M);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        if (accumulate) return PA2D_OK;
        if ((rc = pa2d_zero(dws, sizeof(float) * M * D, st))) return rc;
        if ((rc = pa2d_zero(dbs, sizeof(float) * M, st))) return rc;
        return pa2d_zero(dtemperature, sizeof(float), st);
    }
    if (!dws || !dbs || !dtemperature) return PA2D_ERR_ARG;
    if (ldx < D || (ldx & 3) || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return PA2D_ERR_ARG;
    if (dx && (lddx < D || (lddx & 3) || ((uintptr_t)dx & 15))) return PA2D_ERR_ARG;
    if (wide_too_big(rows, ldx, D) || (dx && wide_too_big(rows, lddx, D)) || wide_too_big(rows, M, M))
        return PA2D_ERR_UNSUPPORTED;
    if (!ws_buf || ws_bytes < pa2d_wide_slice_weights_bwd_workspace(rows, D, M)) return PA2D_ERR_WORKSPACE;
    const int Mp = (int)round4(M), nblk = ceil_div(rows, W_ROWS);
    float* const dl = (float*)ws_buf;
    float* const after_dl = dl + (size_t)rows * Mp;      // 16-byte aligned: Mp % 4 == 0
    double* const dtpart = (double*)after_dl;
    float* const padded = (M & 3) ? after_dl + round4(2 * (size_t)nblk) : nullptr;
    float* const gws = after_dl + round4(2 * (size_t)nblk) + ((M & 3) ? (size_t)Mp * D + Mp : 0);
    const size_t gbytes = pa2d_gemm_bwd_weight_workspace(rows, Mp, D, 0);
    const dim3 grid(nblk);
    if (ev_start && hipEventRecord((hipEvent_t)ev_start, st) != hipSuccess) return PA2D_ERR_ARG;
#define CALL_WB(MPL_)                                                                                                     \
    hipLaunchKernelGGL((wide_sw_kernel<MPL_, true>), grid, dim3(NT), 0, st, x, ldx, ws, bs, temperature, (float*)nullptr, \
                       dsw, dx, lddx, dl, dtpart, rows, D, M, Mp, clamp_temperature)
    switch (wide_mpl(M)) {
        case 1: CALL_WB(1); break;
        case 2: CALL_WB(2); break;
        case 4: CALL_WB(4); break;
        default: CALL_WB(8); break;
    }
#undef CALL_WB
    PA2D_CHECK_LAUNCH();
    if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, st) != hipSuccess) return PA2D_ERR_ARG;
    // dWs [M, D] = dl^T . x and dbs = column sums of dl on the exact-fp32 weight-gradient GEMM (fixed-order slab reduce)
    if (padded) rc = pa2d_gemm_bwd_weight(dl, Mp, x, ldx, padded, padded + (size_t)Mp * D, gws, gbytes, rows, Mp, D, 0, 0, st);
    else rc = pa2d_gemm_bwd_weight(dl, Mp, x, ldx, dws, dbs, gws, gbytes, rows, M, D, accumulate, 0, st);
    if (rc) return rc;
    const int fin = 1 + (padded ? ceil_div(M * D + M, NT) : 0);
    hipLaunchKernelGGL(wide_sw_finish_kernel, dim3(fin), dim3(NT), 0, st, dtpart, nblk, temperature, clamp_temperature,
                       dtemperature, padded, dws, dbs, M, Mp, D, accumulate);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
