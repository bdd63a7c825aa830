// The loss of one exp_airfoil / exp_pipe / exp_elas / exp_plas iteration on the head output, per sample:
//   o = pred * std + mean, y = y_n * std + mean            (UnitTransformer.decode; both decoded, then subtracted, as
//   ratio_b = ||o - y|| / ||y||                              exp_pipe.py:210-213 and pa2d_darcy_loss do)
// mean / std are one-element device tensors (never read on the host); NULL for both is the identity (airfoil, plas).
// pred is [B, L] contiguous; the target is read through an element stride and a batch stride, so the plasticity target
// yy[..., t:t+1] of a [B, N, 4, T] tensor is consumed where it lies.
//   * pa2d_rel_l2_affine_fwd : workgroups over (split, B): unlike rel_l2_fwd_kernel (ONE workgroup per sample) a sample
//                              is spread over up to PA2D_REL_L2_AFFINE_SPLIT workgroups (these drivers run B = 1..8);
//                              each writes one (sum d^2, sum y^2) record, and a one-wave pass adds a sample's records in
//                              split order (double) -> the same bits every call, no float atomics.
//   * pa2d_rel_l2_affine_bwd : dpred = gout_b * std * (o - y) / (dnorm_b * ynorm_b); zero sub-gradient at dnorm_b == 0.
// 16-byte accesses on the part of a row where pred (and a unit-stride target, and dpred) are 16-byte aligned at the same
// elements; the row's head and tail, and rows whose operands disagree in phase or whose target is strided, go scalar.
#include "pa2d_internal.h"

#define RA_THREADS 256
#define RA_SPLIT 64                  // == PA2D_REL_L2_AFFINE_SPLIT (include/pa2d.h)
#define RA_CHUNK 1024                // elements one workgroup covers per pass: 256 lanes x 16 bytes

static __device__ __forceinline__ float ra_block_sum(float v, float* red /* [4] */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// elements in front of the first 16-byte boundary of a float row (at most L)
static __device__ __forceinline__ long long ra_head(const float* p, long long L) {
    const long long h = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return h < L ? h : L;
}

// partial: [B][nsplit][2] = (sum (o - y)^2, sum y^2) of the elements this workgroup covers
__global__ __launch_bounds__(RA_THREADS) void rel_l2_affine_fwd_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ y, long long yes,
                                                                       long long ybs, const float* __restrict__ mean,
                                                                       const float* __restrict__ stdv, long long L,
                                                                       float* __restrict__ partial) {
    __shared__ float red[4];
    const int k = blockIdx.x, nsplit = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const float mu = mean ? *mean : 0.f, sd = stdv ? *stdv : 1.f;
    const float* pb = pred + (size_t)b * L;
    const float* yb = y + (long long)b * ybs;
    float sdq = 0.f, syq = 0.f;
#define RA_ACC(P, Y)                                        \
    {                                                       \
        const float y_ = fmaf((Y), sd, mu);                 \
        const float d_ = fmaf((P), sd, mu) - y_;            \
        sdq += d_ * d_;                                     \
        syq += y_ * y_;                                     \
    }
    const long long head = ra_head(pb, L);
    const bool vec = yes == 1 && (((uintptr_t)(yb + head)) & 15) == 0;
    if (vec) {
        const long long n4 = (L - head) >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(pb + head);
        const float4* y4 = reinterpret_cast<const float4*>(yb + head);
        for (long long i = (long long)k * RA_THREADS + tid; i < n4; i += (long long)nsplit * RA_THREADS) {
            const float4 p = p4[i], t = y4[i];
            RA_ACC(p.x, t.x) RA_ACC(p.y, t.y) RA_ACC(p.z, t.z) RA_ACC(p.w, t.w)
        }
        if (k == 0) {                // the row's head and tail: fewer than 4 elements each
            if (tid < head) RA_ACC(pb[tid], yb[tid])
            const long long t0 = head + (n4 << 2);
            if (t0 + tid < L) RA_ACC(pb[t0 + tid], yb[t0 + tid])
        }
    } else {
        for (long long i = (long long)k * RA_THREADS + tid; i < L; i += (long long)nsplit * RA_THREADS)
            RA_ACC(pb[i], yb[i * yes])
    }
#undef RA_ACC
    const float td = ra_block_sum(sdq, red);
    const float ty = ra_block_sum(syq, red);
    if (tid == 0) {
        float* p = partial + ((size_t)b * nsplit + k) * 2;
        p[0] = td;
        p[1] = ty;
    }
}

// one wave: a lane adds the records of its samples in split order
__global__ __launch_bounds__(64) void rel_l2_affine_finish_kernel(const float* __restrict__ partial, int B, int nsplit,
                                                                  float* __restrict__ dnorm, float* __restrict__ ynorm,
                                                                  float* __restrict__ ratio) {
    for (int b = threadIdx.x; b < B; b += 64) {
        const float* p = partial + (size_t)b * nsplit * 2;
        double s0 = 0., s1 = 0.;
        for (int k = 0; k < nsplit; ++k) {
            s0 += p[2 * k];
            s1 += p[2 * k + 1];
        }
        const float d = sqrtf((float)s0), n = sqrtf((float)s1);
        dnorm[b] = d;
        ynorm[b] = n;
        ratio[b] = d / n;
    }
}

__global__ __launch_bounds__(RA_THREADS) void rel_l2_affine_bwd_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ y, long long yes,
                                                                       long long ybs, const float* __restrict__ mean,
                                                                       const float* __restrict__ stdv,
                                                                       const float* __restrict__ dnorm,
                                                                       const float* __restrict__ ynorm,
                                                                       const float* __restrict__ gout, long long L,
                                                                       float* __restrict__ dpred) {
    const int k = blockIdx.x, nsplit = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const float mu = mean ? *mean : 0.f, sd = stdv ? *stdv : 1.f;
    const float dn = dnorm[b];
    const float s = dn > 0.f ? gout[b] * sd / (dn * ynorm[b]) : 0.f;
    const float* pb = pred + (size_t)b * L;
    const float* yb = y + (long long)b * ybs;
    float* gb = dpred + (size_t)b * L;
#define RA_GRAD(P, Y) (s * (fmaf((P), sd, mu) - fmaf((Y), sd, mu)))
    const long long head = ra_head(pb, L);
    const bool vec = yes == 1 && ((((uintptr_t)(yb + head)) | ((uintptr_t)(gb + head))) & 15) == 0;
    if (vec) {
        const long long n4 = (L - head) >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(pb + head);
        const float4* y4 = reinterpret_cast<const float4*>(yb + head);
        float4* g4 = reinterpret_cast<float4*>(gb + head);
        for (long long i = (long long)k * RA_THREADS + tid; i < n4; i += (long long)nsplit * RA_THREADS) {
            const float4 p = p4[i], t = y4[i];
            g4[i] = make_float4(RA_GRAD(p.x, t.x), RA_GRAD(p.y, t.y), RA_GRAD(p.z, t.z), RA_GRAD(p.w, t.w));
        }
        if (k == 0) {
            if (tid < head) gb[tid] = RA_GRAD(pb[tid], yb[tid]);
            const long long t0 = head + (n4 << 2);
            if (t0 + tid < L) gb[t0 + tid] = RA_GRAD(pb[t0 + tid], yb[t0 + tid]);
        }
    } else {
        for (long long i = (long long)k * RA_THREADS + tid; i < L; i += (long long)nsplit * RA_THREADS)
            gb[i] = RA_GRAD(pb[i], yb[i * yes]);
    }
#undef RA_GRAD
}

static int ra_nsplit(long long L) {
    const long long n = ceil_div_ll(L, RA_CHUNK);
    return n > RA_SPLIT ? RA_SPLIT : (int)n;
}

extern "C" {

// dnorm, ynorm, ratio: [B]; ws: at least 2 * B * PA2D_REL_L2_AFFINE_SPLIT floats
int pa2d_rel_l2_affine_fwd(const float* pred, const float* y, long long y_elem_stride, long long y_batch_stride,
                           const float* mean, const float* stdv, float* dnorm, float* ynorm, float* ratio, void* ws,
                           size_t ws_bytes, int B, long long L, hipStream_t st) {
    if ((mean == nullptr) != (stdv == nullptr) || B < 0 || L < 0) return PA2D_ERR_ARG;
    if (B == 0 || L == 0) return PA2D_OK;
    if (((((uintptr_t)pred) | ((uintptr_t)y)) & 3) || y_elem_stride < 1) return PA2D_ERR_ARG;
    if (B > 65535) return PA2D_ERR_UNSUPPORTED;
    if (ws_bytes < sizeof(float) * 2 * (size_t)B * RA_SPLIT) return PA2D_ERR_WORKSPACE;
    const int nsplit = ra_nsplit(L);
    hipLaunchKernelGGL(rel_l2_affine_fwd_kernel, dim3(nsplit, B), dim3(RA_THREADS), 0, st, pred, y, y_elem_stride,
                       y_batch_stride, mean, stdv, L, (float*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(rel_l2_affine_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)ws, B, nsplit, dnorm, ynorm,
                       ratio);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// gout: the per-sample upstream gradient [B]; dpred: [B, L]
int pa2d_rel_l2_affine_bwd(const float* pred, const float* y, long long y_elem_stride, long long y_batch_stride,
                           const float* mean, const float* stdv, const float* dnorm, const float* ynorm,
                           const float* gout, float* dpred, int B, long long L, hipStream_t st) {
    if ((mean == nullptr) != (stdv == nullptr) || B < 0 || L < 0) return PA2D_ERR_ARG;
    if (B == 0 || L == 0) return PA2D_OK;
    if (((((uintptr_t)pred) | ((uintptr_t)y) | ((uintptr_t)dpred)) & 3) || y_elem_stride < 1) return PA2D_ERR_ARG;
    if (B > 65535) return PA2D_ERR_UNSUPPORTED;
    long long nb = ceil_div_ll(L, RA_CHUNK);
    if (nb > 256) nb = 256;
    hipLaunchKernelGGL(rel_l2_affine_bwd_kernel, dim3((int)nb, B), dim3(RA_THREADS), 0, st, pred, y, y_elem_stride,
                       y_batch_stride, mean, stdv, dnorm, ynorm, gout, L, dpred);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
