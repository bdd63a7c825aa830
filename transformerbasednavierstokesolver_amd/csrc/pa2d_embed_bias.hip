// The input embedding's broadcast adds of TransolverBase (model/_core.py; reference …_2D.py:205-215), one launch each way:
//   z[b, n, :] = (h[b, n, :] + placeholder[:]) + tvec[b, :]
// h is the preprocess MLP's output [B, N, C], placeholder the [C] parameter, tvec = time_fc(timestep embedding) [B, C];
// either addend may be NULL.  The sums and their order per element are those of the torch expressions they replace
// (`h + placeholder[None, None, :]`, then `+ tvec[:, None, :]`), so the result is the same bits.
//   * pa2d_embed_bias_fwd : float4 stream over [B N C / 4]; z may be h (in place).
//   * pa2d_embed_bias_bwd : dh IS dz (the caller hands it on), so the only work is the column reduction
//                           dtvec[b, c] = sum_n dz[b, n, c] and dplaceholder[c] = sum_b dtvec[b, c].  Workgroups over
//                           (row chunks, B) add their rows into one [C] record each; one pass adds a sample's records
//                           in chunk order (double) and then the samples in order: no float atomics, same bits on
//                           every call.  Without tvec the rows of all samples are one [B N, C] matrix reduced straight
//                           to [C].
// C % 4 == 0 and 16-byte aligned operands (every access is a float4); anything else is refused, and the caller keeps
// the torch expression.
#include "pa2d_internal.h"

#define EB_THREADS 256
#define EB_CHUNKS 64                 // == PA2D_EMBED_BIAS_CHUNKS (include/pa2d.h)

__global__ __launch_bounds__(EB_THREADS) void embed_bias_fwd_kernel(const float4* h /* may be z */,
                                                                    const float4* __restrict__ placeholder,
                                                                    const float4* __restrict__ tvec, float4* z,
                                                                    long long total4, long long per_sample4, int C4) {
    for (long long i = (long long)blockIdx.x * EB_THREADS + threadIdx.x; i < total4;
         i += (long long)gridDim.x * EB_THREADS) {
        const int c = (int)(i % C4);
        float4 v = h[i];
        if (placeholder) {
            const float4 p = placeholder[c];
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        if (tvec) {
            const float4 t = tvec[(i / per_sample4) * C4 + c];
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        z[i] = v;
    }
}

// dz: [S][R][C4] float4; workgroup (chunk, s) adds rows [chunk * rows_per, ...) of sample s into partial[s][chunk][C4].
// Thread t: column group t % W, row lane t / W (W = min(C4, 256) columns side by side, 256 / W rows at a time).
__global__ __launch_bounds__(EB_THREADS) void embed_bias_colsum_kernel(const float4* __restrict__ dz, long long R,
                                                                       long long rows_per, int C4,
                                                                       float4* __restrict__ partial) {
    __shared__ float4 lds[EB_THREADS];
    const int W = C4 < EB_THREADS ? C4 : EB_THREADS, RL = EB_THREADS / W;
    const int cw = threadIdx.x % W, rl = threadIdx.x / W;
    int RLP = 1;                                          // the power of two >= RL
    while (RLP < RL) RLP <<= 1;
    const long long r0 = (long long)blockIdx.x * rows_per;
    const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
    const float4* src = dz + (size_t)blockIdx.y * R * C4;
    float4* dst = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C4;
    for (int cg0 = 0; cg0 < C4; cg0 += W) {
        const int cg = cg0 + cw;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rl < RL && cg < C4)
            for (long long r = r0 + rl; r < r1; r += RL) {
                const float4 v = src[r * C4 + cg];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        __syncthreads();
        lds[threadIdx.x] = a;
        __syncthreads();
        for (int s = RLP >> 1; s > 0; s >>= 1) {          // pairwise over the row lanes: rows [0, s) take rows [s, 2s)
            if (rl < s && rl + s < RL) {
                const float4 v = lds[threadIdx.x + s * W];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
                lds[threadIdx.x] = a;
            }
            __syncthreads();
        }
        if (rl == 0 && cg < C4) dst[cg] = a;
    }
}

// partial: [S][nchunk][C]; dtvec[s][c] = sum over the chunks in order (may be NULL), dplaceholder[c] = sum over s in order
// of those per-sample sums, rounded to float first (may be NULL)
__global__ __launch_bounds__(EB_THREADS) void embed_bias_finish_kernel(const float* __restrict__ partial, int S,
                                                                       int nchunk, int C, float* __restrict__ dtvec,
                                                                       float* __restrict__ dplaceholder) {
    const int c = blockIdx.x * EB_THREADS + threadIdx.x;
    if (c >= C) return;
    double all = 0.;
    for (int s = 0; s < S; ++s) {
        const float* p = partial + (size_t)s * nchunk * C + c;
        double acc = 0.;
        for (int k = 0; k < nchunk; ++k) acc += p[(size_t)k * C];
        const float f = (float)acc;
        if (dtvec) dtvec[(size_t)s * C + c] = f;
        all += f;
    }
    if (dplaceholder) dplaceholder[c] = (float)all;
}

static int eb_nchunk(long long R, int C4) {
    long long n = ceil_div_ll(R * C4, 4096);      // at least 16 float4 per lane and workgroup
    if (n > EB_CHUNKS) n = EB_CHUNKS;
    if (n > R) n = R;
    return n < 1 ? 1 : (int)n;
}

extern "C" {

// z[b, n, :] = (h[b, n, :] + placeholder[:]) + tvec[b, :]; placeholder [C] and tvec [B, C] may each be NULL; z may be h
int pa2d_embed_bias_fwd(const float* h, const float* placeholder, const float* tvec, float* z, int B, int N, int C,
                        hipStream_t st) {
    if (B < 0 || N < 0 || C < 1) return PA2D_ERR_ARG;
    if (C % 4) return PA2D_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return PA2D_OK;
    if ((((uintptr_t)h) | ((uintptr_t)placeholder) | ((uintptr_t)tvec) | ((uintptr_t)z)) & 15) return PA2D_ERR_ARG;
    const int C4 = C / 4;
    const long long per4 = (long long)N * C4, total4 = per4 * B;
    long long nb = ceil_div_ll(total4, EB_THREADS * 4);
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(embed_bias_fwd_kernel, dim3((int)nb), dim3(EB_THREADS), 0, st, (const float4*)h,
                       (const float4*)placeholder, (const float4*)tvec, (float4*)z, total4, per4, C4);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

// dz [B, N, C] -> dtvec [B, C] (NULL: no time vector) and dplaceholder [C] (NULL: no placeholder), both overwritten.
// ws: at least PA2D_EMBED_BIAS_CHUNKS * (dtvec ? B : 1) * C floats.  B * N == 0: the outputs are zero-filled.
int pa2d_embed_bias_bwd(const float* dz, float* dplaceholder, float* dtvec, void* ws, size_t ws_bytes, int B, int N,
                        int C, hipStream_t st) {
    if (B < 0 || N < 0 || C < 1) return PA2D_ERR_ARG;
    if (C % 4) return PA2D_ERR_UNSUPPORTED;
    if (!dplaceholder && !dtvec) return PA2D_OK;
    if (B == 0 || N == 0) {
        int rc = pa2d_zero(dplaceholder, sizeof(float) * (size_t)C, st);
        if (rc == PA2D_OK) rc = pa2d_zero(dtvec, sizeof(float) * (size_t)B * C, st);
        return rc;
    }
    if ((((uintptr_t)dz) | ((uintptr_t)ws)) & 15) return PA2D_ERR_ARG;
    const int S = dtvec ? B : 1;                                  // samples kept apart in the reduction
    const long long R = dtvec ? N : (long long)B * N;             // rows per such sample
    if (S > 65535) return PA2D_ERR_UNSUPPORTED;
    if (ws_bytes < sizeof(float) * (size_t)EB_CHUNKS * S * C) return PA2D_ERR_WORKSPACE;
    const int C4 = C / 4, nchunk = eb_nchunk(R, C4);
    const long long rows_per = ceil_div_ll(R, nchunk);
    hipLaunchKernelGGL(embed_bias_colsum_kernel, dim3(nchunk, S), dim3(EB_THREADS), 0, st, (const float4*)dz, R, rows_per,
                       C4, (float4*)ws);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_bias_finish_kernel, dim3(ceil_div(C, EB_THREADS)), dim3(EB_THREADS), 0, st, (const float*)ws,
                       S, nchunk, C, dtvec, dplaceholder);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
