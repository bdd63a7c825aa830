// Training-mode dropout of the Physics-Attention output (Physics_Attention.py:28 `to_out = Sequential(Linear, Dropout)`
// and the block's residual add, Transolver_*.py `Attn(ln_1(fx)) + fx`) as one flat streaming kernel:
//     out[e] = (res ? res[e] : 0) + (keep(e) ? z[e] * scale : 0)
// with keep(e) from the draw (seed, offset) of pa2d_philox.h.  The forward calls it with z = to_out(y), res = fx; the
// backward with z = dout, res = null, which regenerates the mask instead of reading a saved one.  HBM-bound: one Philox
// evaluation (about 60 integer operations) per four elements rides under the 32 to 48 bytes they move.
#include "pa2d_internal.h"
#include "pa2d_philox.h"

#define DROP_THREADS 256
#define DROP_MAX_BLOCKS 2048      // include/pa2d.h: PA2D_DROPOUT_TRIP = DROP_MAX_BLOCKS * DROP_THREADS * 4 elements per trip

// one thread = the groups g, g + stride, ... of four consecutive elements (one counter each).  VEC: z, res and out are
// 16-byte aligned, whole groups move as float4; the last, partial group and the unaligned case go element by element.
template <bool VEC>
__global__ __launch_bounds__(DROP_THREADS) void dropout_residual_kernel(const float* __restrict__ z, const float* __restrict__ res,
                                                                        float* __restrict__ out, long long n, unsigned thresh,
                                                                        float scale, unsigned long long seed,
                                                                        unsigned long long offset) {
#pragma clang fp contract(off)      // product and sum round separately, on both paths alike
    const long long ngroups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * DROP_THREADS + threadIdx.x; g < ngroups; g += (long long)gridDim.x * DROP_THREADS) {
        const Pa2dPhilox4 r = pa2d_dropout_words(seed, offset, (unsigned long long)g);
        const long long e0 = 4 * g;
        if (VEC && e0 + 4 <= n) {
            const float4 zv = *reinterpret_cast<const float4*>(z + e0);
            float4 o = res ? *reinterpret_cast<const float4*>(res + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (r.w[0] >= thresh) o.x += zv.x * scale;
            if (r.w[1] >= thresh) o.y += zv.y * scale;
            if (r.w[2] >= thresh) o.z += zv.z * scale;
            if (r.w[3] >= thresh) o.w += zv.w * scale;
            *reinterpret_cast<float4*>(out + e0) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j < n) {
                    float o = res ? res[e0 + j] : 0.f;
                    if (r.w[j] >= thresh) o += z[e0 + j] * scale;
                    out[e0 + j] = o;
                }
            }
        }
    }
}

extern "C" {

int pa2d_dropout_keep_host(unsigned long long seed, unsigned long long offset, unsigned long long first,
                           unsigned long long count, unsigned thresh, unsigned char* keep) {
    if (count && !keep) return PA2D_ERR_ARG;
    for (unsigned long long i = 0; i < count; ++i) keep[i] = pa2d_dropout_keep(seed, offset, first + i, thresh) ? 1 : 0;
    return PA2D_OK;
}

int pa2d_dropout_residual(const float* z, const float* res, float* out, long long n, unsigned thresh, float scale,
                          unsigned long long seed, unsigned long long offset, hipStream_t st) {
    if (n <= 0) return PA2D_OK;
    if (!z || !out || (((uintptr_t)z | (uintptr_t)res | (uintptr_t)out) & 3)) return PA2D_ERR_ARG;
    long long blocks = ceil_div_ll(ceil_div_ll(n, 4), DROP_THREADS);
    if (blocks > DROP_MAX_BLOCKS) blocks = DROP_MAX_BLOCKS;
    const bool vec = !(((uintptr_t)z | (uintptr_t)res | (uintptr_t)out) & 15);
    if (vec)
        hipLaunchKernelGGL(dropout_residual_kernel<true>, dim3((unsigned)blocks), dim3(DROP_THREADS), 0, st, z, res, out, n,
                           thresh, scale, seed, offset);
    else
        hipLaunchKernelGGL(dropout_residual_kernel<false>, dim3((unsigned)blocks), dim3(DROP_THREADS), 0, st, z, res, out, n,
                           thresh, scale, seed, offset);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
