// Device helpers and record layout shared by the two "slice weights from the code" stages: pa2d_code_slice_weights.hip
// (two point coordinates, a rank-2 point term per row) and pa2d_point_slice_weights.hip (P point features, the point term
// made once per point).  Both run weight_projection = MLP(C+P, 64, 1) with one hidden layer on rows (point, slice).
#pragma once
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

// points per workgroup: a multiple of the points per tile, about `target` workgroups in all
int points_per_block(int B, int N, int pt, int target) {
    int nx = ceil_div(target, B);
    const int maxc = ceil_div(N, pt);
    if (nx > maxc) nx = maxc;
    if (nx < 1) nx = 1;
    return ceil_div(ceil_div(N, nx), pt) * pt;
}

}  // namespace
