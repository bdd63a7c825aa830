// The exact bf16 operand split and the bf16-MFMA helpers built on it (gfx950 / CDNA4): the one home of this code for the
// v3 slice kernels (pa2d_slice3.hip, pa2d_slice3_bwd.hip) and the split-engine GEMMs (pa2d_gemm_common.h), including the
// two term orders (mfma_terms: slice kernels; split_terms: GEMMs and convs) and the transposed fragment read.
//
// An fp32 value is carried as up to three bf16 planes, x = p0 + p1 + p2 up to 2^-25 |x|; a product of two split operands
// keeps the terms a[i] * b[j] with i + j <= 2 on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: a 24-bit significand.
#pragma once
#include "pa2d_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ f32x4 mfma_bf(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Exact split x = p0 + p1 + p2 (up to 2^-25 |x|) into bf16 planes, for 8 floats (NP planes of one MFMA fragment each) and
// for 4 floats (hi, mid, lo).  Both are written on the PACKED conversion result: the straightforward scalar form makes hipcc
// convert every element a second time on its own to build the residual (7.5 instructions per element); per pair this is
// 3 v_cvt_pk_bf16_f32 + 2 x (v_lshlrev, v_and, v_pk_add_f32) = 4.5.  They are two texts on purpose: folding them onto one
// per-pair helper computes the same values but changes the instruction order of 66 kernels that use them.
template <int NP>
__device__ __forceinline__ void split8(const f32x8 x, bf16x8 (&pl)[NP]) {
    u32x4 p0, p1, p2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 a = {x[2 * q], x[2 * q + 1]};
        const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2));
        p0[q] = h;
        if constexpr (NP > 1) {
            const f32x2 hf = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
            const f32x2 r = a - hf;                                  // explicit vector op -> v_pk_add_f32
            const unsigned m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
            p1[q] = m;
            if constexpr (NP > 2) {
                const f32x2 mf = {__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};
                p2[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(r - mf, bf16x2));
            }
        }
    }
    pl[0] = __builtin_bit_cast(bf16x8, p0);
    if constexpr (NP > 1) pl[1] = __builtin_bit_cast(bf16x8, p1);
    if constexpr (NP > 2) pl[2] = __builtin_bit_cast(bf16x8, p2);
}
__device__ __forceinline__ void split3(const float4 v, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
    const f32x2 a[2] = {{v.x, v.y}, {v.z, v.w}};
    u32x2 ph, pm, pl;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(a[q], bf16x2));
        const f32x2 hf = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
        const f32x2 r1 = a[q] - hf;
        const unsigned m = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
        const f32x2 mf = {__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};
        const unsigned l = __builtin_bit_cast(unsigned, __builtin_convertvector(r1 - mf, bf16x2));
        ph[q] = h; pm[q] = m; pl[q] = l;
    }
    hi = __builtin_bit_cast(bf16x4, ph);
    mid = __builtin_bit_cast(bf16x4, pm);
    lo = __builtin_bit_cast(bf16x4, pl);
}

// planes kept per operand kind: activations (bf16 storage: the values ARE the one plane), parameters, softmax weights
template <typename T> struct Planes;
template <> struct Planes<float> { static constexpr int ACT = 3, PAR = 3, WGT = 3; };
template <> struct Planes<bf16_t> { static constexpr int ACT = 1, PAR = 3, WGT = 2; };

// acc + sum over the kept terms a[i] * b[j] (i + j <= 2, smallest first)
template <int NA, int NB>
__device__ __forceinline__ f32x4 mfma_terms(const bf16x8 (&a)[NA], const bf16x8 (&b)[NB], f32x4 acc) {
#pragma unroll
    for (int s = 2; s >= 0; --s)
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int j = s - i;
            if (j >= 0 && j < NB) acc = mfma_bf(a[i], b[j], acc);
        }
    return acc;
}

// The split-engine GEMMs (pa2d_gemm_split / _panel / _mc / _mc_planes, pa2d_conv_halo) keep the same six terms in ANOTHER
// order, (A plane, B plane) = (1,1) (2,0) (0,2) (1,0) (0,1) (0,0): still smallest first, but the three second-order terms
// start with (1,1) where mfma_terms (order of the slice kernels: (2,0) (1,1) (0,2) ...) starts with (2,0).  Both orders
// are older than this header and every result bit of an engine depends on its own, so neither moves: a new GEMM kernel of
// the split engine uses split_terms, a new slice kernel mfma_terms.  NT = 1 (bf16 compute) is the one term (0,0).
// The accumulator type selects the MFMA: f32x16 = v_mfma_f32_32x32x16_bf16 (a, b); f32x4 = v_mfma_f32_16x16x32_bf16 of the
// transposed product, b as the instruction's first operand (an accumulator quad = four consecutive columns of B's side).
// acc is a reference on purpose: returned by value, the compiler copies accumulators of the 256 x 256 weight-gradient kernel.
__device__ __forceinline__ void mfma_ab(const bf16x8& a, const bf16x8& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_ab(const bf16x8& a, const bf16x8& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, acc, 0, 0, 0);
}
template <int NT, typename ACC>
__device__ __forceinline__ void split_terms(const bf16x8 (&a)[NT], const bf16x8 (&b)[NT], ACC& acc) {
    if constexpr (NT == 3) {
        mfma_ab(a[1], b[1], acc);
        mfma_ab(a[2], b[0], acc);
        mfma_ab(a[0], b[2], acc);
        mfma_ab(a[1], b[0], acc);
        mfma_ab(a[0], b[1], acc);
    }
    mfma_ab(a[0], b[0], acc);
}

// two transposed LDS reads (ds_read_b64_tr_b16) = one 8-element MFMA fragment (elements 0..3 from base + off0, 4..7 from
// base + off1).  Base (stage / plane image) and the lane's two byte offsets are separate arguments: with complete pointers,
// or with the plane folded into the offsets, the compiler emits other address arithmetic in the weight-gradient kernels.
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* base, unsigned off0, unsigned off1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off1));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}
