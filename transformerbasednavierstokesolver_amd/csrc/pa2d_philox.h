// Counter-based random words for training-mode dropout: Philox4x32-10 (Salmon et al., SC'11), the one definition the
// kernels and the host function pa2d_dropout_keep_host share.  A DRAW is (seed, offset, n): element e < n takes word e & 3
// of philox(counter = (lo32(offset + e/4), hi32(offset + e/4), 0, 0), key = (lo32(seed), hi32(seed))) and is KEPT iff that
// word >= thresh (thresh = floor(p 2^32), made on the host).  No mask is ever stored: the backward evaluates the same
// function again.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PA2D_HD __host__ __device__ __forceinline__
#else
#define PA2D_HD inline
#endif

struct Pa2dPhilox4 { uint32_t w[4]; };

PA2D_HD Pa2dPhilox4 pa2d_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Pa2dPhilox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// the four words of the elements 4 g .. 4 g + 3 of a draw (g = group index, e / 4)
PA2D_HD Pa2dPhilox4 pa2d_dropout_words(uint64_t seed, uint64_t offset, uint64_t group) {
    const uint64_t ctr = offset + group;
    return pa2d_philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// element e of a draw alone (one Philox evaluation; callers that walk consecutive elements use pa2d_dropout_words)
PA2D_HD bool pa2d_dropout_keep(uint64_t seed, uint64_t offset, uint64_t e, uint32_t thresh) {
    const Pa2dPhilox4 r = pa2d_dropout_words(seed, offset, e >> 2);
    const uint32_t j = (uint32_t)e & 3u;
    const uint32_t w = j == 0 ? r.w[0] : j == 1 ? r.w[1] : j == 2 ? r.w[2] : r.w[3];   // selects: no indexed register array
    return w >= thresh;
}
