// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011) for host and device code: ten rounds on a 128-bit counter under a 64-bit
// key, integer arithmetic only, so host and device return the same words.  The samplers keep their own copy in
// fast/sampler.h (device only; its digest feeds the fused kernels); the rounds here are the same ones, pinned by the
// Random123 known-answer vectors in the tests.
// Internal and of internal linkage.
#ifndef ISO_COMMON_PHILOX_H
#define ISO_COMMON_PHILOX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// A uniform of 53 bits from two words: (hi * 2^21 + (lo & 0x1FFFFF) + 0.5) / 2^53.  The sum is an integer below 2^53 plus a
// half; above 2^52 the half rounds to even, so the largest integer would round to 2^53 and give 1: that one value is held
// at 1 - 2^-53.  Every step is exact or one correctly rounded operation, the same on host and device; 0 < u < 1.
__host__ __device__ inline double philox_uniform53(uint32_t hi, uint32_t lo) {
    const uint64_t m = ((uint64_t)hi << 21) | (uint64_t)(lo & 0x1FFFFFu);
    const double u = ((double)m + 0.5) * 1.1102230246251565e-16;          // 2^-53
    return u < 1.0 ? u : 0.99999999999999989;                             // 1 - 2^-53
}

}  // namespace

#endif
