// Reductions over the 64 lanes of a wavefront for the kernels whose summation order is part of their header's definition
// (csrc/diag/, csrc/hier/ and the libraries on its records).  Internal and of internal linkage.
#ifndef ISO_COMMON_WAVE_REDUCE_H
#define ISO_COMMON_WAVE_REDUCE_H

#include <hip/hip_runtime.h>
#include <math.h>

namespace {

// xor butterflies over the 64 lanes, distances 32 .. 1: every lane ends with the same value, in a fixed order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

#endif
