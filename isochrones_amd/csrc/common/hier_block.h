// What the workgroups of the likelihood kernels on per-(hyper row, star) tables share (csrc/hier/, csrc/relation/,
// csrc/binned/): their size, and the total of a row over the stars, on the device and on the host.  Internal and of
// internal linkage.  The source writes no fused multiply-add; it is meant for -ffp-contract=off.
#ifndef ISO_COMMON_HIER_BLOCK_H
#define ISO_COMMON_HIER_BLOCK_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wave_reduce.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;

// the body of a k_*_total kernel, one workgroup per row: L and min_ess over the unmasked stars in a fixed order
__device__ __forceinline__ void row_total(const double* ell, const double* ess, const int32_t* mask, int n_ens, double* L,
                                          double* min_ess) {
    __shared__ double s_red[2 * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)blockIdx.x * (size_t)n_ens;
    double sum = 0.0, mn = HUGE_VAL;
    for (int s = tid; s < n_ens; s += BLOCK) {
        if (mask && mask[s] == 0) continue;
        sum += ell[row + s];
        mn = fmin(mn, ess[row + s]);
    }
    const double a = wave_sum(sum), b = wave_min(mn);
    if (lane == 0) {
        s_red[wave] = a;
        s_red[WAVES + wave] = b;
    }
    __syncthreads();
    if (tid == 0) {
        L[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        min_ess[blockIdx.x] = fmin(fmin(s_red[WAVES], s_red[WAVES + 1]), fmin(s_red[WAVES + 2], s_red[WAVES + 3]));
    }
}

// the host entries' totals: every row's stars in ascending order
inline void row_totals_host(const double* ell, const double* ess, const int32_t* mask, int32_t n_ens, int32_t H, double* L,
                            double* min_ess) {
    const size_t ld = (size_t)n_ens;
    for (int h = 0; h < H; ++h) {
        double sum = 0.0, mn = HUGE_VAL;
        for (int s = 0; s < n_ens; ++s) {
            if (mask && mask[s] == 0) continue;
            sum += ell[(size_t)h * ld + s];
            mn = fmin(mn, ess[(size_t)h * ld + s]);
        }
        L[h] = sum;
        min_ess[h] = mn;
    }
}

}  // namespace

#endif
