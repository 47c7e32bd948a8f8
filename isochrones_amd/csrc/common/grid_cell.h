// Where a coordinate sits on a grid axis: the bracket, the on-axis rule and the NaN of every library that reads a packed
// grid.  csrc/solve/ includes it directly; csrc/derived/, csrc/predict/ and csrc/population/ through grid_interp.h, which
// builds the cells on it; csrc/diag/ and csrc/hier/ take qnan().  include/isochrones_amd_derived.h defines the bracket: an
// index and a fraction are the same bits in these libraries, kernel and host entry, because they compile these lines.
// Internal.
#ifndef ISO_COMMON_GRID_CELL_H
#define ISO_COMMON_GRID_CELL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ inline double qnan() {
    union { uint64_t u; double d; } x;
    x.u = 0x7ff8000000000000ULL;
    return x.d;
}

// i = the largest index with ax[i] <= x, at most n - 2; t = (x - ax[i]) / (ax[i + 1] - ax[i]).  Stays inside the axis for
// every x (a NaN compares false everywhere: i = 0); the caller has decided whether x is on the axis at all.
__host__ __device__ inline void bracket(const double* __restrict__ ax, int n, double x, int& i, double& t) {
    int base = 0, len = n;
    while (len > 1) {
        const int half = len >> 1;
        base = (ax[base + half] <= x) ? base + half : base;
        len -= half;
    }
    base = base < n - 2 ? base : n - 2;
    const double lo = ax[base], hi = ax[base + 1];
    i = base;
    t = (x - lo) / (hi - lo);
}

// NaN first, then the bounds test, as the interpolator
__host__ __device__ inline bool on_axis(const double* __restrict__ ax, int n, double x) {
    return x == x && !(x < ax[0]) && !(x > ax[n - 1]);
}

}  // namespace

#endif
