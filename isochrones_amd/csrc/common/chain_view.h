// A stored ensemble chain as the libraries that post-process it see it (csrc/diag/, csrc/derived/, csrc/predict/): the
// strides of its two layouts, a component's packed parameter indices and the checks on its shape with their messages; it
// brings the library's last error (last_error.h) with it.  Internal, no part of any ABI, and of internal linkage.
#ifndef ISO_COMMON_CHAIN_VIEW_H
#define ISO_COMMON_CHAIN_VIEW_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "last_error.h"

namespace {

// the values of ISO_CHAIN_ROW_MAJOR / ISO_CHAIN_PARAM_MAJOR of isochrones_amd.h, which every library's own pair repeats
constexpr int CHAIN_ROW_MAJOR = 0, CHAIN_PARAM_MAJOR = 1;

struct ChainStrides {
    int64_t st_t, st_d, st_w;                   // strides of (step, parameter, row) in doubles
};

inline ChainStrides chain_strides(int layout, int64_t rows, int32_t ndim) {
    if (layout == CHAIN_PARAM_MAJOR) return {(int64_t)ndim * rows, rows, 1};
    return {rows * ndim, 1, ndim};
}

// the chain parameters (p0, p1, pk) a component reads its coordinates on (ax0, ax1, axk) from, each below 256
inline int32_t pack_comp(int32_t p0, int32_t p1, int32_t pk) { return p0 | p1 << 8 | pk << 16; }
__host__ __device__ inline int comp_p0(int32_t comp) { return comp & 255; }
__host__ __device__ inline int comp_p1(int32_t comp) { return (comp >> 8) & 255; }
__host__ __device__ inline int comp_pk(int32_t comp) { return (comp >> 16) & 255; }

struct ChainShape {
    int layout;
    int64_t nsteps;
    int32_t n_ens, W, ndim;
    int32_t ens_begin = 0, n_ens_out = 0;       // CHAIN_CHECK_RANGE
    const int32_t* comps = nullptr;             // CHAIN_CHECK_COMPS: [C][3], C already checked
    int32_t C = 0;
};

enum { CHAIN_CHECK_LAYOUT = 1, CHAIN_CHECK_SIZES = 2, CHAIN_CHECK_RANGE = 4, CHAIN_CHECK_ROWS = 8, CHAIN_CHECK_COMPS = 16 };

// What is wrong with the shape, or nullptr: the checks named in `checks`, in the order of the enumeration.  A library has
// checks of its own between these and reports the first that fails, so it asks for them a run at a time.
inline const char* chain_shape_error(int checks, const ChainShape& s) {
    if ((checks & CHAIN_CHECK_LAYOUT) && s.layout != CHAIN_ROW_MAJOR && s.layout != CHAIN_PARAM_MAJOR)
        return "unknown chain layout";
    if ((checks & CHAIN_CHECK_SIZES) && (s.nsteps < 1 || s.n_ens < 1 || s.W < 1 || s.ndim < 1))
        return "nsteps, n_ens, W and ndim must be at least 1";
    if ((checks & CHAIN_CHECK_RANGE) && (s.ens_begin < 0 || s.n_ens_out < 1 || (int64_t)s.ens_begin + s.n_ens_out > s.n_ens))
        return "ensemble range [ens_begin, ens_begin + n_ens_out) must be non-empty and inside [0, n_ens)";
    if ((checks & CHAIN_CHECK_ROWS) && (int64_t)s.n_ens * s.W > INT32_MAX) return "more than 2^31 - 1 rows (split the batch)";
    if (checks & CHAIN_CHECK_COMPS)
        for (int c = 0; c < s.C * 3; ++c)
            if (s.comps[c] < 0 || s.comps[c] >= s.ndim) return "a component's parameter index is outside [0, ndim)";
    return nullptr;
}

}  // namespace

#endif
