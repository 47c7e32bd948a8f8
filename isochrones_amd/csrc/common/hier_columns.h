// The columns of include/isochrones_amd_hier.h (an iso_hier_column: one column of a stored chain, in a storage of its own)
// as the libraries that read them see them: the check of a column's storage with its messages, the column as a kernel
// reads it and the load of one sample, for host and device code.  Internal and of internal linkage.
#ifndef ISO_COMMON_HIER_COLUMNS_H
#define ISO_COMMON_HIER_COLUMNS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "isochrones_amd_hier.h"
#include "chain_view.h"

namespace {

static_assert(ISO_HIER_ROW_MAJOR == CHAIN_ROW_MAJOR && ISO_HIER_PARAM_MAJOR == CHAIN_PARAM_MAJOR, "chain layouts");

// one column as a kernel reads it: sample (t, w) of ensemble s at base[t * st_t + ((s - first) * W + w) * st_w]
struct DevCol {
    const double* base;                         // the storage's first double of the column
    int64_t st_t, st_w;
    int32_t first, pad;
};

__host__ __device__ __forceinline__ double load(const DevCol& c, int s, int W, int t, int w) {
    return c.base[(int64_t)t * c.st_t + ((int64_t)(s - c.first) * W + w) * c.st_w];
}

inline DevCol dev_col(const iso_hier_column& c, int layout, int32_t W) {
    const ChainStrides st = chain_strides(layout, (int64_t)c.n_ens * W, c.ncols);
    return DevCol{c.base + (int64_t)c.col * st.st_d, st.st_t, st.st_w, c.first, 0};
}

// what is wrong with a column's storage for the ensembles [ens_begin, ens_begin + n_ens_out) of W walkers, or nullptr
inline const char* column_error(const iso_hier_column& c, int32_t W, int32_t ens_begin, int32_t n_ens_out) {
    if (!c.base) return "null column storage";
    if (c.ncols < 1 || c.col < 0 || c.col >= c.ncols) return "a column index is outside [0, ncols)";
    if (c.n_ens < 1 || (int64_t)c.n_ens * W > INT32_MAX) return "a column storage's n_ens must be at least 1 and n_ens * W below 2^31";
    if (c.first < 0 || c.first > ens_begin || (int64_t)ens_begin + n_ens_out > (int64_t)c.first + c.n_ens)
        return "a column storage does not hold the ensembles [ens_begin, ens_begin + n_ens_out)";
    return nullptr;
}

}  // namespace

#endif
