// Model-grid columns interpolated at every sample of a stored ensemble chain, for gfx950.  See
// include/isochrones_amd_derived.h for the definition and the order of the arithmetic, DESIGN.md section 14 for the
// mapping and what bounds the kernel.
//
// One kernel, one sample per lane, float64:
//   k_derived_chain  a work item is (step t, 256 consecutive rows of the ensemble range); workgroups stride over the
//                    items.  Lanes run along the row axis, the contiguous one of the parameter-major storage, so every
//                    parameter-row load and every output-row store of a wavefront is one contiguous run.  A sample
//                    brackets ax0 and ax1 once for all components that read the same two parameters, brackets axk per
//                    component, reads the eight corners of the cell - Q adjacent doubles each, two per load when Q is
//                    even - and writes Q output rows per component.  Q is a compile-time constant inside each branch of
//                    one wave-uniform switch, so the accumulators stay in registers.  A NaN value costs one vector
//                    atomic add on its (ensemble, column) counter; a fit's chain has none.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "isochrones_amd_derived.h"
#include "../common/chain_view.h"
#include "../common/grid_interp.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 256 * 8;             // a memory-bound stream: eight workgroups per CU, the rest by striding
constexpr int MAXC = ISO_DERIVED_MAX_COMPS;
static_assert(ISO_DERIVED_ROW_MAJOR == CHAIN_ROW_MAJOR && ISO_DERIVED_PARAM_MAJOR == CHAIN_PARAM_MAJOR, "chain layouts");

struct Args {
    const double* chain;
    double* out;
    int32_t* nan_count;
    iso_derived_table T;
    ChainStrides st;
    int64_t row0;                               // ens_begin * W
    int32_t R, W, C, nsteps;                    // R = n_ens_out * W
    int32_t chunks, items;                      // ceil(R / BLOCK), nsteps * chunks
    int32_t comp[MAXC];                         // pack_comp() | FRESH01 where (p0, p1) differ from the component
};                                              // before (the first component: always)

constexpr int FRESH01 = 1 << 24;

template <int Q>
__device__ __forceinline__ void derive(const Args& A) {
    const iso_derived_table& T = A.T;
    const int R = A.R, CQ = A.C * Q;
    for (int item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int t = item / A.chunks;
        const int r = (item - t * A.chunks) * BLOCK + (int)threadIdx.x;
        if (r >= R) continue;
        const double* __restrict__ row = A.chain + (int64_t)t * A.st.st_t + (A.row0 + r) * A.st.st_w;
        double* __restrict__ o = A.out + (int64_t)t * CQ * R + r;
        int i0 = 0, i1 = 0;
        double t0 = 0.0, t1 = 0.0;
        bool ok01 = false;
        for (int c = 0; c < A.C; ++c) {
            const int comp = c == 0 ? A.comp[0] : (c == 1 ? A.comp[1] : A.comp[2]);      // wave-uniform
            // the first two axes: once for every run of components that read them from the same parameters
            if (comp & FRESH01) {
                const double x0 = row[comp_p0(comp) * A.st.st_d], x1 = row[comp_p1(comp) * A.st.st_d];
                ok01 = on_axis(T.ax0, T.n0, x0) && on_axis(T.ax1, T.n1, x1);
                bracket(T.ax0, T.n0, x0, i0, t0);
                bracket(T.ax1, T.n1, x1, i1, t1);
            }
            const double xk = row[comp_pk(comp) * A.st.st_d];
            const bool ok = ok01 && on_axis(T.axk, T.nk, xk);
            double v[Q];
            if (ok) {
                int ik, off[8];
                double tk, w[8];
                bracket(T.axk, T.nk, xk, ik, tk);
                cell3_corners(T.n1, T.nk, Q, t0, t1, tk, off, w);
                cell3_columns<Q, Q % 2 == 0>(T.cols + ((i0 * T.n1 + i1) * T.nk + ik) * Q, off, w, v);
            } else {
#pragma unroll
                for (int j = 0; j < Q; ++j) v[j] = qnan();
            }
            bool any = false;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                o[(int64_t)(c * Q + j) * R] = v[j];
                any |= v[j] != v[j];
            }
            if (any) {
                int32_t* __restrict__ nc = A.nan_count + (int64_t)(r / A.W) * CQ + c * Q;
#pragma unroll
                for (int j = 0; j < Q; ++j)
                    if (v[j] != v[j]) atomicAdd(nc + j, 1);
            }
        }
    }
}

__global__ void __launch_bounds__(BLOCK) k_derived_chain(const Args A) {
    switch (A.T.Q) {                            // wave-uniform
    case 1: derive<1>(A); break;
    case 2: derive<2>(A); break;
    case 3: derive<3>(A); break;
    case 4: derive<4>(A); break;
    case 5: derive<5>(A); break;
    case 6: derive<6>(A); break;
    case 7: derive<7>(A); break;
    default: derive<8>(A); break;
    }
}

// arguments checked, strides and the work split filled in; device = the checks only the kernel needs
int prepare(const char* who, bool device, const iso_derived_table* t, const double* chain, int layout, int64_t nsteps,
            int32_t n_ens, int32_t W, int32_t ndim, int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C,
            double* out, int32_t* nan_count, Args& A) {
    const ChainShape s{layout, nsteps, n_ens, W, ndim, ens_begin, n_ens_out, comps, C};
    const char* why = nullptr;
    if (!t || !t->cols || !t->ax0 || !t->ax1 || !t->axk) why = "null table pointer";
    else if (!chain || !out || !nan_count || !comps) why = "null pointer";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES, s))) {}
    else if (t->Q < 1 || t->Q > ISO_DERIVED_MAX_COLS) why = "Q must be 1 to 8 columns per call";
    else if (C < 1 || C > ISO_DERIVED_MAX_COMPS) why = "C must be 1 to 3 components";
    else if (t->n0 < 2 || t->n1 < 2 || t->nk < 2) why = "every axis needs at least 2 nodes";
    else if ((int64_t)t->n0 * t->n1 * t->nk * t->Q > INT32_MAX) why = "table too large (more than 2^31 - 1 entries)";
    else if ((why = chain_shape_error(CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (nsteps > INT32_MAX) why = "nsteps beyond 2^31 - 1";
    else if (ndim > 256) why = "more than 256 parameters";
    else if (device && t->Q % 2 == 0 && ((uintptr_t)t->cols & 15)) why = "cols must be 16-byte aligned for an even Q";
    else why = chain_shape_error(CHAIN_CHECK_COMPS, s);
    if (!why) {
        const int64_t R = (int64_t)n_ens_out * W, chunks = (R + BLOCK - 1) / BLOCK;
        if (nsteps * chunks > INT32_MAX) why = "too many samples in one call (split the ensemble range)";
        A.R = (int32_t)R;
        A.chunks = (int32_t)chunks;
        A.items = (int32_t)(nsteps * chunks);
    }
    if (why) return fail(ISO_DERIVED_ERR_INVALID, who, why);
    A.st = chain_strides(layout, (int64_t)n_ens * W, ndim);
    A.chain = chain;
    A.out = out;
    A.nan_count = nan_count;
    A.T = *t;
    A.row0 = (int64_t)ens_begin * W;
    A.W = W;
    A.C = C;
    A.nsteps = (int32_t)nsteps;
    for (int c = 0; c < MAXC; ++c) {
        A.comp[c] = 0;
        if (c >= C) continue;
        const bool fresh = c == 0 || comps[3 * c] != comps[3 * c - 3] || comps[3 * c + 1] != comps[3 * c - 2];
        A.comp[c] = pack_comp(comps[3 * c], comps[3 * c + 1], comps[3 * c + 2]) | (fresh ? FRESH01 : 0);
    }
    return 0;
}

}  // namespace

extern "C" {

const char* iso_derived_version(void) { return "isochrones_amd derived 1"; }

const char* iso_derived_last_error(void) { return g_err; }

int iso_derived_chain(const iso_derived_table* table, const double* chain, int layout, int64_t nsteps, int32_t n_ens,
                      int32_t W, int32_t ndim, int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C,
                      double* out, int32_t* nan_count, void* stream) {
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_derived_chain", true, table, chain, layout, nsteps, n_ens, W, ndim, ens_begin, n_ens_out,
                           comps, C, out, nan_count, A);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(nan_count, 0, sizeof(int32_t) * (size_t)n_ens_out * C * table->Q, st);
    if (e != hipSuccess) return fail(ISO_DERIVED_ERR_HIP, hipGetErrorString(e));
    const int blocks = A.items < MAX_BLOCKS ? A.items : MAX_BLOCKS;
    hipLaunchKernelGGL(k_derived_chain, dim3((unsigned)blocks), dim3(BLOCK), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_DERIVED_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_derived_chain_host(const iso_derived_table* table, const double* chain, int layout, int64_t nsteps,
                           int32_t n_ens, int32_t W, int32_t ndim, int32_t ens_begin, int32_t n_ens_out,
                           const int32_t* comps, int32_t C, double* out, int32_t* nan_count, void* stream) {
    (void)stream;
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_derived_chain_host", false, table, chain, layout, nsteps, n_ens, W, ndim, ens_begin,
                           n_ens_out, comps, C, out, nan_count, A);
    if (rc) return rc;
    const iso_derived_table& T = A.T;
    const int Q = T.Q, CQ = C * Q, R = A.R;
    memset(nan_count, 0, sizeof(int32_t) * (size_t)n_ens_out * CQ);
    for (int64_t t = 0; t < nsteps; ++t)
        for (int r = 0; r < R; ++r) {
            const double* row = chain + t * A.st.st_t + (A.row0 + r) * A.st.st_w;
            for (int c = 0; c < C; ++c) {
                const int comp = A.comp[c];
                const double x0 = row[comp_p0(comp) * A.st.st_d], x1 = row[comp_p1(comp) * A.st.st_d],
                             xk = row[comp_pk(comp) * A.st.st_d];
                double v[ISO_DERIVED_MAX_COLS];
                cell3(T, Q, x0, x1, xk, v);
                for (int q = 0; q < Q; ++q) {
                    out[(t * CQ + c * Q + q) * R + r] = v[q];
                    if (v[q] != v[q]) ++nan_count[(int64_t)(r / W) * CQ + c * Q + q];
                }
            }
        }
    return 0;
}

}  // extern "C"
