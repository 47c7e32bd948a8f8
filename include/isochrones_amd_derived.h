/* C ABI of libiso_derived.so: model-grid columns (mass, radius, Teff, logg, age ...) interpolated at every sample of a
 * stored ensemble-sampler chain, for gfx950.  The result is a chain of its own, in the sampler's storage layout, so the
 * quantile entry point of libiso_hip.so (iso_chain_quantiles_layout) summarises it where it lies.
 *
 * Table.  cols[n0][n1][nk][Q]: Q selected columns of a 3-D model grid, the Q values of one node adjacent, NaN-padded as
 * the grid is; 1 <= Q <= ISO_DERIVED_MAX_COLS.  ax0, ax1, axk: the axes, strictly increasing, not necessarily uniform,
 * n0, n1, nk >= 2 entries.  n0 * n1 * nk * Q <= 2^31 - 1.
 *
 * Chain.  nsteps x (n_ens * W) rows x ndim parameters, float64, in either layout of isochrones_amd.h:
 *   ISO_DERIVED_PARAM_MAJOR  chain[(t * ndim + d) * (n_ens * W) + row]     (the sampler's storage, read in place)
 *   ISO_DERIVED_ROW_MAJOR    chain[(t * (n_ens * W) + row) * ndim + d]
 * with row = ensemble * W + walker.  The call works on the ensembles [ens_begin, ens_begin + n_ens_out); R is
 * n_ens_out * W and r = row - ens_begin * W.
 *
 * Components.  comps[C][3] (host memory), 1 <= C <= ISO_DERIVED_MAX_COMPS: component c reads its coordinates on
 * (ax0, ax1, axk) from the chain parameters (comps[c][0], comps[c][1], comps[c][2]), each in [0, ndim).  A track grid
 * with axes (feh, mass, eep) and parameters (mass, eep, feh, ...) is {2, 0, 1}; an isochrone grid with axes (age, feh,
 * eep) and parameters (eep, age, feh, ...) is {1, 2, 0}; a binary on it, (eep_0, eep_1, age, feh, ...), is {2, 3, 0} and
 * {2, 3, 1}.
 *
 * One sample and component: x = (x0, x1, xk) -> Q values, trilinear, with the interpolator's own rules (the ones
 * include/isochrones_amd_solve.h states):
 *   - a NaN coordinate, or one below the first or above the last node of its axis, gives NaN for all Q columns;
 *   - otherwise, per axis a with n nodes: i_a = the largest index with ax[i_a] <= x_a, but at most n - 2 (a query on a
 *     node takes the cell above it; a query on the last node takes the cell below), t_a = (x_a - ax[i_a]) /
 *     (ax[i_a + 1] - ax[i_a]) (0 on a node, 1 on the last node), u_a = 1 - t_a;
 *   - the corner (b0, b1, bk), b in {0, 1}, is the node (i_0 + b0, i_1 + b1, i_k + bk) and has the weight
 *         w = (f_0 * f_1) * f_k,       f_a = t_a where b_a = 1, u_a where b_a = 0;
 *   - value[q] = 0.0, then value[q] = value[q] + cols[corner][q] * w for the eight corners in the order
 *     (b0, b1, bk) = 000, 001, 010, 011, 100, 101, 110, 111 (bk fastest).  Every corner is multiplied by its weight even
 *     when that weight is zero, so a NaN neighbour gives NaN.
 * Every operation above is one IEEE float64 operation, rounded on its own, in the order written; there is no fused
 * multiply-add anywhere (the library is built with -ffp-contract=off and writes no fma).  A sample's values therefore
 * do not depend on the batch it is in, on the ensemble range or on the chain layout, and this is the arithmetic of the
 * interpolator (oracle/iso_oracle.c, orc_interp_value) term by term.  The kernel, the host entry and the libraries of
 * isochrones_amd_predict.h and isochrones_amd_population.h compile one statement of this cell (the internal
 * csrc/common/grid_interp.h), so one table and one point give the same bits in all of them.
 *
 * Output.  out[(t * (C * Q) + c * Q + q) * R + r]: parameter-major storage [nsteps][C * Q][R] of n_ens_out ensembles,
 * which iso_chain_quantiles_layout takes with n_params = C * Q.  nan_count[e * (C * Q) + c * Q + q], e < n_ens_out
 * (int32): cleared by the call on the stream, then the number of NaN values written for that ensemble and column over
 * all steps and walkers.
 *
 * The library allocates nothing, starts no resident waves and works on device pointers the caller owns (comps and the
 * table struct itself are host memory, read before the call returns).  iso_derived_chain launches on the given stream and
 * does not synchronise.  iso_derived_chain_host does the same on host pointers in plain C++ with ascending loops and
 * touches no device.  Return codes: 0 ok, ISO_DERIVED_ERR_INVALID for a bad argument (iso_derived_last_error() says
 * which), ISO_DERIVED_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_DERIVED_H
#define ISOCHRONES_AMD_DERIVED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_DERIVED_ERR_INVALID (-1)
#define ISO_DERIVED_ERR_HIP (-2)

/* chain layouts: the values of ISO_CHAIN_ROW_MAJOR / ISO_CHAIN_PARAM_MAJOR of isochrones_amd.h */
#define ISO_DERIVED_ROW_MAJOR 0
#define ISO_DERIVED_PARAM_MAJOR 1

#define ISO_DERIVED_MAX_COLS 8
#define ISO_DERIVED_MAX_COMPS 3

/* One packed table; every pointer is a device pointer the caller owns (a host pointer for iso_derived_chain_host).
 * For an even Q, iso_derived_chain wants cols 16-byte aligned (a node's columns are read two at a time). */
typedef struct iso_derived_table {
    const double* cols;
    const double* ax0;
    const double* ax1;
    const double* axk;
    int32_t n0, n1, nk, Q;
} iso_derived_table;

const char* iso_derived_version(void);
const char* iso_derived_last_error(void);

/* chain, out (nsteps * C * Q * n_ens_out * W doubles), nan_count (n_ens_out * C * Q int32): device pointers */
int iso_derived_chain(const iso_derived_table* table, const double* chain, int layout, int64_t nsteps, int32_t n_ens,
                      int32_t W, int32_t ndim, int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C,
                      double* out, int32_t* nan_count, void* stream);

/* the same on host pointers, in plain C++ (no device is touched; stream is ignored) */
int iso_derived_chain_host(const iso_derived_table* table, const double* chain, int layout, int64_t nsteps,
                           int32_t n_ens, int32_t W, int32_t ndim, int32_t ens_begin, int32_t n_ens_out,
                           const int32_t* comps, int32_t C, double* out, int32_t* nan_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif
