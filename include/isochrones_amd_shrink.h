/* C ABI of libiso_shrink.so: the population-informed posterior of every star of a catalog under a population density that
 * is piecewise constant on a grid of bins (the histogram of include/isochrones_amd_binned.h), and the posterior probability
 * that the star lies in each cell of the grid, for gfx950.  It is the per-star counterpart of that header, as
 * include/isochrones_amd_reweight.h is of include/isochrones_amd_hier.h (Hogg, Myers & Bovy 2010, the "shrinkage" half).  It
 * reads the records and columns of isochrones_amd_hier.h as they stand and defines no record type.
 *
 * Notation.  It is isochrones_amd_binned.h's: S stars (ensembles), M = W * T samples each (sample m = t * W + w), Q value
 * columns passed as iso_hier_column in either chain layout, the interim records, the grid (n_axes, axis_col, n_bins, edges,
 * B cells, cell b = k0 * n_bins[1] + k1, the bin rule with the closed last bin), the frozen columns and their records,
 * and per sample the term c_m, "bad", "out" and the sample's cell: all that header's, word for word (the kernels and the
 * host entries compile one statement of them, csrc/common/binned_sample.h).  There is no `extra`: injections are no stars.
 * A, mx are the tables iso_binned_compress wrote, lnh [H][B] the log cell densities of H hyper rows, ell [H][n_ens] what
 * iso_binned_lnlike wrote for those rows: the weights' normaliser, ln Z_s(row h).
 *
 * The weights.  With the H rows taken as equally weighted draws of the hyper posterior, the weight of sample m of star s is
 * isochrones_amd_reweight.h's u = sum_h exp(r[h][s][m] - ell[h][s]); for a histogram r = c_m + lnh[h][cell(m)], so
 *     u[s][m] = exp(c_m - mx[s]) * G[s][cell(m)],      G[s][b] = sum_h exp(lnh[h][b] - (ell[h][s] - mx[s])):
 * the sum over the rows belongs to the (star, cell), not to the sample.  iso_shrink_cells takes it once per (star, cell)
 * from the tables alone; iso_shrink_weights then reads the chain once, with one exp per sample whatever H is.
 *
 * iso_shrink_cells.  Per (star s, cell b): row h is live if ell[h][s] is neither NaN nor +-inf and lnh[h][b] is neither NaN
 * nor -inf (+inf is not allowed; iso_shrink_cells_host refuses it).  a_h = lnh[h][b] - (ell[h][s] - mx[s]); g = the maximum
 * of a_h over the live rows;
 *     lnG[b][s] = g + ln(sum over the live h, ascending, from 0.0, of exp(a_h - g)),
 * -inf if no row is live or mx[s] is -inf (NaN if mx[s] is NaN).  Then pc_b = A[b][s] > 0 ? exp(ln A[b][s] + lnG[b][s]) : 0, tot = the sum of pc_b
 * over ascending b from 0.0, and
 *     cellp[b][s] = pc_b / tot,
 * the posterior probability that star s lies in cell b (mx cancels); NaN for every b if tot is not positive and finite (a
 * star with no weight left).  lnG and cellp are cell-major, [B][n_ens], as A is.  A call writes the stars
 * [ens_begin, ens_begin + n_ens_out) and leaves the rest alone; a star with mask[s] == 0 gets NaN in both.  cellp may be
 * NULL.  With ell the likelihood's own normaliser every exp(a_h) is at most M / A[b][s]: nothing overflows.
 *
 * iso_shrink_weights.  Per sample of an unmasked star,
 *     u[s][m] = exp((c_m - mx[s]) + lnG[cell(m)][s])
 * for a good in-grid sample with c_m > -inf, else 0.  Every term is at most H * M, isochrones_amd_reweight.h's argument for
 * subtracting no maximum.  weights is [n_ens_out][M], numbered from ens_begin (row s - ens_begin holds u[s][.], m = t * W
 * + w): the layout iso_reweight_summary reads.  Per star wsum[s] = sum_m u, ess[s] = (sum u)^2 / sum u^2 (0 when sum u is
 * 0), n_bad[s] and n_out[s] as iso_binned_compress counts them.  With ell from iso_binned_lnlike, wsum is M times the number
 * of live rows, to rounding.  A star with mask[s] == 0 gets wsum = ess = NaN and n_bad = n_out = 0; its samples are not read
 * and its weights are not written.  mx, lnG ([B][n_ens]), wsum, ess, n_bad, n_out and mask are [n_ens] in the call's
 * numbering; a call writes the stars of its range and leaves the rest alone.
 *
 * Summation order of the device kernels.  All sums start from 0.0.  k_shrink_cells gives a workgroup a block of 256
 * stars, a lane one star, and takes the cells a tile of ISO_SHRINK_CELL_TILE at a time: per tile one pass over the rows in
 * ascending order for the maxima (a maximum has no order), a second for the sums, each cell's an accumulator of its own, so
 * a (star, cell) result is the ascending sum of the definition whatever the star's block and the cell's place in a tile;
 * then the lane adds its star's pc_b over ascending b.  k_shrink_weights gives a workgroup of 256 lanes one star: lane i
 * takes the samples m = i, i + 256, ... in ascending order and adds u and u * u of its samples; the 256 partial sums are
 * combined by an xor butterfly inside each of the four wavefronts (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3
 * over the wavefronts: the reduction of k_reweight_weights.  No floating-point atomics; the source writes no fused
 * multiply-add and is compiled with -ffp-contract=off.  So a star's outputs are the same bits alone, in any batch, in any
 * sub-range of stars, from either layout, from a column and from a copy of it in another storage with a `first` offset,
 * and on a repeated call.  The _host entries state the same definitions with plain ascending loops; device and host agree
 * to rounding, not bit for bit (exp and log differ).
 *
 * The library works on pointers the caller owns.  The device entries allocate nothing, launch on the given stream and do
 * not synchronise.  Return codes: 0 ok, ISO_SHRINK_ERR_INVALID for a bad argument or a refused shape
 * (iso_shrink_last_error() says which: it is refused, not answered), ISO_SHRINK_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_SHRINK_H
#define ISOCHRONES_AMD_SHRINK_H

#include <stdint.h>

#include "isochrones_amd_hier.h"
#include "isochrones_amd_binned.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_SHRINK_ERR_INVALID (-1)
#define ISO_SHRINK_ERR_HIP (-2)

/* cells a lane of k_shrink_cells takes per pass over the rows; no part of the summation order */
#define ISO_SHRINK_CELL_TILE 2

const char* iso_shrink_version(void);
const char* iso_shrink_last_error(void);

/* A ([B][n_ens]), mx ([n_ens]), lnh ([H][B]), ell ([H][n_ens]), mask ([n_ens] int32, or NULL), lnG, cellp ([B][n_ens]; cellp
 * or NULL): device pointers.  1 <= B <= ISO_BINNED_MAX_CELLS, H >= 1. */
int iso_shrink_cells(const double* A, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin, int32_t n_ens_out,
                     const double* lnh, const double* ell, int32_t H, const int32_t* mask, double* lnG, double* cellp,
                     void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; stream is ignored); it sees lnh and
 * refuses a +inf in it */
int iso_shrink_cells_host(const double* A, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin, int32_t n_ens_out,
                          const double* lnh, const double* ell, int32_t H, const int32_t* mask, double* lnG, double* cellp,
                          void* stream);

/* columns ([Q] descriptors whose base pointers are device pointers), axis_col, n_bins ([n_axes]) and frozen_col ([n_frozen],
 * or NULL when n_frozen is 0): host arrays.  interim, frozen ([Q] records), edges, mx ([n_ens]), lnG ([B][n_ens]), mask
 * ([n_ens] int32, or NULL), weights ([n_ens_out][M]), wsum, ess ([n_ens]), n_bad, n_out ([n_ens] int32): device pointers. */
int iso_shrink_weights(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                       int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* frozen,
                       int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col,
                       const int32_t* n_bins, const double* edges, const double* mx, const double* lnG, const int32_t* mask,
                       double* weights, double* wsum, double* ess, int32_t* n_bad, int32_t* n_out, void* stream);

/* the same on host pointers; it sees the edges and the records and refuses edges that are not finite and strictly
 * increasing and records of another kind */
int iso_shrink_weights_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                            int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                            const iso_hier_record* frozen, int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes,
                            const int32_t* axis_col, const int32_t* n_bins, const double* edges, const double* mx,
                            const double* lnG, const int32_t* mask, double* weights, double* wsum, double* ess,
                            int32_t* n_bad, int32_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
