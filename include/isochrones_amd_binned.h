/* C ABI of libiso_binned.so: the hierarchical (population) likelihood of include/isochrones_amd_hier.h for a population
 * density that is piecewise constant on a grid of bins over one or two columns (a histogram: an age distribution, a
 * star-formation history, [Fe/H] bins per age bin), for gfx950.  It reads that header's records and columns as they stand
 * and defines no record type.
 *
 * For such a density the mean importance weight of a star is linear in the cell heights,
 *     (1/M) sum_m f(x_m; theta) / f0(x_m) = (1/M) sum_b h_b(theta) * A[s][b],   A[s][b] = sum over the star's samples in
 *     cell b of 1 / f0(x_m),
 * so the chain is read once per (catalog, edges) and compressed to B numbers per star (iso_binned_compress); every
 * likelihood evaluation after that, for any number of hyper rows, is a contraction of that table with the rows' log cell
 * densities (iso_binned_lnlike).
 *
 * Inputs.  The notation is isochrones_amd_hier.h's: S stars (ensembles), M = W * T samples each (sample m = t * W + w),
 * Q value columns (1 <= Q <= 4; M <= 2^31 - 257) passed as iso_hier_column, both chain layouts, the interim records interim[q].  The kinds
 * 1 .. 8 are that header's, with its arithmetic (csrc/common/family_lnf.h).
 *
 * Grid.  n_axes (1 or 2) of the Q columns are binned axes: axis a is column axis_col[a] and has n_bins[a] >= 1 bins on the
 * strictly increasing finite edges e[a][0 .. n_bins[a]], uniform or not; `edges` holds axis 0's n_bins[0] + 1 edges, then
 * axis 1's.  B = n_bins[0] (* n_bins[1]) <= ISO_BINNED_MAX_CELLS cells; cell b = k0 * n_bins[1] + k1 (b = k0 with one axis).
 * A value x falls in bin k if e[k] <= x < e[k + 1]; the last bin is closed above, so x == e[K] is in bin K - 1
 * (numpy.histogram's rule).  Every other column is frozen: it is listed in frozen_col[0 .. n_frozen) and has one population
 * record frozen[q] of the kinds 1 .. 8, the same for every hyper row (`frozen` is [Q], indexed by column; the entries of
 * the axes are not read).  Every column is an axis or frozen, and none is both.
 *
 * Per sample.  c_m = 0.0, then + (ln f_q - ln f0_q) for every frozen q, ascending, then - ln f0_q for every binned q,
 * ascending, then + extra[s * M + m] if extra is given (a log factor per sample: the detection probability of an
 * injection).  A frozen population term that is NaN counts as -inf.  A sample is bad, counted once in n_bad[s], if a used
 * column is NaN, an interim term is -inf or NaN, or extra is NaN or positive.  A good sample with a binned value outside
 * [e[0], e[K]] on an axis is out: it is counted once in n_out[s] and weighs 0.  M in every mean stays W * T.
 *
 * Compression.  mx[s] = max of c_m over the good in-grid samples with c_m > -inf, -inf if there is none.  Over those samples
 * of cell b, in ascending m, each sum from 0.0:
 *     A[b][s] = sum exp(c_m - mx[s]),        A2[b][s] = sum exp(c_m - mx[s])^2.
 * All are 0 when mx is -inf.  A and A2 are cell-major, [B][n_ens], so that the contraction's lanes, which run along the
 * stars, read consecutive doubles; mx, n_bad, n_out and mask are [n_ens].  A call writes the stars
 * [ens_begin, ens_begin + n_ens_out) and leaves the rest alone.  A star with mask[s] == 0 gets A = A2 = 0, mx = NaN,
 * n_bad = n_out = 0, and its samples are not read.  There is one reference value mx per star, not one per cell: a cell
 * whose samples all lie more than some 700 nats below the star's heaviest sample underflows to 0.  That is deliberate (a
 * cell that light adds nothing to the star's mean weight unless every heavier cell has height 0).
 *
 * Contraction.  lnh is [H][B]: the log cell densities of every hyper row; -inf is a cell of height 0, a NaN counts as
 * -inf, +inf is not allowed (iso_binned_lnlike_host refuses it).  Per row hmx = max_b lnh and u_b = exp(lnh_b - hmx), 0
 * for a cell of height 0: the exps are taken once per row, not per star.  Per (row, star), over ascending b, each from 0.0:
 *     s1 = sum_b u_b * A[b][s],   s2 = sum_b (u_b * u_b) * A2[b][s],
 *     ell[h][s] = (mx[s] + hmx) + ln s1 - ln M,   ess[h][s] = s1 * s1 / s2.
 * If s1 is not > 0: ell = -inf, ess = 0.  A masked star has ell = ess = NaN.
 *
 * Rescue.  hmx belongs to the row, so a star whose table lies only in cells far below the row's top has products
 * u_b * A[b][s] that leave float64's range while its answer is well inside it: from 372 nats below the top u_b * u_b is 0
 * (ess = 0 / 0), from 708 u_b is subnormal, from 745 it is 0 (ell = -inf).  So a (row, star) whose s1 above is below
 * ISO_BINNED_RESCUE_BELOW = 2^-400 (0 included) is taken again with the star's own reference height,
 *     ref = max{lnh_b : A[b][s] > 0 and lnh_b > -inf},   u'_b = exp(lnh_b - ref) over those cells,
 *     s1 = sum_b u'_b * A[b][s],   s2 = sum_b (u'_b * u'_b) * A2[b][s]   (ascending b, each from 0.0),
 *     ell[h][s] = (mx[s] + ref) + ln s1 - ln M,   ess[h][s] = s1 * s1 / s2;
 * without such a cell ell = -inf and ess = 0 as before.  The largest term of the new s1 is A of the reference cell itself,
 * so ell and ess are those of exact arithmetic wherever the star has weight under the row.  The threshold: at s1 >= 2^-400
 * every term the ordinary sums lose is harmless.  A term of s1 with a subnormal u_b is off by at most 2^-1074 * A[b][s] <=
 * 2^-1043 (A <= M < 2^31), 2^-643 of s1.  A term of s2 whose u_b * u_b is subnormal or 0 is off by at most 2^-1022 *
 * A2[b][s] <= 2^-991, while s2 >= s1 * s1 / M >= 2^-831 (Cauchy-Schwarz over the star's at most M samples): 2^-154 of s2
 * for all 64 cells together.  And s1 * s1 >= 2^-800 is a normal number.  The threshold is far above the point where any of
 * this matters and far below any s1 an ordinary row produces, so a pair that does not take the rescue keeps the bits of the
 * formula above.  What remains deliberate is the compression's single mx per star: a table entry that underflowed there is
 * 0 here too, and an A2 entry that is 0 under a positive A gives the ess it gave before.
 *
 * ell and ess are [H][n_ens].  L[h] and
 * min_ess[h] are isochrones_amd_hier.h's, over the unmasked stars of ell and ess as they stand after the call (0 and +inf
 * when there is none; both or neither).  M is an argument (int64), so that a call on the table of an injection set passes
 * the number of injections.
 *
 * Summation order of the device kernels.  k_binned_compress gives a workgroup of 256 lanes one star.  Lane i evaluates the
 * samples m = i, i + 256, ...; the star's mx is an xor butterfly of the lanes' maxima inside each wavefront and a maximum
 * over the four wavefronts (a maximum has no order).  A second pass takes the same samples a tile of 256 at a time: every
 * lane stages (cell or -1, exp(c - mx)) in LDS, then lane b < B, the one owner of cell b, walks the tile's 256 entries in
 * ascending order and adds the matching ones to its two sums.  That is the ascending-m order of the definition whatever the
 * layout, the batch and the range of stars; no floating-point atomics, no per-lane histograms.  k_binned_rows gives a
 * workgroup a tile of ISO_BINNED_ROW_TILE consecutive rows and a block of 256 stars, a lane one star: it adds over
 * ascending b with a separate multiply and add; a row's arithmetic does not depend on its place in the tile, nor a star's
 * on its block.  The lane that owns a star takes a rescued pair again after the tile's ordinary results, from the tables and
 * the row in global memory, by the function the host entry calls: the same ascending order, and the same identities.  k_binned_total is k_hier_total: lane i adds the unmasked stars s = i, i + 256, ... in ascending order,
 * then the xor butterfly inside each wavefront (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3.  The source writes
 * no fused multiply-add and is compiled with -ffp-contract=off.  So a star's A, A2 and mx are the same bits alone, in any
 * batch, in any sub-range of stars, from either layout, from a column and from a copy of it in another storage with a
 * `first` offset, and on a repeated call; a (row, star) result is the same bits in any sub-range or tiling of the rows.  The
 * _host entries state the same definitions with plain ascending loops; device and host agree to rounding, not bit for
 * bit (exp and log differ).
 *
 * The library works on pointers the caller owns.  The device entries allocate nothing, launch on the given stream and do
 * not synchronise; the _host entries hold a star's M sample terms and a row's B heights in vectors of their own.  Return
 * codes: 0 ok, ISO_BINNED_ERR_INVALID for a bad argument or a refused shape (iso_binned_last_error() says which: it is
 * refused, not answered), ISO_BINNED_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_BINNED_H
#define ISOCHRONES_AMD_BINNED_H

#include <stdint.h>

#include "isochrones_amd_hier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_BINNED_ERR_INVALID (-1)
#define ISO_BINNED_ERR_HIP (-2)

#define ISO_BINNED_MAX_CELLS 64
#define ISO_BINNED_MAX_AXES 2
/* hyper rows a workgroup of k_binned_rows takes; no part of the summation order */
#define ISO_BINNED_ROW_TILE 8
/* a (row, star) whose s1 is below this, 0 included, is taken again with the star's own reference height (Contraction) */
#define ISO_BINNED_RESCUE_BELOW 0x1p-400

const char* iso_binned_version(void);
const char* iso_binned_last_error(void);

/* columns ([Q] descriptors whose base pointers are device pointers), axis_col, n_bins ([n_axes]) and frozen_col ([n_frozen],
 * or NULL when n_frozen is 0): host arrays.  interim, frozen ([Q] records), edges, extra ([n_ens * W * nsteps], or NULL),
 * mask ([n_ens] int32, or NULL), A, A2 ([B][n_ens]), mx ([n_ens]), n_bad, n_out ([n_ens] int32): device pointers. */
int iso_binned_compress(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                        int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* frozen,
                        int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col,
                        const int32_t* n_bins, const double* edges, const double* extra, const int32_t* mask, double* A,
                        double* A2, double* mx, int32_t* n_bad, int32_t* n_out, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; stream is ignored); it sees the
 * edges and the records and refuses edges that are not finite and strictly increasing and records of another kind */
int iso_binned_compress_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                             int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                             const iso_hier_record* frozen, int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes,
                             const int32_t* axis_col, const int32_t* n_bins, const double* edges, const double* extra,
                             const int32_t* mask, double* A, double* A2, double* mx, int32_t* n_bad, int32_t* n_out,
                             void* stream);

/* A, A2 ([B][n_ens]), mx ([n_ens]), lnh ([H][B]), mask ([n_ens] int32, or NULL), ell, ess ([H][n_ens]), L, min_ess ([H], or
 * both NULL): device pointers.  A sub-range of the rows is a call with lnh, ell and ess advanced to its first row. */
int iso_binned_lnlike(const double* A, const double* A2, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin,
                      int32_t n_ens_out, int64_t M, const double* lnh, int32_t H, const int32_t* mask, double* ell,
                      double* ess, double* L, double* min_ess, void* stream);

/* the same on host pointers */
int iso_binned_lnlike_host(const double* A, const double* A2, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin,
                           int32_t n_ens_out, int64_t M, const double* lnh, int32_t H, const int32_t* mask, double* ell,
                           double* ess, double* L, double* min_ess, void* stream);

#ifdef __cplusplus
}
#endif

#endif
