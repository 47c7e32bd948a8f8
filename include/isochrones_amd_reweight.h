/* C ABI of libiso_reweight.so: the population-informed posterior of every star of a catalog from its stored chain, by
 * importance reweighting of the star's samples from the prior the fit used to a fitted population (Hogg, Myers & Bovy
 * 2010, the "shrinkage" half), for gfx950.  It is the per-star counterpart of include/isochrones_amd_hier.h and reads that
 * header's records and columns as they stand.
 *
 * Inputs.  The notation is isochrones_amd_hier.h's: S stars (ensembles), M = W * T samples each (sample m = t * W + w),
 * Q model columns (1 <= Q <= 4), H hyper rows (H >= 1), the interim records interim[q] and the population records
 * rows[h * Q + q].  The per-sample log ratio r[h][s][m], the bad-sample rule, the mask, and the addressing of a column
 * (iso_hier_column, `first`, both layouts) are that header's, word for word.  ln_norm is [H][n_ens]: the per-(row, star)
 * normaliser of the weights; callers pass ell of iso_hier_lnlike.
 *
 * Weights.  u[s][m] = (((0.0 + t_0) + t_1) + ...) + t_{H-1}, t_h = exp(r[h][s][m] - ln_norm[h][s]), summed over h in
 * ascending order whatever the tiling of the rows.  A row whose ln_norm is -inf or NaN contributes 0.  A bad sample has
 * u = 0.  With ln_norm = ell every t_h <= M: no maximum is subtracted, and an underflow to 0 is the right answer.  u is the
 * posterior weight of sample m when the H rows are equally weighted draws of the hyper posterior:
 *     p(x_s | all data)  ~  (1 / H) sum_h f(x; Lambda_h) / (f0(x) Z_s(Lambda_h)),       Z_s = exp(ell[h][s]).
 * The selection term (isochrones_amd_select.h) does not enter: a star that is in the catalog was detected whatever Lambda
 * is, so alpha(Lambda) weighs the rows of the hyper posterior (which the caller's rows already are draws of), not the
 * samples of a star.
 *
 * Per star.  wsum[s] = sum_m u, ess[s] = (sum u)^2 / sum u^2 (0 when sum u = 0), n_bad[s].  A star with mask[s] == 0 has
 * wsum = ess = NaN and n_bad = 0; its samples are not read, its weights are not written, and its value summaries below
 * are NaN with n_nan = 0.  mask == NULL masks nothing.
 *
 * Per (star, value column v).  There are V value columns, 1 <= V <= 8, each an iso_hier_column of its own (a chain
 * parameter or a derived column, a model column or not); y is the column's samples.  A sample whose y is NaN has weight 0
 * for that column and is counted in n_nan[s][v]; over the rest, with u as above,
 *     tot = sum u,     mean = (sum u * y) / tot,     sd = sqrt((sum u * ((y - mean) * (y - mean))) / tot),
 * and for each of K probabilities 0 < p_k < 1, 1 <= K <= 8, quant[s][v][k] is the inverted weighted distribution function:
 * the smallest sample value y* with C(y*) >= p_k * tot, C(y*) = sum of u over the samples with y <= y*.  Samples of weight 0
 * take no part (they change no C).  -0 counts as +0 and is returned as +0.  If rounding leaves every C below p_k * tot
 * (p_k within rounding of 1), y* is the largest sample of positive weight.  With equal weights this is
 * numpy.percentile(y, 100 p, method="inverted_cdf").  When tot = 0 (or is not finite and positive) mean, sd and quant
 * are NaN.
 *
 * Addressing.  wsum, ess, n_bad are [n_ens]; mean, sd, n_nan [n_ens][V]; quant [n_ens][V][K]; ln_norm [H][n_ens]; mask
 * [n_ens]: all in the call's numbering.  A call writes the stars [ens_begin, ens_begin + n_ens_out) and leaves the rest
 * alone.  weights is [n_ens_out][M], numbered from ens_begin: row s - ens_begin holds u[s][.].  It is required: it is an
 * output and the second kernel's input (and, between row tiles, the first kernel's accumulator).
 *
 * Summation order of the device kernels.  It depends on W, T and H only.  All sums start from 0.0.
 *   k_reweight_weights gives a workgroup of 256 lanes one star.  Lane i takes the samples m = i, i + 256, ... in ascending
 *   order; per sample the rows run innermost, ascending.  Rows are staged ISO_REWEIGHT_ROW_TILE at a time; between tiles u
 *   waits in weights and is read back by the lane that wrote it, so u is the ascending sum of the definition for any H.
 *   Each lane adds u and u * u of its samples in ascending order; the 256 partial sums are combined by an xor butterfly
 *   inside each of the four wavefronts (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3 over the wavefronts.
 *   k_reweight_summary gives a workgroup one (star, value column) and reads (y, u) from memory in every pass.  Pass one:
 *   tot, sum u * y and n_nan; pass two: sum u * ((y - mean) * (y - mean)); both lane-strided and combined as above (a NaN
 *   sample adds +0.0).  Then, per probability in the order given, y* by a weighted radix select on the order-preserving
 *   64-bit key of y + 0.0 (key = bits ^ sign bit for y >= 0, ~bits for y < 0): 16 passes of 4 bits from the top.  A pass
 *   keeps `below` (0.0 at first) and the key's digits found so far; each lane adds u of its samples that match those digits
 *   into 16 bins by the next digit, ascending m; each bin is combined as above to B[0..15]; then with c = below, for d = 0
 *   .. 15 in turn c' = c + B[d]; the digit is the first d with B[d] > 0 and c' >= p_k * tot (the last d with B[d] > 0 if
 *   there is none), below becomes the c in front of it, and c = c' goes on.  After 16 passes the digits are y*'s key.
 * No floating-point atomics; the source writes no fused multiply-add and is compiled with -ffp-contract=off.  So a star's
 * outputs are the same bits alone, in any batch, in any sub-range of stars, from either layout, from columns at another
 * address and on a repeated call, and a value column's alone or among eight.  iso_reweight_stars_host states the same
 * definition with plain ascending loops and a stable sort; the two agree to rounding, and in y* exactly unless some C lies
 * within rounding of p_k * tot.
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_reweight_stars launches on the given stream
 * and does not synchronise.  Return codes: 0 ok, ISO_REWEIGHT_ERR_INVALID for a bad argument or a refused shape
 * (iso_reweight_last_error() says which: it is refused, not answered), ISO_REWEIGHT_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_REWEIGHT_H
#define ISOCHRONES_AMD_REWEIGHT_H

#include <stdint.h>

#include "isochrones_amd_hier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_REWEIGHT_ERR_INVALID (-1)
#define ISO_REWEIGHT_ERR_HIP (-2)

#define ISO_REWEIGHT_MAX_VALUES 8
#define ISO_REWEIGHT_MAX_PROBS 8
/* hyper rows staged at a time by k_reweight_weights; no part of the summation order */
#define ISO_REWEIGHT_ROW_TILE 64

const char* iso_reweight_version(void);
const char* iso_reweight_last_error(void);

/* columns ([Q]), values ([V]): host arrays of descriptors whose base pointers are device pointers.  probs ([K]): host.
 * interim ([Q]), rows ([H][Q]), ln_norm ([H][n_ens]), mask ([n_ens] int32, or NULL), weights ([n_ens_out][M]), wsum, ess
 * ([n_ens]), n_bad ([n_ens] int32), mean, sd ([n_ens][V]), quant ([n_ens][V][K]), n_nan ([n_ens][V] int32): device
 * pointers. */
int iso_reweight_stars(const iso_hier_column* columns, int32_t Q, const iso_hier_column* values, int32_t V, int layout,
                       int64_t nsteps, int32_t n_ens, int32_t W, int32_t ens_begin, int32_t n_ens_out,
                       const iso_hier_record* interim, const iso_hier_record* rows, int32_t H, const double* ln_norm,
                       const int32_t* mask, const double* probs, int32_t K, double* weights, double* wsum, double* ess,
                       int32_t* n_bad, double* mean, double* sd, double* quant, int32_t* n_nan, void* stream);

/* the same on host pointers, in plain C++ with ascending loops and a stable sort (no device is touched; stream is ignored) */
int iso_reweight_stars_host(const iso_hier_column* columns, int32_t Q, const iso_hier_column* values, int32_t V, int layout,
                            int64_t nsteps, int32_t n_ens, int32_t W, int32_t ens_begin, int32_t n_ens_out,
                            const iso_hier_record* interim, const iso_hier_record* rows, int32_t H, const double* ln_norm,
                            const int32_t* mask, const double* probs, int32_t K, double* weights, double* wsum,
                            double* ess, int32_t* n_bad, double* mean, double* sd, double* quant, int32_t* n_nan,
                            void* stream);

/* The summaries alone, of weights the caller supplies (iso_shrink_weights's, for a binned population density): the
 * "Per (star, value column)" paragraph above with u = weights, by k_reweight_summary as iso_reweight_stars launches it, so
 * fed the weights that call wrote it returns that call's mean, sd, quant and n_nan bit for bit.  values ([V]): a host array of
 * descriptors whose base pointers are device pointers.  probs ([K]): host.  mask ([n_ens] int32, or NULL), weights
 * ([n_ens_out][M], numbered from ens_begin: an input), mean, sd ([n_ens][V]), quant ([n_ens][V][K]), n_nan ([n_ens][V]
 * int32): device pointers.  A masked star's weights are not read. */
int iso_reweight_summary(const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                         int32_t ens_begin, int32_t n_ens_out, const int32_t* mask, const double* probs, int32_t K,
                         const double* weights, double* mean, double* sd, double* quant, int32_t* n_nan, void* stream);

/* the same on host pointers, by iso_reweight_stars_host's loops */
int iso_reweight_summary_host(const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                              int32_t ens_begin, int32_t n_ens_out, const int32_t* mask, const double* probs, int32_t K,
                              const double* weights, double* mean, double* sd, double* quant, int32_t* n_nan,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif
