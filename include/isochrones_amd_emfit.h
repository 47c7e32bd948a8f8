/* C ABI of libiso_emfit.so: a batch of weighted EM fits of the cell masses of a population density that is piecewise
 * constant on a grid of bins (the histogram of include/isochrones_amd_binned.h), and the star weights of a bootstrap, for
 * gfx950.  Every replicate of the batch is one fit on the same per-star table A that iso_binned_compress wrote, under its
 * own weight per star; the whole iteration runs on the device, one workgroup per replicate.  The chain is not read.
 *
 * Notation.  A [B][n_ens], cell-major, non-negative: the table of n_ens stars over B cells (1 <= B <=
 * ISO_BINNED_MAX_CELLS).  scale [B], finite and >= 0: what turns a cell's mass into its height in A's units (1 / cell
 * volume without selection, 1 / a_b with an injection set's one-star table a); a zero closes the cell.  w [R][n_ens], float64
 * star weights of R replicates, finite and >= 0, or NULL: every weight is 1.  mask [n_ens] int32 or NULL, zero for a star
 * to leave out.  g0: the start masses, [R] rows g0_stride doubles apart (g0_stride >= B), or one row [B] shared by all
 * replicates when g0_stride == 0; finite, >= 0, every row with a sum above 0.  max_iter >= 0; tol, not a NaN.
 *
 * Definition.  Per replicate r, with g = its row of g0 and t = 0, 1, ...:
 *   1. v_b = g_b * scale_b.
 *   2. Per star, over ascending b from 0.0 with a separate multiply and add: s1 = sum_b v_b * A[b][s].
 *      Rescue: v is not normalised, and a fit drives the mass of an unsupported cell geometrically to 0, so a star whose
 *      table lies only in such cells has an s1 that is tiny, subnormal or 0 while w / s1 is beyond float64.  A star that is
 *      unmasked with w > 0 and whose s1 is below ISO_BINNED_RESCUE_BELOW = 2^-400 (0 included; isochrones_amd_binned.h has
 *      the argument for the threshold) takes its products again as mantissas and powers of two: with frexp's g_b = mg 2^eg,
 *      scale_b = ms 2^es and A[b][s] = ma 2^ea, the product is ((mg * ms) * ma) * 2^(eg + es + ea); emax is the largest of
 *      these exponents over the cells where both mg * ms and A[b][s] are above 0, and
 *          v_b * A[b][s] := ldexp((mg * ms) * ma, eg + es + ea - emax),   s1 their sum over ascending b from 0.0,
 *          log(s1) := log(s1) + emax * ln 2   (ln 2 its nearest float64),
 *      so that w / s1 and every product of step 4 are those of the star scaled by 2^-emax, which cancels.  No factor is
 *      rounded before it is scaled: a subnormal g_b enters with all its bits.  Without such a cell s1 = 0.
 *   3. Star s is live if it is unmasked, w[r][s] > 0 and s1 > 0.  Anything else, a NaN included, adds nothing.
 *   4. Over the live stars, each sum from 0.0:
 *        Q_t    = sum_s w * log(s1)
 *        N_b    = sum_s (v_b * A[b][s]) * (w / s1)
 *        W      = sum_s w
 *        n_live = their number.
 *   5. In this order: if n_live == 0, stop with status ISO_EMFIT_EMPTY and g as it is; else if t >= 1 and
 *      Q_t - Q_{t-1} < tol, stop with ISO_EMFIT_CONVERGED; else if t == max_iter, stop with ISO_EMFIT_MAX_ITER; else
 *      g_b = N_b / T with T = sum_b N_b over ascending b from 0.0, and go on with t + 1.
 * Outputs: g [R][B] the masses Q was evaluated at, objective [R] that Q, n_iter [R] the steps applied (the last t),
 * status [R], n_live [R] and wsum [R] (W) of the last evaluation.  tol = -INFINITY disables the second stop: exactly
 * max_iter steps are taken unless a replicate is empty.  Q_t is the weighted log likelihood up to a constant, and a step
 * never lowers it but for rounding.  A sub-range of the replicates is a call with w, g0 (unless shared), and every output
 * advanced to its first replicate.  g0 may be g itself (g0_stride == B): a replicate reads its row before it writes it.
 *
 * Summation order of k_emfit_run.  One workgroup of ISO_EMFIT_LANES = 256 lanes per replicate; the loop over t runs inside
 * the kernel.  Lane l owns the stars s = l (mod 256) and takes them in ascending order into sums of its own that start at
 * 0.0 with every t: Q, W, the live count and one sum per cell.  A live star's s1 is taken in a first pass over ascending
 * b; a second pass over ascending b reads the star's column again and adds (v_b * A[b][s]) * (w / s1) to the cell's sum,
 * w / s1 rounded once; a rescued star goes through the same two passes with its scaled products (a cell's mg * ms and
 * eg + es are kept in LDS next to v, taken once per step).  The 256 lane sums of each output are combined within each wavefront of 64 lanes by xor butterflies
 * of distances 32 .. 1 (wave_sum of common/wave_reduce.h), and the four wavefront totals are added in ascending wavefront
 * order from the first.  T and g_b = N_b / T are the definition's.  No floating-point atomics; the source writes no fused
 * multiply-add and is compiled with -ffp-contract=off.  So a replicate's outputs are the same bits alone, in any batch,
 * at any replicate offset and on every call.  iso_emfit_run_host states the definition with plain ascending loops over
 * all stars; device and host agree to rounding, not bit for bit (log differs, and the host has no lanes).
 *
 * Launches.  A kernel applies at most `steps` steps: the largest number with n_ens * B * steps <= ISO_EMFIT_LAUNCH_WORK, at
 * least 1, or steps_per_launch where that is above 0.  iso_emfit_run enqueues max(1, ceil(max_iter / steps)) launches on
 * the caller's stream.  The state travels between them in the outputs themselves: g, objective as Q_{t-1}, n_iter as t,
 * status as ISO_EMFIT_RUNNING; a replicate that has stopped returns at once.  A chain of launches gives the bits of one
 * launch, whatever `steps`.
 *
 * Weights.  iso_emfit_weights fills out [R][n_ens]: for (replicate r, star s) the words of Philox4x32-10
 * (common/philox.h) at the counter (s, first_replicate + r, 0, ISO_EMFIT_PHILOX_TAG) under the key (seed's low word,
 * seed's high word), u = philox_uniform53(word 0, word 1), 0 < u < 1.  ISO_EMFIT_POISSON: the Poisson(1) count by the
 * inverse distribution function, the number of k with u >= c_k, c_k = sum_{j <= k} e^-1 / j! (ISO_EMFIT_POISSON_CDF: the
 * eighteen c_k below 1 as hexadecimal literals, so host and device compare against the same doubles and the counts are
 * equal integers).  ISO_EMFIT_EXP: -log(u), the weights of the Bayesian bootstrap; their Dirichlet normalisation cancels
 * in g.  A weight depends on (seed, first_replicate + r, s) alone.  One lane per (replicate, star), consecutive lanes
 * consecutive stars.
 *
 * The library works on pointers the caller owns.  The device entries allocate nothing, launch on the given stream and do
 * not synchronise; they cannot see their inputs' values and check the shapes only.  The host entries see them and refuse
 * a negative or non-finite scale, w or g0 and a g0 row without a sum above 0.  Return codes: 0 ok, ISO_EMFIT_ERR_INVALID
 * for a bad argument or a refused shape or value (iso_emfit_last_error() says which: it is refused, not answered),
 * ISO_EMFIT_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_EMFIT_H
#define ISOCHRONES_AMD_EMFIT_H

#include <stdint.h>

#include "isochrones_amd_binned.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_EMFIT_ERR_INVALID (-1)
#define ISO_EMFIT_ERR_HIP (-2)

/* status of a replicate */
#define ISO_EMFIT_RUNNING 0
#define ISO_EMFIT_CONVERGED 1
#define ISO_EMFIT_MAX_ITER 2
#define ISO_EMFIT_EMPTY 3

/* kinds of weights */
#define ISO_EMFIT_POISSON 0
#define ISO_EMFIT_EXP 1

/* lanes of a replicate's workgroup; part of the summation order */
#define ISO_EMFIT_LANES 256
/* (star, cell, step) products a launch takes at most; no part of the summation order */
#define ISO_EMFIT_LAUNCH_WORK 2147483648
/* the last counter word of the weights' Philox calls */
#define ISO_EMFIT_PHILOX_TAG 0xB7
/* the cumulative Poisson(1) probabilities below 1, c_0 .. c_17 */
#define ISO_EMFIT_POISSON_TERMS 18
#define ISO_EMFIT_POISSON_CDF                                                                                       \
    0x1.78b56362cef38p-2, 0x1.78b56362cef38p-1, 0x1.d6e2bc3b82b06p-1, 0x1.f6472f2e6944ap-1, 0x1.fe204beb22e9cp-1,  \
    0x1.ffb21e77480acp-1, 0x1.fff516e3f8e59p-1, 0x1.fffea81812296p-1, 0x1.ffffda3e9551ep-1, 0x1.fffffc42dcc83p-1,  \
    0x1.ffffffa9b0ba6p-1, 0x1.fffffff8db44cp-1, 0x1.ffffffff7425ap-1, 0x1.fffffffff60f9p-1, 0x1.ffffffffff572p-1,  \
    0x1.fffffffffff58p-1, 0x1.ffffffffffff6p-1, 0x1.fffffffffffffp-1

const char* iso_emfit_version(void);
const char* iso_emfit_last_error(void);

/* A ([B][n_ens]), scale ([B]), w ([R][n_ens], or NULL), mask ([n_ens] int32, or NULL), g0, g ([R][B]), objective ([R]),
 * n_iter, status, n_live ([R] int32), wsum ([R]): device pointers.  1 <= B <= ISO_BINNED_MAX_CELLS, n_ens >= 1, R >= 1,
 * g0_stride == 0 or >= B, max_iter >= 0, tol not a NaN, steps_per_launch > 0 or 0 for the library's choice. */
int iso_emfit_run(const double* A, int32_t B, int32_t n_ens, const double* scale, const double* w, int32_t R,
                  const int32_t* mask, const double* g0, int32_t g0_stride, int32_t max_iter, double tol,
                  int32_t steps_per_launch, double* g, double* objective, int32_t* n_iter, int32_t* status,
                  int32_t* n_live, double* wsum, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; steps_per_launch and stream are
 * ignored); it sees scale, w and g0 and refuses what the text above says */
int iso_emfit_run_host(const double* A, int32_t B, int32_t n_ens, const double* scale, const double* w, int32_t R,
                       const int32_t* mask, const double* g0, int32_t g0_stride, int32_t max_iter, double tol,
                       int32_t steps_per_launch, double* g, double* objective, int32_t* n_iter, int32_t* status,
                       int32_t* n_live, double* wsum, void* stream);

/* out ([R][n_ens]): a device pointer.  kind: ISO_EMFIT_POISSON or ISO_EMFIT_EXP; first_replicate >= 0, R >= 1, n_ens >= 1,
 * first_replicate + R <= 2^31 - 1 */
int iso_emfit_weights(int32_t kind, uint64_t seed, int32_t first_replicate, int32_t R, int32_t n_ens, double* out,
                      void* stream);

/* the same on a host pointer (no device is touched; stream is ignored) */
int iso_emfit_weights_host(int32_t kind, uint64_t seed, int32_t first_replicate, int32_t R, int32_t n_ens, double* out,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif
