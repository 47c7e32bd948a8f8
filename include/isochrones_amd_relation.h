/* C ABI of libiso_relation.so: the hierarchical (population) likelihood of include/isochrones_amd_hier.h for a population
 * density in which one column's Gaussian follows another column linearly (an age-metallicity relation, AV against
 * distance, radius against mass), for gfx950.  It reads that header's records and columns as they stand and adds one
 * record kind.
 *
 * Inputs.  The notation is isochrones_amd_hier.h's: S stars (ensembles), M = W * T samples each (sample m = t * W + w),
 * Q value columns (1 <= Q <= 4), H hyper rows (H >= 1), the interim records interim[q] and the population records
 * rows[h * Q + q], a column passed as an iso_hier_column.  The kinds 1 .. 8 are that header's, with its arithmetic
 * (csrc/common/family_lnf.h).
 *
 * The linked kind.  A population record rows[h * Q + q] may have kind ISO_RELATION_LINGAUSS: column q is Gaussian about a
 * mean that is linear in the same sample's value of another column p, and renormalised on [lo, hi] for that mean:
 *   reserved = p, the parent column, 0 <= p < Q and p != q; lo and hi finite;
 *   p0 = intercept, p1 = sigma, p2 = -ln sqrt(2 pi) - ln sigma, p3 = 1 / sigma, p4 = slope, p5 = pivot.
 * With x the sample's value of column q and xp its value of column p:
 *   mu = p0 + p4 * (xp - p5);   z = (x - mu) * p3
 *   a = (lo - mu) * p3;  b = (hi - mu) * p3;  if a > 0: (a, b) = (-b, -a)        the mass in the lower tail: no 1 - 1
 *   mass = 0.5 * (erfc(-b * 0.7071067811865476) - erfc(-a * 0.7071067811865476))
 *   x < lo or x > hi: -inf;   mass not > 0 (a mean some 38 sigma outside the bounds, or NaN): -inf;
 *   otherwise (-(z * z) / 2 + p2) - log(mass)
 * The normaliser differs for every (hyper row, sample), so it is not a parameter of the record: the kernel evaluates it.
 * A parent index outside [0, Q) or equal to q gives NaN, which like every NaN population term counts as -inf.  Links may
 * form chains (3 on 1, 1 on 0) and a parent may have a higher index than its child; every term reads the sample's own
 * values, so the order of the columns does not matter.
 *
 * Interim records are of the kinds 1 .. 8.  iso_relation_lnlike_host refuses a LINGAUSS interim record;
 * iso_relation_lnlike cannot see its records (they are device memory) and gives NaN for it as for an unknown kind, which
 * makes every sample bad.
 *
 * Everything else is isochrones_amd_hier.h's, word for word: the per-sample log ratio r[h][s][m] and its ascending-q sum,
 * the bad samples (the parent is a used column: a NaN there is a bad sample), ell, ess and n_bad per star and row, the
 * mask, L and min_ess per row, and the addressing of ell, ess, n_bad, mask, L and min_ess and of a call's range of stars.
 *
 * Summation order of the device kernel.  It is k_hier_stars's: k_relation_stars gives a workgroup of 256 lanes one star and
 * a tile of ISO_RELATION_ROW_TILE consecutive rows; a row's arithmetic does not depend on its place in the tile nor on the
 * tile's size.  Lane i takes the samples m = i, i + 256, ... in ascending order: their maximum first, then in a second
 * pass over the same samples sum w and sum w^2, each from 0.0.  The 256 partial sums are combined by an xor butterfly
 * inside each of the four wavefronts (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3 over the wavefronts.
 * k_relation_total is k_hier_total.  The source writes no fused multiply-add and is compiled with -ffp-contract=off; no
 * floating-point atomics.  So a star's (ell, ess) for a row is the same bits alone, in any batch, in any sub-range of stars,
 * in any sub-range or tiling of the hyper rows, from a column and from a copy of it in another storage, and on a repeated
 * call; and records of the kinds 1 .. 8 alone give the bits of iso_hier_lnlike.  iso_relation_lnlike_host states the same
 * definition with plain ascending loops; the two agree to rounding, not bit for bit.
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_relation_lnlike launches on the given stream
 * and does not synchronise.  Return codes: 0 ok, ISO_RELATION_ERR_INVALID for a bad argument or a refused shape
 * (iso_relation_last_error() says which: it is refused, not answered), ISO_RELATION_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_RELATION_H
#define ISOCHRONES_AMD_RELATION_H

#include <stdint.h>

#include "isochrones_amd_hier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_RELATION_ERR_INVALID (-1)
#define ISO_RELATION_ERR_HIP (-2)

/* the record kind this library adds to ISO_HIER_FLAT .. ISO_HIER_TRUNCGAUSS */
#define ISO_RELATION_LINGAUSS 9
/* hyper rows a workgroup of k_relation_stars takes; no part of the summation order */
#define ISO_RELATION_ROW_TILE 8

const char* iso_relation_version(void);
const char* iso_relation_last_error(void);

/* the arguments of iso_hier_lnlike: columns is a host array of Q descriptors whose base pointers are device pointers.
 * interim ([Q]), rows ([H][Q]), mask ([n_ens] int32, or NULL), ell, ess ([H][n_ens]), n_bad ([n_ens] int32), L, min_ess
 * ([H], or both NULL): device pointers. */
int iso_relation_lnlike(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                        int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* rows,
                        int32_t H, const int32_t* mask, double* ell, double* ess, int32_t* n_bad, double* L,
                        double* min_ess, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; stream is ignored) */
int iso_relation_lnlike_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                             int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                             const iso_hier_record* rows, int32_t H, const int32_t* mask, double* ell, double* ess,
                             int32_t* n_bad, double* L, double* min_ess, void* stream);

/* host only: out[i * n + j] = ln f(x[j]; records[i]) with xp[j] the parent's value that goes with x[j], i < n_rec, j < n.
 * xp is read by LINGAUSS records only (their parent index is not looked at); it may be NULL when there is none. */
int iso_relation_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, const double* xp, int64_t n,
                            double* out);

#ifdef __cplusplus
}
#endif

#endif
