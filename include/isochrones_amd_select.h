/* C ABI of libiso_select.so: the detectable fraction alpha of a population density under a survey's selection, estimated
 * from an injection set by importance reweighting (Mandel, Farr & Gair 2019; Farr 2019), for gfx950.  It is the selection
 * term of the hierarchical likelihood of include/isochrones_amd_hier.h:
 *     ln L_sel(h) = sum_s ell[h][s] - S_unmasked * ln_alpha[h].
 *
 * Inputs.  There are J injections, 1 <= J <= 2^31 - 1, drawn from a known density g = prod_q g_q, with Q value columns,
 * 1 <= Q <= 4.  x is [Q][J] (column q of injection j at x[q * J + j]: consecutive injections are consecutive doubles).
 * lnd is [J]: the natural log of the probability that injection j is detected, -inf for an undetected one, +0 for a
 * certainly detected one.  draw is [Q] iso_hier_record (isochrones_amd_hier.h: the family record and ln f of it are used
 * as they stand): draw[q] is g_q.  rows is [H][Q]: rows[h * Q + q] is the population density f_{h,q} of hyper row h.
 *
 * Per injection and row.  d_q = ln f_{h,q}(x_q) - ln g_q(x_q); r = d_0, then + d_1, + d_2, + d_3 (ascending q);
 * t[h][j] = r + lnd[j] (lnd is added last).  A population term that is NaN (LOGNORMAL, CHABRIER at x <= 0) counts as -inf.
 *
 * Bad injections.  An injection is bad if a used column is NaN, a draw term is -inf (density zero) or NaN, or lnd is NaN
 * or positive.  A bad injection has weight 0 under every row and is counted once in n_bad[0].  J in the mean stays J.
 *
 * Per row.  With MX = max_j t over the good injections and w_j = exp(t_j - MX) (0 for a bad one):
 *     ln_alpha[h] = MX + ln(sum_j w_j) - ln J,         n_eff[h] = (sum_j w_j)^2 / sum_j w_j^2.
 * If no good injection has t > -inf (no support, or nothing detected): ln_alpha = -inf, n_eff = 0.
 *
 * Summation order of the device kernels.  It depends on J and ISO_SELECT_CHUNK only.  The injections are cut into chunks
 * of ISO_SELECT_CHUNK consecutive ones (the last one ragged).  k_select_partial gives a workgroup of 256 lanes one chunk
 * and a tile of ISO_HIER_ROW_TILE consecutive rows; a row's arithmetic does not depend on its place in the tile.  Lane i
 * takes the chunk's injections i, i + 256, ... in ascending order: their maximum first, then in a second pass over the
 * same injections sum w and sum w^2 relative to the chunk's own maximum mx_c, each from 0.0.  The 256 partial values are
 * combined by an xor butterfly inside each of the four wavefronts (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3
 * over the wavefronts.  Per (chunk, row) the workgroup writes (mx_c, s1_c, s2_c) to the workspace; a chunk without a good
 * injection of t > -inf writes (-inf, 0, 0).  k_select_total gives a workgroup one row: MX = max_c mx_c,
 *     S1 = sum_c s1_c * exp(mx_c - MX),      S2 = sum_c s2_c * exp(2 * (mx_c - MX)),
 * lane i taking the chunks i, i + 256, ... in ascending order, then the same butterfly and wavefront order;
 * ln_alpha = (MX + ln S1) - ln J, n_eff = (S1 * S1) / S2.  n_bad is the sum of per-chunk integer counts.  No
 * floating-point atomics; the source writes no fused multiply-add and is compiled with -ffp-contract=off.  So a row's
 * (ln_alpha, n_eff) is the same bits alone, in any sub-range or tiling of the hyper rows, on a repeated call and from a copy
 * of x at another address.  iso_select_alpha_host states the same definition with plain ascending loops and one global
 * maximum; the two agree to rounding, not bit for bit.
 *
 * Workspace.  iso_select_alpha needs iso_select_workspace_doubles(J, H) doubles of device memory the caller owns (three per
 * (chunk, row) and the chunks' counts); their contents before the call do not matter and mean nothing after it.  The host
 * entry ignores the workspace (NULL is fine).
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_select_alpha launches on the given stream and
 * does not synchronise.  Return codes: 0 ok, ISO_SELECT_ERR_INVALID for a bad argument or a refused shape
 * (iso_select_last_error() says which: it is refused, not answered), ISO_SELECT_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_SELECT_H
#define ISOCHRONES_AMD_SELECT_H

#include <stdint.h>

#include "isochrones_amd_hier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_SELECT_ERR_INVALID (-1)
#define ISO_SELECT_ERR_HIP (-2)

/* injections per workgroup of k_select_partial: part of the summation order */
#define ISO_SELECT_CHUNK 4096

const char* iso_select_version(void);
const char* iso_select_last_error(void);

/* doubles of workspace a call with J injections and H rows needs; 0 for J < 1 or H < 1 */
int64_t iso_select_workspace_doubles(int64_t J, int32_t H);

/* x ([Q][J]), lnd ([J]), draw ([Q]), rows ([H][Q]), workspace, ln_alpha, n_eff ([H]), n_bad ([1] int32): device pointers */
int iso_select_alpha(const double* x, int32_t Q, int64_t J, const double* lnd, const iso_hier_record* draw,
                     const iso_hier_record* rows, int32_t H, double* workspace, double* ln_alpha, double* n_eff,
                     int32_t* n_bad, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; workspace and stream are ignored) */
int iso_select_alpha_host(const double* x, int32_t Q, int64_t J, const double* lnd, const iso_hier_record* draw,
                          const iso_hier_record* rows, int32_t H, double* workspace, double* ln_alpha, double* n_eff,
                          int32_t* n_bad, void* stream);

/* host only: out[i * n + j] = ln f(x[j]; records[i]), i < n_rec, j < n; iso_hier_lnpdf_host's arithmetic, bit for bit */
int iso_select_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, int64_t n, double* out);

#ifdef __cplusplus
}
#endif

#endif
