/* C ABI of libiso_binfit.so: the two moments of every star's posterior cell probabilities under a population density that
 * is piecewise constant on a grid of bins (the histogram of include/isochrones_amd_binned.h), summed over the stars, for
 * gfx950.  They are the expected number of stars per cell (the E-step of a maximum-likelihood fit of the cell heights, and
 * the gradient of that header's ln L with respect to the log heights) and the sum of the outer products of the cell
 * probabilities (its curvature).  Both come from the per-star table A that iso_binned_compress wrote; the chain is not read.
 *
 * Notation.  It is isochrones_amd_binned.h's: A [B][n_ens], cell-major, the table of n_ens stars over B cells
 * (1 <= B <= ISO_BINNED_MAX_CELLS); lnh [H][B] the log cell densities of H hyper rows, -inf a cell of height 0, a NaN counts
 * as -inf, +inf is not allowed (iso_binfit_moments_host refuses it); mask [n_ens] int32 or NULL, zero for a star to leave
 * out.  mx[s] cancels in everything below and is no input.
 *
 * Definition.  Per row h: hmx = max_b lnh[h][b] and u_b = exp(lnh[h][b] - hmx), 0 for a cell of height 0 (that header's u,
 * word for word).  Per (row, star), over ascending b from 0.0 with a separate multiply and add,
 *     s1[h][s] = sum_b u_b * A[b][s].
 * Rescue (isochrones_amd_binned.h gives the reason and the argument for the threshold): an unmasked star whose s1 is below
 * ISO_BINNED_RESCUE_BELOW = 2^-400, 0 included, is taken again relative to its own largest height.  A row's height is also
 * kept as u_b = m_b * 2^k_b with k_b = rint((lnh_b - hmx) / ln 2), at least -2^30, and m_b = u_b / 2^k_b (exact) where u_b is
 * a normal number, exp((lnh_b - hmx) - k_b ln 2) with ln 2 in two parts where it is not; m_b is in [0.70, 1.42], 0 for a
 * cell of height 0.  With kmax the largest k_b over the cells with A[b][s] > 0 and m_b > 0, the star's products become
 *     u_b * A[b][s] := (m_b * 2^(k_b - kmax)) * A[b][s]   over those cells, 0.0 in the others,
 * and s1 their sum over ascending b from 0.0 (0 if there is no such cell).  The common factor 2^kmax cancels in p.
 * Star s is live for row h if it is unmasked and s1 > 0: exactly where ell of iso_binned_lnlike is finite.  For a live star
 *     p[s][b] = (u_b * A[b][s]) / s1,
 * the posterior probability that the star lies in cell b; a star that is not live has p = 0 in every cell.  Over the live
 * stars, in ascending s, each sum from 0.0:
 *     N[h][b]     = sum_s p[s][b]                  the expected number of stars in cell b
 *     C[h][b][b'] = sum_s p[s][b] * p[s][b']       symmetric
 *     n_live[h]   = the number of live stars.
 * To rounding, sum_b N[h][b] = n_live[h] and sum_b' C[h][b][b'] = N[h][b].  With lnh as coordinates, not normalised,
 * d ln L / d lnh_b = N_b and d^2 ln L / d lnh_b d lnh_b' = delta_bb' N_b - C_bb'.  N is [H][B], C [H][B][B] (or NULL: the
 * pair sums are not taken), n_live [H] int32.  A sub-range of the rows is a call with lnh, N, C and n_live advanced to its
 * first row.  A table of one star (an injection set's, n_ens = 1) gives q_b, the same first moment of the selection term.
 *
 * Summation order of the device kernels.  k_binfit_partial gives a workgroup of 256 lanes one (chunk of ISO_BINFIT_CHUNK
 * consecutive stars, row).  It takes the chunk's stars in ascending order a tile of ISO_BINFIT_TILE at a time: the tile's
 * u_b * A[b][s] is staged in LDS, one lane per star adds its s1 over ascending b, and every entry is divided by its
 * star's s1 (0 where the star is not live); the lane that added a star's s1 writes a rescued star's products over the staged
 * ones before the division (the m_b of the row wait in the tile's pad column, written once per workgroup), by the function the host
 * entry calls.  Every output has one owner lane: lane 64 + b owns N_b, and the B (B + 1) / 2
 * pairs b <= b' are dealt out in blocks of 3 x 3 cells, block (I, J), I <= J, numbered row by row, to lane number of the
 * block (at most 253 blocks of at most 9 pairs a lane; a lane reads six values a star for its nine products).  An owner
 * walks the tile's stars in ascending order and adds p[s][b], or p[s][b] * p[s][b'] with a separate multiply and add, to
 * an accumulator of that output alone that starts at 0.0 with the chunk and runs on from tile to tile (a star that is not
 * live adds +0.0, which changes no bit).  So a chunk's partial sum is the ascending sum of the definition over the chunk's stars whatever the
 * tile size: the chunk size is part of the summation order, the tile size is not.  The partial sums go to the workspace,
 * [H][n_chunks][B + B (B + 1) / 2] doubles (the pair part is absent without C), the chunks' live counts after them as
 * int32 [H][n_chunks].  k_binfit_total gives a workgroup one row: the owner of an output adds the chunks' partial sums in
 * ascending order from 0.0, and a pair's sum is written to C[b][b'] and C[b'][b].  No floating-point atomics; the source
 * writes no fused multiply-add and is compiled with -ffp-contract=off.  So a row's outputs are the same bits alone, in any
 * sub-range of the rows and on a repeated call.  iso_binfit_moments_host states the same definition with plain ascending
 * loops over all stars; device and host agree to rounding, not bit for bit (exp differs, and the host has no chunks).
 *
 * The library works on pointers the caller owns.  The device entry allocates nothing, launches on the given stream and does
 * not synchronise; the workspace holds iso_binfit_workspace_doubles(B, n_ens, H, with_pairs) doubles.  Return codes: 0 ok,
 * ISO_BINFIT_ERR_INVALID for a bad argument or a refused shape (iso_binfit_last_error() says which: it is refused, not
 * answered), ISO_BINFIT_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_BINFIT_H
#define ISOCHRONES_AMD_BINFIT_H

#include <stdint.h>

#include "isochrones_amd_binned.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_BINFIT_ERR_INVALID (-1)
#define ISO_BINFIT_ERR_HIP (-2)

/* stars a workgroup of k_binfit_partial sums; part of the summation order */
#define ISO_BINFIT_CHUNK 4096
/* stars staged in LDS at a time; no part of the summation order */
#define ISO_BINFIT_TILE 64

const char* iso_binfit_version(void);
const char* iso_binfit_last_error(void);

/* doubles of workspace iso_binfit_moments needs (0 for a shape it refuses); with_pairs: C is not NULL */
int64_t iso_binfit_workspace_doubles(int32_t B, int32_t n_ens, int32_t H, int with_pairs);

/* A ([B][n_ens]), lnh ([H][B]), mask ([n_ens] int32, or NULL), N ([H][B]), C ([H][B][B], or NULL), n_live ([H] int32),
 * workspace: device pointers.  1 <= B <= ISO_BINNED_MAX_CELLS, n_ens >= 1, H >= 1. */
int iso_binfit_moments(const double* A, int32_t B, int32_t n_ens, const double* lnh, int32_t H, const int32_t* mask,
                       double* N, double* C, int32_t* n_live, double* workspace, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; workspace and stream are ignored);
 * it sees lnh and refuses a +inf in it */
int iso_binfit_moments_host(const double* A, int32_t B, int32_t n_ens, const double* lnh, int32_t H, const int32_t* mask,
                            double* N, double* C, int32_t* n_live, double* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
