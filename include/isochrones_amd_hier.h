/* C ABI of libiso_hier.so: the hierarchical (population) likelihood of a catalog from the stored chains of its stars, by
 * importance reweighting of every star's posterior samples under a population density (Hogg, Myers & Bovy 2010), for
 * gfx950.
 *
 * Inputs.  There are S ensembles ("stars"), each with M = W * T stored samples (W walkers, T = nsteps steps; sample
 * m = t * W + w).  There are Q value columns x_q[s][m], 1 <= Q <= 4.  Every column is read from a storage of nsteps steps,
 * C_q columns and n_q * W rows in the call's layout (parameter-major [T][C_q][n_q * W], the sampler's own, or row-major
 * [T][n_q * W][C_q]): the sampler's chain or a derived chain.  A column is passed as an iso_hier_column (base pointer, C_q,
 * column index, n_q, first): the kernel reads it where it lies, without a copy.  `first` is the number, in the call's
 * numbering 0 .. n_ens - 1, of the storage's first ensemble, so that a derived chain made for a slice of the stars sits
 * next to the whole sampler chain: ensemble s is the storage's ensemble s - first.
 *
 * Family record.  An iso_hier_record holds a kind, lo, hi and six doubles p[0..5]: the parameters and the log-normalisers,
 * precomputed on the host.  ln f(x; record) is what the matching class of isochrones_amd/priors.py defines as lnpdf, its
 * bounds test and the -inf outside included ("out" below: x < lo or x > hi; a NaN x is never out).  With lx = ln x:
 *   FLAT        out: -inf; p0                                            p0 = ln(1 / (hi - lo))
 *   FLATLOG     out: -inf; p0 + x * ln 10                                p0 = ln(ln 10 / (10^hi - 10^lo))
 *   POWERLAW    out: -inf; p0 + p1 * lx                                  p0 = ln C, p1 = alpha
 *   GAUSS       out: -inf; z = (x - p0) * p3; -(z * z) / 2 + p2          p0 = mean, p1 = sigma, p3 = 1 / sigma,
 *               p2 = -ln sqrt(2 pi) - ln sigma - lognorm (GaussianPrior's own norm); unbounded: lo = -inf, hi = +inf
 *   LOGNORMAL   no bounds test; l = lx - p0; v = l * p3; (p2 - l) - 0.5 * (v * v)
 *               p0 = mu, p1 = sigma, p3 = 1 / sigma, p2 = -ln sqrt(2 pi) - ln sigma - mu; NaN for x <= 0, as lnpdf
 *   CHABRIER    x < p5: l = lx - p0; v = l * p1; (p2 - l) - 0.5 * (v * v); otherwise out: -inf; p4 + p3 * lx
 *               p0 = mu, p1 = 1 / sigma, p2 = -ln sqrt(2 pi) - ln sigma - mu - lognorms[0], p3 = alpha,
 *               p4 = ln C - lognorms[1], p5 = breakpoint; lo, hi = the power law's bounds (lnpdf tests no others)
 *   FEH         out: -inf; ln(shape(x) / p1), shape = p0 * halo + (1 - p0) * disk as FehPrior._shape
 *               p0 = halo fraction, p1 = norm, p2 = 1 for the local disk, 0 otherwise; default bounds: -inf, +inf
 *   TRUNCGAUSS  GAUSS's arithmetic with p2 = -ln sqrt(2 pi) - ln sigma - ln(Phi((hi - mean) / sigma) - Phi((lo - mean) /
 *               sigma)): a Gaussian renormalised on [lo, hi]
 * An unknown kind gives NaN.
 *
 * Interim and population records.  interim[q], q < Q: the prior the fit used for column q.  rows[h * Q + q], h < H: the
 * population density of hyper row h for column q.
 *
 * Per-sample log ratio.  d_q = ln f_{h,q}(x_q) - ln f0_q(x_q); r[h][s][m] = d_0, then + d_1, + d_2, + d_3 (ascending q).
 * A population term that is NaN (LOGNORMAL, CHABRIER at x <= 0) counts as -inf.
 *
 * Bad samples.  A sample is bad if a used column is NaN or an interim term is -inf (density zero) or NaN.  A bad sample
 * has weight 0 under every row and is counted once in n_bad[s].  M in the mean stays W * T.
 *
 * Per star and row.  With mx = max_m r over good samples, w = exp(r - mx):
 *     ell[h][s] = mx + ln(sum_m w) - ln M,         ess[h][s] = (sum_m w)^2 / sum_m w^2.
 * If no good sample has r > -inf: ell = -inf, ess = 0.  A star with mask[s] == 0 has ell = ess = NaN, n_bad = 0 (its
 * samples are not read) and adds nothing to L; mask == NULL masks nothing.
 *
 * Per row.  L[h] = sum_s ell[h][s] and min_ess[h] = min_s ess[h][s] over the unmasked stars (0 and +inf when there is
 * none).
 *
 * Addressing.  ell and ess are [H][n_ens], n_bad and mask [n_ens], all in the call's numbering; a call writes the stars
 * [ens_begin, ens_begin + n_ens_out) and leaves the rest alone.  L and min_ess ([H]; both or neither) are taken over all
 * n_ens stars of ell and ess as they stand after the call's own stars are written: a caller that slices the stars passes
 * them with its last slice.
 *
 * Summation order of the device kernel.  It depends on W and T only.  k_hier_stars gives a workgroup of 256 lanes one
 * star and a tile of ISO_HIER_ROW_TILE consecutive rows; a row's arithmetic does not depend on its place in the tile.
 * Lane i takes the samples m = i, i + 256, ... in ascending order: their maximum first, then in a second pass over the
 * same samples sum w and sum w^2, each from 0.0.  The 256 partial sums are combined by an xor butterfly inside each of
 * the four wavefronts (distances 32, 16, ..., 1), then ((v0 + v1) + v2) + v3 over the wavefronts.  The source writes no
 * fused multiply-add and is compiled with -ffp-contract=off.  So a star's (ell, ess) for a row is the same bits alone,
 * in any batch, in any sub-range of stars and in any sub-range or tiling of the hyper rows, and from a column and from a
 * copy of it in another storage.  k_hier_total gives a workgroup one row: lane i adds the unmasked stars s = i, i + 256, ...
 * in ascending order, then the same butterfly and wavefront order; no floating-point atomics, so a repeated call returns
 * the same bits.  iso_hier_lnlike_host states the same definition with plain ascending loops; the two agree to rounding,
 * not bit for bit.
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_hier_lnlike launches on the given stream and
 * does not synchronise.  Return codes: 0 ok, ISO_HIER_ERR_INVALID for a bad argument or a refused shape
 * (iso_hier_last_error() says which: it is refused, not answered), ISO_HIER_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_HIER_H
#define ISOCHRONES_AMD_HIER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_HIER_ERR_INVALID (-1)
#define ISO_HIER_ERR_HIP (-2)

/* chain layouts: the values of ISO_CHAIN_ROW_MAJOR / ISO_CHAIN_PARAM_MAJOR of isochrones_amd.h */
#define ISO_HIER_ROW_MAJOR 0
#define ISO_HIER_PARAM_MAJOR 1

#define ISO_HIER_MAX_COLS 4
#define ISO_HIER_NPAR 6
#define ISO_HIER_ROW_TILE 8

/* kinds: 1 .. 7 are the ISO_PRIOR_* values of isochrones_amd.h */
#define ISO_HIER_FLAT 1
#define ISO_HIER_FLATLOG 2
#define ISO_HIER_POWERLAW 3
#define ISO_HIER_GAUSS 4
#define ISO_HIER_LOGNORMAL 5
#define ISO_HIER_CHABRIER 6
#define ISO_HIER_FEH 7
#define ISO_HIER_TRUNCGAUSS 8

typedef struct iso_hier_record {
    int32_t kind;
    int32_t reserved;
    double lo, hi;
    double p[ISO_HIER_NPAR];
} iso_hier_record;

typedef struct iso_hier_column {
    const double* base; /* the storage: nsteps steps, ncols columns, n_ens * W rows, in the call's layout */
    int32_t ncols;
    int32_t col;        /* the column read, 0 <= col < ncols */
    int32_t n_ens;      /* ensembles the storage holds */
    int32_t first;      /* the call's number of the storage's first ensemble: first <= ens_begin and
                           ens_begin + n_ens_out <= first + n_ens */
} iso_hier_column;

const char* iso_hier_version(void);
const char* iso_hier_last_error(void);

/* columns: host array of Q descriptors whose base pointers are device pointers.  interim ([Q]), rows ([H][Q]), mask
 * ([n_ens] int32, or NULL), ell, ess ([H][n_ens]), n_bad ([n_ens] int32), L, min_ess ([H], or both NULL): device pointers. */
int iso_hier_lnlike(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                    int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* rows,
                    int32_t H, const int32_t* mask, double* ell, double* ess, int32_t* n_bad, double* L, double* min_ess,
                    void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; stream is ignored) */
int iso_hier_lnlike_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                         int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                         const iso_hier_record* rows, int32_t H, const int32_t* mask, double* ell, double* ess,
                         int32_t* n_bad, double* L, double* min_ess, void* stream);

/* host only: out[i * n + j] = ln f(x[j]; records[i]), i < n_rec, j < n */
int iso_hier_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, int64_t n, double* out);

#ifdef __cplusplus
}
#endif

#endif
