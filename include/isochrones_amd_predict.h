/* C ABI of libiso_predict.so: the posterior-predictive check of a stored ensemble-sampler chain, for gfx950.  At every
 * sample of the chain the model's magnitudes (through the bolometric-correction grid), Teff, logg, [Fe/H] and parallax are
 * evaluated and compared with the star's own measurements; per ensemble the call returns the mean chi-square of every
 * term, their mean over the terms (the reference's StarModel.posterior_predictive), the sample of largest log-probability
 * (map_pars) and, as a chain of its own in the sampler's storage layout, the system magnitudes - which the quantile entry
 * point of libiso_hip.so (iso_chain_quantiles_layout) summarises where they lie.
 *
 * Model table.  cols[n0][n1][nk][4]: the columns (Teff, logg, feh, Mbol) of a 3-D model grid, the four values of one node
 * adjacent, NaN-padded as the grid is, with its axes ax0, ax1, axk: the layout and the rules of iso_derived_table
 * (isochrones_amd_derived.h) with Q = 4.  n0 * n1 * nk * 4 <= 2^31 - 1.
 *
 * Bolometric-correction table.  bc[nT][ng][nf][nA][B]: B selected band columns of the 4-D grid on (Teff, logg, [Fe/H],
 * AV), the B values of one node adjacent, with its axes axT, axg, axf, axA (strictly increasing, at least 2 nodes each);
 * 1 <= B <= ISO_PREDICT_MAX_BANDS.  nT * ng * nf * nA * B <= 2^31 - 1.
 *
 * Chain.  nsteps x (n_ens * W) rows x ndim parameters, float64, in either layout of isochrones_amd_derived.h:
 *   ISO_PREDICT_PARAM_MAJOR  chain[(t * ndim + d) * (n_ens * W) + row]     (the sampler's storage, read in place)
 *   ISO_PREDICT_ROW_MAJOR    chain[(t * (n_ens * W) + row) * ndim + d]
 * with row = ensemble * W + walker.  lnprob[t * (n_ens * W) + row] is the sampler's log-probability of that sample; it
 * may be null.  The call works on the ensembles [ens_begin, ens_begin + n_ens_out); R = n_ens_out * W, r = row -
 * ens_begin * W, e = ensemble - ens_begin.  nsteps * W <= 2^31 - 1.
 *
 * Components.  comps[C][3] (host memory), 1 <= C <= ISO_PREDICT_MAX_COMPS, as in isochrones_amd_derived.h: component c
 * reads its coordinates on (ax0, ax1, axk) from the chain parameters comps[c][0..2].  i_dist and i_AV are the chain
 * parameters that hold the distance (pc) and AV of the system.
 *
 * Observations.  obs_val[n_ens][B + 4] and obs_unc[n_ens][B + 4], indexed by the ensemble itself (not by e): the B bands,
 * then Teff, logg, feh, parallax.  A NaN value means that the term is absent for that star.
 *
 * One sample.  Every operation is one IEEE float64 operation rounded on its own, in the order written; no fused
 * multiply-add anywhere (the library is built with -ffp-contract=off and writes no fma).
 *   1. per component c: (Teff_c, logg_c, feh_c, Mbol_c) = the four model columns at (x0, x1, xk), trilinear, by the rules
 *      of isochrones_amd_derived.h (corner order 000 .. 111 with bk fastest, weight (f0 * f1) * fk, value = 0.0 then
 *      value + node * weight per corner, NaN off an axis, a NaN neighbour propagates);
 *   2. bc_c[b] = the B columns of the BC table at (Teff_c, logg_c, feh_c, AV) by the same rule in four dimensions: per
 *      axis i = the largest index with ax[i] <= x but at most n - 2, t = (x - ax[i]) / (ax[i + 1] - ax[i]), u = 1 - t;
 *      the sixteen corners in the order (bT, bg, bf, bA) = 0000, 0001, ... 1111 (bA fastest), weight ((fT * fg) * ff) *
 *      fA; a NaN coordinate or one outside its axis gives NaN for every band (oracle/iso_oracle.c, orc_interp_value);
 *   3. mag_c[b] = (Mbol_c + 5 * log10(distance / 10)) - bc_c[b];
 *   4. the system magnitude mag[b] is mag_0[b] for C = 1, else -2.5 * log10(sum), sum = 0.0 then sum + pow(10, -0.4 *
 *      mag_c[b]) for c ascending;
 *   5. the system's Teff, logg and feh are component 0's; the model parallax is 1000 / distance;
 *   6. term j (band b: j = b; Teff, logg, feh, parallax: j = B .. B + 3), present when obs_val[j] is not NaN:
 *      d = obs_val[j] - model[j], z_j = (d * d) / (obs_unc[j] * obs_unc[j]).
 * log10 and pow are the math library's of the side that runs (device or host), so a magnitude of the kernel and one of the
 * host entry may differ in the last bits; everything else is the same sequence of operations on both sides (steps 1 and
 * 2 are one statement, the internal csrc/common/grid_interp.h, compiled for the kernel and for the host entry).
 * A sample is bad when the model value of any present term is not finite.  Bad samples enter no mean and are counted.
 *
 * Means and their summation order.  The samples of one ensemble are numbered s = t * W + walker, 0 <= s < nsteps * W.
 * Partial sum l, 0 <= l < ISO_PREDICT_LANES: 0.0, then + z_j of the good samples with s mod ISO_PREDICT_LANES == l, s
 * ascending.  The partials are combined by the tree  for h = ISO_PREDICT_LANES / 2, / 4, ... 1: p[l] = p[l] + p[l + h]
 * for every l < h;  the mean is p[0] / (number of good samples).  The sums use no floating-point atomics and depend on the
 * ensemble's own samples only, so a star's outputs are bit-identical alone, in any batch, in any ensemble range and from
 * either chain layout.
 *
 * Outputs, every one skipped when its pointer is null:
 *   mags[(t * B + b) * R + r]    the system-magnitude chain in parameter-major storage [nsteps][B][R], which
 *                                iso_chain_quantiles_layout takes with n_params = B; NaN where the sample is off a grid
 *   term_chi2[e * (B + 4) + j]   the mean of z_j over the ensemble's good samples; NaN for an absent term
 *   ppc[e]                       the sum over the present terms, j ascending from 0.0, of those means, divided by the
 *                                number of present terms; NaN if no term is present or no sample is good
 *   n_bad[e]                     (int32) the number of bad samples
 *   mag_nan[e * B + b]           (int32) the number of samples whose system magnitude in band b is NaN (what mags holds,
 *                                whether or not mags is asked for)
 *   map_index[e], map_pars[e * ndim + d]   (int64; needs lnprob, else nothing is written) s = t * W + walker of the sample
 *                                with the largest non-NaN lnprob, ties to the lowest s (the lowest t, then the lowest
 *                                walker), and its ndim parameters; -1 and NaN if every lnprob is NaN
 *
 * The library allocates nothing and works on device pointers the caller owns (comps and the table structs themselves are
 * host memory, read before the call returns).  iso_predict_chain launches on the given stream and does not synchronise.
 * iso_predict_chain_host does the same on host pointers in plain C++ with ascending loops and touches no device.  Return
 * codes: 0 ok, ISO_PREDICT_ERR_INVALID for a bad argument (iso_predict_last_error() says which), ISO_PREDICT_ERR_HIP for
 * a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_PREDICT_H
#define ISOCHRONES_AMD_PREDICT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_PREDICT_ERR_INVALID (-1)
#define ISO_PREDICT_ERR_HIP (-2)

/* chain layouts: the values of ISO_CHAIN_ROW_MAJOR / ISO_CHAIN_PARAM_MAJOR of isochrones_amd.h */
#define ISO_PREDICT_ROW_MAJOR 0
#define ISO_PREDICT_PARAM_MAJOR 1

#define ISO_PREDICT_MAX_BANDS 32
#define ISO_PREDICT_MAX_COMPS 3
#define ISO_PREDICT_NSPEC 4
#define ISO_PREDICT_LANES 128
/* the grid's cap: one workgroup an ensemble; a call of more than ISO_PREDICT_MAX_BLOCKS ensembles strides */
#define ISO_PREDICT_MAX_BLOCKS 2048

/* every pointer is a device pointer the caller owns (a host pointer for iso_predict_chain_host) */
typedef struct iso_predict_model_table {
    const double* cols;
    const double* ax0;
    const double* ax1;
    const double* axk;
    int32_t n0, n1, nk, reserved;
} iso_predict_model_table;

typedef struct iso_predict_bc_table {
    const double* bc;
    const double* axT;
    const double* axg;
    const double* axf;
    const double* axA;
    int32_t nT, ng, nf, nA, B, reserved;
} iso_predict_bc_table;

/* the outputs of one call; a null pointer skips that output */
typedef struct iso_predict_out {
    double* mags;
    double* term_chi2;
    double* ppc;
    int32_t* n_bad;
    int64_t* map_index;
    double* map_pars;
    int32_t* mag_nan;
} iso_predict_out;

const char* iso_predict_version(void);
const char* iso_predict_last_error(void);

int iso_predict_chain(const iso_predict_model_table* model, const iso_predict_bc_table* bc, const double* chain,
                      const double* lnprob, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                      int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C, int32_t i_dist, int32_t i_AV,
                      const double* obs_val, const double* obs_unc, const iso_predict_out* out, void* stream);

/* the same on host pointers, in plain C++ (no device is touched; stream is ignored) */
int iso_predict_chain_host(const iso_predict_model_table* model, const iso_predict_bc_table* bc, const double* chain,
                           const double* lnprob, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                           int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C, int32_t i_dist,
                           int32_t i_AV, const double* obs_val, const double* obs_unc, const iso_predict_out* out,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif
