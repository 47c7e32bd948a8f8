/* C ABI of libiso_cluster.so: the star-cluster likelihood (StarClusterModel) for gfx950.
 *
 * The library allocates nothing, starts no resident waves and does not synchronise: every entry point launches on
 * device pointers the caller owns and on the stream it is given.  Return codes: 0 ok, ISO_CLUSTER_ERR_INVALID for a bad
 * argument, ISO_CLUSTER_ERR_HIP for a failed launch (iso_cluster_last_error() says which).
 *
 * Layout of one call over P parameter rows, N_s member stars, N_b bands and N_p further properties:
 *
 *   cols      [P][3 + 2 N_b + N_p][ld]  per row, the compacted EEP columns (only the first n_valid[r] entries are read):
 *                                       0: EEP, 1: initial mass m_j, 2: powerlaw_lnpdf(m_j; alpha, mass_lo, mass_hi) +
 *                                       ln|dm/dEEP|_j, 3 .. 3+N_b-1: 10^(-0.4 M_jb), 3+N_b .. 3+2N_b-1: M_jb, then the
 *                                       model value of each property
 *   n_valid   [P]      int32            number of valid EEPs of each row; clamped to [0, ld] (a count below 2 gives
 *                                       like_s = 0 for every star)
 *   rowpar    [P][4]                    ln fB, ln(1 - fB), gamma, ln C_q (C_q = (gamma+1) / (1 - minq^(gamma+1)))
 *   star_val  [N_b + N_p][N_s]          measured magnitudes, then property values
 *   star_w    [N_b + N_p][N_s]          1 / uncertainty^2 of the same
 *   work      [P][N_s][ld]              scratch: the inner integral I_sj of every (row, star, primary EEP)
 *   lnlike    [P]                       out: sum_s ln like_s, -inf when any like_s == 0
 *   lnlike_star [P][N_s] or NULL        out: ln like_s
 */
#ifndef ISOCHRONES_AMD_CLUSTER_H
#define ISOCHRONES_AMD_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_CLUSTER_MAX_BANDS 32
#define ISO_CLUSTER_MAX_PROPS 8
#define ISO_CLUSTER_ERR_INVALID (-1)
#define ISO_CLUSTER_ERR_HIP (-2)

const char* iso_cluster_version(void);
const char* iso_cluster_last_error(void);

int iso_cluster_lnlike(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                       const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                       double minq, double* work, double* lnlike, double* lnlike_star, void* stream);

#ifdef __cplusplus
}
#endif

#endif
