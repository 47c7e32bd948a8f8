/* C ABI of libiso_members.so: per-star moments of the star-cluster likelihood's integrand (StarClusterModel.star_moments)
 * for gfx950 - what a cluster fit says about each member star: its primary's EEP and mass, its mass ratio and secondary
 * mass, and how much of its likelihood comes from cells where every band's light is a pair's or a single star's.
 *
 * The library allocates nothing, starts no resident waves and does not synchronise: every entry point launches on device
 * pointers the caller owns and on the stream it is given (the _host entry takes host pointers and touches no device).
 * Return codes: 0 ok, ISO_MEMBERS_ERR_INVALID for a bad argument (nothing is launched), ISO_MEMBERS_ERR_HIP for a failed
 * launch (iso_members_last_error() says which).
 *
 * Inputs are exactly those of iso_cluster_lnlike (isochrones_amd_cluster.h), in the same layouts and with the same
 * clamping of n_valid to [0, ld], over P parameter rows, N_s member stars, N_b bands and N_p further properties:
 *
 *   cols      [P][3 + 2 N_b + N_p][ld]  0: EEP, 1: initial mass m_j, 2: mass_term_j, 3 .. 3+N_b-1: 10^(-0.4 M_jb),
 *                                       3+N_b .. 3+2N_b-1: M_jb, then the model value of each property
 *   n_valid   [P]      int32
 *   rowpar    [P][4]                    ln fB, ln(1 - fB), gamma, ln C_q
 *   star_val  [N_b + N_p][N_s]          measured magnitudes, then property values
 *   star_w    [N_b + N_p][N_s]          1 / uncertainty^2 of the same
 *   work      [P][N_s][6][ld]           scratch: the six inner integrals of every (row, star, primary EEP)
 *   ln_like   [P][N_s]                  out: ln like_s, the same bits as lnlike_star of iso_cluster_lnlike
 *   moments   [P][N_s][ISO_MEMBERS_NMOM] out: the eleven moments below
 *
 * Definition.  For row r, star s and cell (j, k <= j) let, per band b,
 *   a_b = ln fB + Lbin_b(j, k)          Lbin_b = -0.5 (M_b(j, k) - v_sb)^2 w_sb, M_b(j, k) = -2.5 log10(flux_jb + flux_kb)
 *   c_b = ln(1 - fB) + Lsingle_b(j)     Lsingle_b = -0.5 (M_jb - v_sb)^2 w_sb
 * the two arguments of the per-band logaddexp of the likelihood, and
 *   phot = sum_b logaddexp(a_b, c_b)
 *   q    = m_k / m_j                    the float64 quotient the mass-ratio cut is made on
 *   e    = exp(phot + mass_term_j + lnq + prop), or 0 where q < minq       (lnq = ln C_q + gamma ln q, prop the
 *                                                                           property term of (s, j))
 * each formed term by term in the order the likelihood forms it, with no fused multiply-add.  For a weight g(j, k)
 *   inner_g(j) = sum_{k=1..j} 0.5 (g_{k-1} e_{k-1} + g_k e_k) (eep_k - eep_{k-1})
 *   N_g        = sum_j 0.5 (u_j inner_g(j) + u_{j+1} inner_g(j+1)) (eep_{j+1} - eep_j)
 *   E[.]       = N_g / like_s,          like_s = N_1 with u = 1
 * where u_j depends on j only and the product g e is one float64 multiplication per cell.  A cell with e == 0
 * contributes 0 to every integral (a select, not a product: exp(-inf - -inf) and inf * 0 never arise at fB = 0, fB = 1
 * or below the cut).  The six weights g of the inner integrals, in the order of `work`:
 *   0: 1    1: q    2: q * q    3: pair = exp(sum_b a_b - phot)    4: single = exp(sum_b c_b - phot)    5: q * pair
 * (sum_b a_b and sum_b c_b in order of b, from 0).  The eleven moments:
 *
 *   index  moment                                          inner g     outer u_j
 *   0, 1   primary EEP, its square                         1           eep_j, eep_j * eep_j
 *   2, 3   primary mass, its square                        1           m_j, m_j * m_j
 *   4, 5   q, q^2                                          q, q * q    1
 *   6, 7   secondary mass, its square                      q, q * q    m_j, m_j * m_j
 *   8      p_pair: every band's light is the pair's        pair        1
 *   9      p_single: every band's light is the primary's   single      1
 *   10     E[q pair]                                       q * pair    1
 *
 * The model mixes pair and single per band, so p_pair + p_single = 1 with one band and is below 1 with more: the rest is
 * the weight of the mixed states.  q and the secondary mass are integrated over the whole grid whatever the state; the
 * mass ratio given a pair is moment 10 over moment 8.
 *
 * Summation order.  Both trapezoids run in ascending order of their index from 0.0, inner over k, outer over j:
 * acc = acc + 0.5 * (x_prev + x) * (eep - eep_prev), with x = u_j * inner_g(j) one multiplication in the outer one.
 * ln_like = log(N_1).  If like_s == 0 (n_valid < 2 included) ln_like is -inf and all eleven moments are NaN.  No atomics,
 * no order that depends on the batch: a (row, star) result is the same bits alone and in any batch.
 */
#ifndef ISOCHRONES_AMD_MEMBERS_H
#define ISOCHRONES_AMD_MEMBERS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_MEMBERS_MAX_BANDS 32
#define ISO_MEMBERS_MAX_PROPS 8
#define ISO_MEMBERS_NMOM 11
#define ISO_MEMBERS_NINNER 6
#define ISO_MEMBERS_ERR_INVALID (-1)
#define ISO_MEMBERS_ERR_HIP (-2)

const char* iso_members_version(void);
const char* iso_members_last_error(void);

int iso_members_moments(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                        const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                        double minq, double* work, double* ln_like, double* moments, void* stream);

int iso_members_moments_host(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                             const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                             double minq, double* work, double* ln_like, double* moments, void* stream);

#ifdef __cplusplus
}
#endif

#endif
