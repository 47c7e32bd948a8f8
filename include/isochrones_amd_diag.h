/* C ABI of libiso_diag.so: convergence diagnostics of a stored ensemble-sampler chain, one row per (ensemble,
 * parameter) pair, for gfx950.
 *
 * For one pair the input is the slab x[t][w], t < T = nsteps, w < W walkers, float64.
 *
 * Centring.  m_w = (1/T) sum_t x[t][w], y[t][w] = x[t][w] - m_w: two passes.  Every product below is formed from
 * centred values, never as sum(x^2) - T m^2.  (Both implementations take the mean about the walker's first value,
 * m_w = x[0][w] + (1/T) sum_t (x[t][w] - x[0][w]) and y = (x - x[0][w]) - that mean: a walker that never moved centres
 * to exact zeros whatever its value.)
 *
 * Pooled autocovariance.  K = min(T - 1, max_lag).  For k = 0..K
 *     A(k) = sum_w sum_{t=0}^{T-1-k} y[t][w] * y[t+k][w],       rho(k) = A(k) / A(0).
 * The walkers are pooled before the division (emcee averages per-walker normalised functions, where a walker that
 * never moved gives 0/0 and makes the estimate NaN; here it contributes zeros).
 *
 * Integrated time with Sokal's window.  tau(M) = 1 + 2 sum_{k=1}^{M} rho(k).  M* is the smallest M in 0..K with
 * M >= c * tau(M); if there is none, M* = K and window_ok = 0, otherwise window_ok = 1.  tau = tau(M*),
 * ess = W * T / tau.  A(0) == 0 (no walker ever moved) gives tau = ess = NaN, window = K and window_ok = 0.
 *
 * Split R-hat.  n = T / 2 (integer division).  Each walker gives two chains, t in [0, n) and t in [T - n, T) (an odd T
 * drops the middle step).  Over the 2 W chains: means mu_j, variances s_j^2 with divisor n - 1 (two passes),
 * Wv = mean(s_j^2), B = n * var(mu_j) with divisor 2 W - 1 (two passes),
 *     rhat = sqrt(((n - 1) / n * Wv + B / n) / Wv).
 * T < 4 or Wv == 0 gives NaN.
 *
 * Output.  out[(s * ndim + d) * 5 + i], i = ISO_DIAG_TAU, _WINDOW (M* as a double), _WINDOW_OK (1.0 or 0.0), _ESS,
 * _RHAT.  A NaN or an infinity anywhere in the slab makes all five NaN (Inf - Inf in the centring makes A(0) NaN).
 *
 * Summation order of the device kernel (fixed, independent of the batch, so a pair's row is bit-identical alone or in
 * any batch): walker w belongs to group w mod 4; inside a group A(k) accumulates walker after walker in ascending w
 * and, inside a walker, in ascending t, each term one fused multiply-add; A(k) = ((g0 + g1) + g2) + g3.  tau(M) is
 * summed in ascending k.  Sums over the 2 W split chains: lane l of one wavefront adds j = l, l + 64, ... in ascending
 * order, then the 64 partial sums are combined by an xor butterfly (distances 32, 16, ..., 1).  iso_diag_chain_host
 * states the same definition with plain ascending loops; the two agree to rounding, not bit for bit.
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_diag_chain launches on the given stream and
 * does not synchronise.  Return codes: 0 ok, ISO_DIAG_ERR_INVALID for a bad argument or a shape the kernel's staging
 * scheme cannot take (iso_diag_last_error() says which: it is refused, not answered), ISO_DIAG_ERR_HIP for a failed
 * runtime call.
 */
#ifndef ISOCHRONES_AMD_DIAG_H
#define ISOCHRONES_AMD_DIAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_DIAG_ERR_INVALID (-1)
#define ISO_DIAG_ERR_HIP (-2)

/* chain layouts: the values of ISO_CHAIN_ROW_MAJOR / ISO_CHAIN_PARAM_MAJOR of isochrones_amd.h */
#define ISO_DIAG_ROW_MAJOR 0   /* chain [nsteps][n_ens * W][ndim] */
#define ISO_DIAG_PARAM_MAJOR 1 /* chain [nsteps][ndim][n_ens * W]: a pair's walkers are consecutive doubles */

#define ISO_DIAG_NOUT 5
#define ISO_DIAG_TAU 0
#define ISO_DIAG_WINDOW 1
#define ISO_DIAG_WINDOW_OK 2
#define ISO_DIAG_ESS 3
#define ISO_DIAG_RHAT 4

#define ISO_DIAG_DEFAULT_C 5.0
#define ISO_DIAG_DEFAULT_MAX_LAG 1024

const char* iso_diag_version(void);
const char* iso_diag_last_error(void);

/* chain, out: device pointers; out holds n_ens * ndim * 5 doubles.  c finite and > 0, max_lag >= 1. */
int iso_diag_chain(const double* chain, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim, double c,
                   int32_t max_lag, double* out, void* stream);

/* the same on host pointers, in plain C++ (no device is touched; stream is ignored) */
int iso_diag_chain_host(const double* chain, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                        double c, int32_t max_lag, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
