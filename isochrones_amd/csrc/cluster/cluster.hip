// Star-cluster likelihood (StarClusterModel.lnlike) for gfx950: the (primary EEP j, secondary EEP k <= j) grid of every
// member star, its two trapezoid integrals and the sum of ln like_s over the stars.  See include/isochrones_amd_cluster.h
// for the data layout and DESIGN.md section 10 for the decomposition.
//
// Two kernels, both with a fixed order of every reduction, so that a row's result does not depend on which rows share
// its launch:
//   k_cluster_pairs   one 64-lane workgroup per (row, tile of 64 stars, primary EEP j).  The star-independent work of a
//                     pair (j, k) - the binary magnitude of each band, the mass-ratio cut and term - is computed once per
//                     pair by one lane for 64 secondaries at a time and read by all 64 stars from LDS; the per-(star, j)
//                     terms (single-star term of each band, property term) are computed once before the k loop.  Each
//                     lane walks k = 0 .. j in order and writes the inner integral I_sj.
//   k_cluster_finish  one workgroup per row: like_s = trapz(I_s, eep) in order of j, ln like_s, and a fixed-tree sum
//                     over the stars.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "isochrones_amd_cluster.h"
#include "../common/last_error.h"

namespace {

constexpr int TILE = 64;          // stars per workgroup = lanes of one wave
constexpr int FINISH = 256;       // threads of the per-row finishing workgroup

// the reference's logaddexp (cluster_utils.py): xmax + log(exp(x1 - xmax) + exp(x2 - xmax)).  One of the two exponentials
// is exp(0) = 1 exactly, so only the other is evaluated; the sum is the same double.  ln 0 = -inf on one side selects
// the other; NaN on either side gives NaN, as there.
__device__ __forceinline__ double logaddexp(double a, double b) {
    const bool second = b > a;
    const double hi = second ? b : a;
    const double lo = second ? a : b;
    return hi + log(exp(lo - hi) + 1.0);
}

__global__ void __launch_bounds__(TILE) k_cluster_pairs(const double* __restrict__ cols, int64_t ld, int64_t tiles,
                                                        const int32_t* __restrict__ n_valid,
                                                        const double* __restrict__ rowpar,
                                                        const double* __restrict__ star_val,
                                                        const double* __restrict__ star_w, int64_t n_stars, int nb,
                                                        int np, double minq, double* __restrict__ work) {
    extern __shared__ double lds[];
    double* s_val = lds;                       // [nb][TILE]  this lane's star: magnitude
    double* s_w = s_val + nb * TILE;           // [nb][TILE]  1 / unc^2
    double* s_single = s_w + nb * TILE;        // [nb][TILE]  ln(1 - fB) + lnL_single at this j
    double* p_mag = s_single + nb * TILE;      // [nb][TILE]  binary magnitude of pair (j, k0 + i)
    double* p_lnq = p_mag + nb * TILE;         // [TILE]      powerlaw_lnpdf(m_k / m_j; gamma, minq, 1)
    double* p_eep = p_lnq + TILE;              // [TILE]      EEP of k0 + i
    int* p_ok = reinterpret_cast<int*>(p_eep + TILE);   // [TILE] m_k / m_j >= minq

    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t j = ld - 1 - b % ld;         // longest inner loops first
    const int64_t rest = b / ld;
    const int64_t tile = rest % tiles;
    const int64_t r = rest / tiles;
    int64_t n = n_valid[r];
    n = n < 0 ? 0 : (n > ld ? ld : n);
    if (j >= n) return;                         // uniform over the workgroup

    const int ncol = 3 + 2 * nb + np;
    const double* c = cols + r * ncol * ld;
    const double* c_eep = c;
    const double* c_mass = c + ld;
    const double* c_flux = c + 3 * ld;
    const double* c_mag = c + (3 + nb) * ld;
    const double* c_prop = c + (3 + 2 * nb) * ld;
    const double lnfB = rowpar[4 * r + 0], ln1mfB = rowpar[4 * r + 1];
    const double gamma = rowpar[4 * r + 2], lnCq = rowpar[4 * r + 3];
    const double m_j = c_mass[j];
    const double mass_term = c[2 * ld + j];

    const int64_t s = tile * TILE + lane;
    const bool active = s < n_stars;
    const int64_t sc = active ? s : 0;
    double prop = 0.0;                          // the reference's lnlike_prop[s, j]: 0 + term_0 + term_1 + ...
    for (int p = 0; p < np; ++p) {
        const double d = star_val[(nb + p) * n_stars + sc] - c_prop[p * ld + j];
        prop += -0.5 * d * d * star_w[(nb + p) * n_stars + sc];
    }
    for (int q = 0; q < nb; ++q) {
        const double v = star_val[q * n_stars + sc], w = star_w[q * n_stars + sc];
        const double rs = c_mag[q * ld + j] - v;
        s_val[q * TILE + lane] = v;
        s_w[q * TILE + lane] = w;
        s_single[q * TILE + lane] = ln1mfB + -0.5 * rs * rs * w;
    }

    double tot = 0.0, e_prev = 0.0, eep_prev = 0.0;
    for (int64_t k0 = 0; k0 <= j; k0 += TILE) {
        const int64_t k = k0 + lane;
        if (k <= j) {                           // the pair work of secondary k, once for all stars of the tile
            const double q = c_mass[k] / m_j;
            const int ok = !(q < minq);
            p_ok[lane] = ok;
            p_eep[lane] = c_eep[k];
            p_lnq[lane] = lnCq + gamma * log(q);
            for (int bb = 0; bb < nb; ++bb)
                p_mag[bb * TILE + lane] = -2.5 * log10(c_flux[bb * ld + j] + c_flux[bb * ld + k]);
        }
        __syncthreads();
        const int kend = (int)((j - k0 + 1) < TILE ? (j - k0 + 1) : TILE);
        for (int kk = 0; kk < kend; ++kk) {
            double e = 0.0;                     // exp(-inf) of a cell below the mass-ratio cut
            if (p_ok[kk]) {
                double phot = 0.0;
                for (int bb = 0; bb < nb; ++bb) {
                    const double rb = p_mag[bb * TILE + kk] - s_val[bb * TILE + lane];
                    phot += logaddexp(lnfB + -0.5 * rb * rb * s_w[bb * TILE + lane], s_single[bb * TILE + lane]);
                }
                e = exp(phot + mass_term + p_lnq[kk] + prop);   // not max-shifted: underflow is part of the semantics
            }
            const double eep_k = p_eep[kk];
            if (k0 + kk > 0) tot += 0.5 * (e_prev + e) * (eep_k - eep_prev);
            e_prev = e;
            eep_prev = eep_k;
        }
        __syncthreads();
    }
    if (active) work[(r * n_stars + s) * ld + j] = tot;
}

__global__ void __launch_bounds__(FINISH) k_cluster_finish(const double* __restrict__ cols, int64_t ld,
                                                           const int32_t* __restrict__ n_valid, int ncol,
                                                           int64_t n_stars, const double* __restrict__ work,
                                                           double* __restrict__ lnlike, double* __restrict__ lnlike_star) {
    __shared__ double s_sum[FINISH];
    __shared__ int s_zero[FINISH];
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x;
    int64_t n = n_valid[r];
    n = n < 0 ? 0 : (n > ld ? ld : n);
    const double* eep = cols + r * ncol * ld;
    double sum = 0.0;
    int zero = 0;
    for (int64_t s = t; s < n_stars; s += FINISH) {
        const double* I = work + (r * n_stars + s) * ld;
        double like = 0.0;                      // trapz(I_s, eep) in order of j
        for (int64_t j = 0; j + 1 < n; ++j) like = like + 0.5 * (I[j] + I[j + 1]) * (eep[j + 1] - eep[j]);
        const double l = log(like);
        zero |= like == 0.0;
        sum += l;
        if (lnlike_star) lnlike_star[r * n_stars + s] = l;
    }
    s_sum[t] = sum;
    s_zero[t] = zero;
    __syncthreads();
    for (int w = FINISH / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_sum[t] = s_sum[t] + s_sum[t + w];
            s_zero[t] |= s_zero[t + w];
        }
        __syncthreads();
    }
    if (t == 0) lnlike[r] = s_zero[0] ? -INFINITY : s_sum[0];
}

}  // namespace

extern "C" {

const char* iso_cluster_version(void) { return "isochrones_amd cluster 1"; }

const char* iso_cluster_last_error(void) { return g_err; }

int iso_cluster_lnlike(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                       const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                       double minq, double* work, double* lnlike, double* lnlike_star, void* stream) {
    g_err[0] = 0;
    if (n_rows < 0 || ld < 1 || n_stars < 1 || n_bands < 1 || n_bands > ISO_CLUSTER_MAX_BANDS || n_props < 0 ||
        n_props > ISO_CLUSTER_MAX_PROPS)
        return fail(ISO_CLUSTER_ERR_INVALID, "iso_cluster_lnlike: need ld >= 1, n_stars >= 1, 1..32 bands, 0..8 props");
    if (!cols || !n_valid || !rowpar || !star_val || !star_w || !work || !lnlike)
        return fail(ISO_CLUSTER_ERR_INVALID, "iso_cluster_lnlike: null pointer");
    if (n_rows == 0) return 0;
    const int64_t tiles = (n_stars + TILE - 1) / TILE;
    const int64_t blocks = n_rows * tiles * ld;
    if (blocks > INT32_MAX || n_rows > INT32_MAX)
        return fail(ISO_CLUSTER_ERR_INVALID, "iso_cluster_lnlike: too many rows in one call (split the batch)");
    const size_t lds = (size_t)(4 * n_bands + 2) * TILE * sizeof(double) + TILE * sizeof(int);
    // function attributes are per device: raise the limit before every large launch, on whichever device is current
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)k_cluster_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
        return fail(ISO_CLUSTER_ERR_HIP, "iso_cluster_lnlike: hipFuncSetAttribute failed");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cluster_pairs, dim3((unsigned)blocks), dim3(TILE), lds, st, cols, ld, tiles, n_valid, rowpar,
                       star_val, star_w, n_stars, n_bands, n_props, minq, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_CLUSTER_ERR_HIP, hipGetErrorString(e));
    hipLaunchKernelGGL(k_cluster_finish, dim3((unsigned)n_rows), dim3(FINISH), 0, st, cols, ld, n_valid,
                       3 + 2 * n_bands + n_props, n_stars, work, lnlike, lnlike_star);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_CLUSTER_ERR_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
