// Per-star moments of the star-cluster likelihood's integrand (StarClusterModel.star_moments) for gfx950: over the
// (primary EEP j, secondary EEP k <= j) grid of every member star, six inner trapezoids instead of the likelihood's one,
// and from them ln like_s and eleven moments per (row, star).  See include/isochrones_amd_members.h for the definition
// and the summation order, DESIGN.md section 26 for the mapping and the resources.
//
// The cell arithmetic is a restatement of csrc/cluster/cluster.hip's (that file is pinned): ln_like here is the same bits
// as its lnlike_star, which is what holds the two together (tests/test_gpu_members.py).
//
// Two kernels, both with a fixed order of every sum, so that a (row, star) result does not depend on its launch:
//   k_members_pairs   k_cluster_pairs's plan: one 64-lane workgroup per (row, tile of 64 stars, primary EEP j), longest j
//                     first.  The star-independent work of a pair (j, k) - the binary magnitude of each band, q, the cut
//                     and ln q's term - is computed once per pair by one lane for 64 secondaries at a time and read by all
//                     64 stars from LDS (every lane reads the same address: a broadcast, no bank conflict).  Each lane
//                     walks k = 0 .. j in order with six running trapezoids.  The two further exponentials of a cell are
//                     taken only where e != 0: most cells of most stars underflow, and a wavefront whose 64 stars all do
//                     skips them.
//   k_members_finish  one lane per (row, star): the outer trapezoids in order of j, the log and the eleven quotients.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "isochrones_amd_members.h"
#include "../common/last_error.h"

namespace {

constexpr int TILE = 64;          // stars per workgroup = lanes of one wave
constexpr int FINISH = 256;       // threads of a finishing workgroup
constexpr int NI = ISO_MEMBERS_NINNER;
constexpr int NM = ISO_MEMBERS_NMOM;

// the likelihood's logaddexp (cluster.hip): hi + log(exp(lo - hi) + 1)
__host__ __device__ __forceinline__ double logaddexp(double a, double b) {
    const bool second = b > a;
    const double hi = second ? b : a;
    const double lo = second ? a : b;
    return hi + log(exp(lo - hi) + 1.0);
}

// the six products g * e of one cell whose e is not 0, in the order of `work`
__host__ __device__ __forceinline__ void cell_products(double e, double q, double suma, double sumc, double phot,
                                                       double* x) {
    const double pair = exp(suma - phot);
    const double single = exp(sumc - phot);
    x[0] = e;
    x[1] = q * e;
    x[2] = (q * q) * e;
    x[3] = pair * e;
    x[4] = single * e;
    x[5] = (q * pair) * e;
}

// the outer trapezoids of one (row, star), the log and the quotients: W is the star's [6][ld] block of `work`
__host__ __device__ __forceinline__ void finish_star(const double* eep, const double* mass, const double* W, int64_t ld,
                                                     int64_t n, double* ln_like, double* mom) {
    double like = 0.0;
    double acc[NM];
    for (int m = 0; m < NM; ++m) acc[m] = 0.0;
    double xp[NM];
    double Ip = 0.0, ep = 0.0;
    for (int64_t j = 0; j < n; ++j) {
        const double ej = eep[j], mj = mass[j];
        const double I0 = W[j], I1 = W[ld + j], I2 = W[2 * ld + j];
        double x[NM];
        x[0] = ej * I0;
        x[1] = (ej * ej) * I0;
        x[2] = mj * I0;
        x[3] = (mj * mj) * I0;
        x[4] = I1;
        x[5] = I2;
        x[6] = mj * I1;
        x[7] = (mj * mj) * I2;
        x[8] = W[3 * ld + j];
        x[9] = W[4 * ld + j];
        x[10] = W[5 * ld + j];
        if (j > 0) {
            const double d = ej - ep;
            like = like + 0.5 * (Ip + I0) * d;      // k_cluster_finish's expression and order
            for (int m = 0; m < NM; ++m) acc[m] = acc[m] + 0.5 * (xp[m] + x[m]) * d;
        }
        for (int m = 0; m < NM; ++m) xp[m] = x[m];
        Ip = I0;
        ep = ej;
    }
    *ln_like = log(like);
    const bool dead = like == 0.0;
    for (int m = 0; m < NM; ++m) mom[m] = dead ? NAN : acc[m] / like;
}

__global__ void __launch_bounds__(TILE) k_members_pairs(const double* __restrict__ cols, int64_t ld, int64_t tiles,
                                                        const int32_t* __restrict__ n_valid,
                                                        const double* __restrict__ rowpar,
                                                        const double* __restrict__ star_val,
                                                        const double* __restrict__ star_w, int64_t n_stars, int nb,
                                                        int np, double minq, double* __restrict__ work) {
    extern __shared__ double lds[];
    double* s_val = lds;                       // [nb][TILE]  this lane's star: magnitude
    double* s_w = s_val + nb * TILE;           // [nb][TILE]  1 / unc^2
    double* s_single = s_w + nb * TILE;        // [nb][TILE]  c_b = ln(1 - fB) + lnL_single at this j
    double* p_mag = s_single + nb * TILE;      // [nb][TILE]  binary magnitude of pair (j, k0 + i)
    double* p_lnq = p_mag + nb * TILE;         // [TILE]      powerlaw_lnpdf(m_k / m_j; gamma, minq, 1)
    double* p_q = p_lnq + TILE;                // [TILE]      m_k / m_j
    double* p_eep = p_q + TILE;                // [TILE]      EEP of k0 + i
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
    double prop = 0.0;
    for (int p = 0; p < np; ++p) {
        const double d = star_val[(nb + p) * n_stars + sc] - c_prop[p * ld + j];
        prop += -0.5 * d * d * star_w[(nb + p) * n_stars + sc];
    }
    double sumc = 0.0;                          // sum_b c_b of (s, j)
    for (int q = 0; q < nb; ++q) {
        const double v = star_val[q * n_stars + sc], w = star_w[q * n_stars + sc];
        const double rs = c_mag[q * ld + j] - v;
        const double cb = ln1mfB + -0.5 * rs * rs * w;
        s_val[q * TILE + lane] = v;
        s_w[q * TILE + lane] = w;
        s_single[q * TILE + lane] = cb;
        sumc += cb;
    }

    double tot[NI], x_prev[NI];
#pragma unroll
    for (int g = 0; g < NI; ++g) tot[g] = x_prev[g] = 0.0;
    double eep_prev = 0.0;
    for (int64_t k0 = 0; k0 <= j; k0 += TILE) {
        const int64_t k = k0 + lane;
        if (k <= j) {                           // the pair work of secondary k, once for all stars of the tile
            const double q = c_mass[k] / m_j;
            const int ok = !(q < minq);
            p_ok[lane] = ok;
            p_eep[lane] = c_eep[k];
            p_q[lane] = q;
            p_lnq[lane] = lnCq + gamma * log(q);
            for (int bb = 0; bb < nb; ++bb)
                p_mag[bb * TILE + lane] = -2.5 * log10(c_flux[bb * ld + j] + c_flux[bb * ld + k]);
        }
        __syncthreads();
        const int kend = (int)((j - k0 + 1) < TILE ? (j - k0 + 1) : TILE);
        for (int kk = 0; kk < kend; ++kk) {
            double e = 0.0, phot = 0.0, suma = 0.0;
            if (p_ok[kk]) {
                for (int bb = 0; bb < nb; ++bb) {
                    const double rb = p_mag[bb * TILE + kk] - s_val[bb * TILE + lane];
                    const double ab = lnfB + -0.5 * rb * rb * s_w[bb * TILE + lane];
                    phot += logaddexp(ab, s_single[bb * TILE + lane]);
                    suma += ab;
                }
                e = exp(phot + mass_term + p_lnq[kk] + prop);   // not max-shifted: underflow is part of the semantics
            }
            double x[NI];
#pragma unroll
            for (int g = 0; g < NI; ++g) x[g] = 0.0;
            if (!(e == 0.0)) cell_products(e, p_q[kk], suma, sumc, phot, x);   // a NaN goes through
            const double eep_k = p_eep[kk];
            if (k0 + kk > 0) {
                const double d = eep_k - eep_prev;
#pragma unroll
                for (int g = 0; g < NI; ++g) tot[g] += 0.5 * (x_prev[g] + x[g]) * d;
            }
#pragma unroll
            for (int g = 0; g < NI; ++g) x_prev[g] = x[g];
            eep_prev = eep_k;
        }
        __syncthreads();
    }
    if (active) {
        double* w = work + (r * n_stars + s) * NI * ld + j;
#pragma unroll
        for (int g = 0; g < NI; ++g) w[g * ld] = tot[g];
    }
}

__global__ void __launch_bounds__(FINISH) k_members_finish(const double* __restrict__ cols, int64_t ld,
                                                           const int32_t* __restrict__ n_valid, int ncol,
                                                           int64_t n_stars, int64_t total,
                                                           const double* __restrict__ work,
                                                           double* __restrict__ ln_like, double* __restrict__ moments) {
    const int64_t i = (int64_t)blockIdx.x * FINISH + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / n_stars;
    int64_t n = n_valid[r];
    n = n < 0 ? 0 : (n > ld ? ld : n);
    const double* c = cols + r * ncol * ld;
    double l, mom[NM];
    finish_star(c, c + ld, work + i * NI * ld, ld, n, &l, mom);
    ln_like[i] = l;
#pragma unroll
    for (int m = 0; m < NM; ++m) moments[i * NM + m] = mom[m];
}

int check_args(const char* who, const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid,
               const double* rowpar, const double* star_val, const double* star_w, int64_t n_stars, int n_bands,
               int n_props, const double* work, const double* ln_like, const double* moments) {
    const char* why = nullptr;
    if (n_rows < 0 || ld < 1 || n_stars < 1 || n_bands < 1 || n_bands > ISO_MEMBERS_MAX_BANDS || n_props < 0 ||
        n_props > ISO_MEMBERS_MAX_PROPS)
        why = "need n_rows >= 0, ld >= 1, n_stars >= 1, 1..32 bands, 0..8 props";
    else if (!cols || !n_valid || !rowpar || !star_val || !star_w || !work || !ln_like || !moments)
        why = "null pointer";
    return why ? fail(ISO_MEMBERS_ERR_INVALID, who, why) : 0;
}

}  // namespace

extern "C" {

const char* iso_members_version(void) { return "isochrones_amd members 1"; }

const char* iso_members_last_error(void) { return g_err; }

int iso_members_moments(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                        const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                        double minq, double* work, double* ln_like, double* moments, void* stream) {
    g_err[0] = 0;
    const char* who = "iso_members_moments";
    const int rc = check_args(who, cols, ld, n_rows, n_valid, rowpar, star_val, star_w, n_stars, n_bands, n_props, work,
                              ln_like, moments);
    if (rc) return rc;
    if (n_rows == 0) return 0;
    const int64_t tiles = (n_stars + TILE - 1) / TILE;
    // in floating point first: the product of three int64 can wrap
    if ((double)n_rows * (double)tiles * (double)ld > (double)INT32_MAX || n_rows > INT32_MAX ||
        (double)n_rows * (double)n_stars > (double)INT32_MAX * FINISH)
        return fail(ISO_MEMBERS_ERR_INVALID, who, "too many rows in one call (split the batch)");
    const int64_t blocks = n_rows * tiles * ld;
    const size_t lds = (size_t)(4 * n_bands + 3) * TILE * sizeof(double) + TILE * sizeof(int);
    // function attributes are per device: raise the limit before every large launch, on whichever device is current
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)k_members_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
        return fail(ISO_MEMBERS_ERR_HIP, who, "hipFuncSetAttribute failed");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_members_pairs, dim3((unsigned)blocks), dim3(TILE), lds, st, cols, ld, tiles, n_valid, rowpar,
                       star_val, star_w, n_stars, n_bands, n_props, minq, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_MEMBERS_ERR_HIP, who, hipGetErrorString(e));
    const int64_t total = n_rows * n_stars;
    hipLaunchKernelGGL(k_members_finish, dim3((unsigned)((total + FINISH - 1) / FINISH)), dim3(FINISH), 0, st, cols, ld,
                       n_valid, 3 + 2 * n_bands + n_props, n_stars, total, work, ln_like, moments);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_MEMBERS_ERR_HIP, who, hipGetErrorString(e));
    return 0;
}

int iso_members_moments_host(const double* cols, int64_t ld, int64_t n_rows, const int32_t* n_valid, const double* rowpar,
                             const double* star_val, const double* star_w, int64_t n_stars, int n_bands, int n_props,
                             double minq, double* work, double* ln_like, double* moments, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_args("iso_members_moments_host", cols, ld, n_rows, n_valid, rowpar, star_val, star_w, n_stars,
                              n_bands, n_props, work, ln_like, moments);
    if (rc) return rc;
    const int nb = n_bands, np = n_props;
    const int64_t ncol = 3 + 2 * nb + np;
    std::vector<double> p_mag((size_t)nb * ld), p_lnq(ld), p_q(ld), cb(nb);
    std::vector<int> p_ok(ld);
    for (int64_t r = 0; r < n_rows; ++r) {
        int64_t n = n_valid[r];
        n = n < 0 ? 0 : (n > ld ? ld : n);
        const double* c = cols + r * ncol * ld;
        const double* c_eep = c;
        const double* c_mass = c + ld;
        const double* c_flux = c + 3 * ld;
        const double* c_mag = c + (3 + nb) * ld;
        const double* c_prop = c + (3 + 2 * nb) * ld;
        const double lnfB = rowpar[4 * r + 0], ln1mfB = rowpar[4 * r + 1];
        const double gamma = rowpar[4 * r + 2], lnCq = rowpar[4 * r + 3];
        for (int64_t j = 0; j < n; ++j) {
            const double m_j = c_mass[j];
            const double mass_term = c[2 * ld + j];
            for (int64_t k = 0; k <= j; ++k) {
                const double q = c_mass[k] / m_j;
                p_ok[k] = !(q < minq);
                p_q[k] = q;
                p_lnq[k] = lnCq + gamma * log(q);
                for (int bb = 0; bb < nb; ++bb)
                    p_mag[(size_t)bb * ld + k] = -2.5 * log10(c_flux[bb * ld + j] + c_flux[bb * ld + k]);
            }
            for (int64_t s = 0; s < n_stars; ++s) {
                double prop = 0.0;
                for (int p = 0; p < np; ++p) {
                    const double d = star_val[(nb + p) * n_stars + s] - c_prop[p * ld + j];
                    prop += -0.5 * d * d * star_w[(nb + p) * n_stars + s];
                }
                double sumc = 0.0;
                for (int bb = 0; bb < nb; ++bb) {
                    const double rs = c_mag[bb * ld + j] - star_val[bb * n_stars + s];
                    cb[bb] = ln1mfB + -0.5 * rs * rs * star_w[bb * n_stars + s];
                    sumc += cb[bb];
                }
                double tot[NI], x_prev[NI];
                for (int g = 0; g < NI; ++g) tot[g] = x_prev[g] = 0.0;
                double eep_prev = 0.0;
                for (int64_t k = 0; k <= j; ++k) {
                    double e = 0.0, phot = 0.0, suma = 0.0;
                    if (p_ok[k]) {
                        for (int bb = 0; bb < nb; ++bb) {
                            const double rb = p_mag[(size_t)bb * ld + k] - star_val[bb * n_stars + s];
                            const double ab = lnfB + -0.5 * rb * rb * star_w[bb * n_stars + s];
                            phot += logaddexp(ab, cb[bb]);
                            suma += ab;
                        }
                        e = exp(phot + mass_term + p_lnq[k] + prop);
                    }
                    double x[NI];
                    for (int g = 0; g < NI; ++g) x[g] = 0.0;
                    if (!(e == 0.0)) cell_products(e, p_q[k], suma, sumc, phot, x);
                    const double eep_k = c_eep[k];
                    if (k > 0) {
                        const double d = eep_k - eep_prev;
                        for (int g = 0; g < NI; ++g) tot[g] += 0.5 * (x_prev[g] + x[g]) * d;
                    }
                    for (int g = 0; g < NI; ++g) x_prev[g] = x[g];
                    eep_prev = eep_k;
                }
                double* w = work + (r * n_stars + s) * NI * ld + j;
                for (int g = 0; g < NI; ++g) w[g * ld] = tot[g];
            }
        }
        for (int64_t s = 0; s < n_stars; ++s) {
            const int64_t i = r * n_stars + s;
            finish_star(c_eep, c_mass, work + i * NI * ld, ld, n, ln_like + i, moments + i * NM);
        }
    }
    return 0;
}

}  // extern "C"
