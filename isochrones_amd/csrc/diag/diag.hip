// Per-(ensemble, parameter) convergence diagnostics of a stored chain for gfx950: integrated autocorrelation time
// with Sokal's window, effective sample size and split R-hat.  See include/isochrones_amd_diag.h for the definition
// and the summation order, DESIGN.md section 13 for the mapping and the LDS budget.
//
// One kernel, one 256-thread workgroup (four wavefronts) per pair, float64:
//   k_diag_chain  walks the pair's [T, W] slab in tiles of WT walkers.  A tile is staged in LDS walker-major
//                 (row stride Tp = T | 1 doubles: odd, so that 16 consecutive walkers written at one t fall on 16
//                 different bank pairs), centred there in two passes, and its two split-chain means and variances
//                 are taken.  Then lanes own lags: an item is (256 consecutive lags, walker group g = w mod 4); lane l
//                 of the wavefront that has the item owns the lags 256 q + 64 j + l, j < 4, reads y[t] as a broadcast
//                 and y[t + k] at consecutive addresses, and carries A_g(k) across tiles through an LDS slot only it
//                 touches.  After the last tile the four groups are added, rho is formed, one wavefront reduces the
//                 split-chain sums and its first lane walks tau(M) up to the window.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "isochrones_amd_diag.h"
#include "../common/chain_view.h"
#include "../common/grid_cell.h"
#include "../common/wave_reduce.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int GROUPS = 4;                       // walker groups of the summation order (w mod 4)
constexpr int LANE_LAGS = 4;                    // lags a lane owns in one item
constexpr int ITEM_LAGS = 64 * LANE_LAGS;
constexpr int TILE_WALKERS = 16;                // walkers staged at once when they fit 64 KB
constexpr size_t LDS_PLAIN = 64 * 1024;         // what a launch gets without asking
constexpr size_t LDS_LIMIT = 160 * 1024;        // a CU's LDS
static_assert(ISO_DIAG_ROW_MAJOR == CHAIN_ROW_MAJOR && ISO_DIAG_PARAM_MAJOR == CHAIN_PARAM_MAJOR, "chain layouts");

struct Shape {
    ChainStrides st;
    int T, S, W, D, K;
    int WT, Tp;                                 // walkers per tile, LDS row stride
    double c;
};

// LDS of one workgroup in doubles: A_g(k) for four groups, mu_j and s_j^2 of the 2 W split chains, the tile's walker
// means and first values, the tile
size_t lds_doubles(int W, int K, int WT, int Tp) {
    return (size_t)GROUPS * (K + 1) + 4 * (size_t)W + 2 * (size_t)WT + (size_t)WT * Tp;
}

// the lag sums of one item over the walkers of group g in the tile; NJ = how many of the lane's lags are <= K in any lane
template <int NJ>
__device__ __forceinline__ void lag_item(const double* __restrict__ tile, double* __restrict__ Ag, int k0, int T,
                                         int K, int Tp, int w0, int wt, int g) {
    double acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = (k0 + 64 * j <= K) ? Ag[k0 + 64 * j] : 0.0;
    const int nt = (k0 <= K) ? T - k0 : 0;      // terms of the lane's smallest lag; the larger ones are masked below
    for (int wl = 0; wl < wt; ++wl) {
        if (((w0 + wl) & (GROUPS - 1)) != g) continue;          // wave-uniform
        const double* __restrict__ row = tile + (size_t)wl * Tp;
        for (int t = 0; t < nt; ++t) {
            const double a = row[t];                            // one address for the wavefront: a broadcast
            acc[0] = fma(a, row[t + k0], acc[0]);
#pragma unroll
            for (int j = 1; j < NJ; ++j) {
                // past the end of the series: read the row's last entry instead and add nothing (a lag beyond a binding
                // max_lag is summed and dropped)
                const int i = t + k0 + 64 * j;
                const double b = row[min(i, T - 1)];
                acc[j] = (i < T) ? fma(a, b, acc[j]) : acc[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (k0 + 64 * j <= K) Ag[k0 + 64 * j] = acc[j];
}

__global__ void __launch_bounds__(BLOCK) k_diag_chain(const double* __restrict__ chain, const Shape P,
                                                      double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int T = P.T, W = P.W, K = P.K, K1 = P.K + 1, WT = P.WT, Tp = P.Tp;
    double* __restrict__ A = lds;                               // [GROUPS][K1]
    double* __restrict__ mu = A + (size_t)GROUPS * K1;          // [2 W]
    double* __restrict__ s2 = mu + 2 * (size_t)W;               // [2 W]
    double* __restrict__ mean = s2 + 2 * (size_t)W;             // [WT]
    double* __restrict__ first = mean + WT;                     // [WT]
    double* __restrict__ tile = first + WT;                     // [WT][Tp]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x, s = pair / P.D, d = pair - s * P.D;
    const double* __restrict__ base = chain + (int64_t)d * P.st.st_d + (int64_t)s * W * P.st.st_w;
    const int n = T / 2;                                        // length of a split chain

    for (int i = tid; i < GROUPS * K1; i += BLOCK) A[i] = 0.0;
    const int nquads = (K1 + ITEM_LAGS - 1) / ITEM_LAGS;
    for (int w0 = 0; w0 < W; w0 += WT) {
        const int wt = min(WT, W - w0);
        __syncthreads();                                        // the previous tile's readers are done
        // stage: consecutive lanes read consecutive walkers of one step (coalesced in the parameter-major layout)
        for (int i = tid; i < wt * T; i += BLOCK) {
            const int t = i / wt, wl = i - t * wt;
            tile[(size_t)wl * Tp + t] = base[(int64_t)t * P.st.st_t + (int64_t)(w0 + wl) * P.st.st_w];
        }
        __syncthreads();
        for (int wl = tid; wl < wt; wl += BLOCK) {
            const double* row = tile + (size_t)wl * Tp;
            // the mean about the walker's first value: a walker that never moved centres to exact zeros
            const double x0 = row[0];
            double sum = 0.0;
            for (int t = 0; t < T; ++t) sum += row[t] - x0;
            first[wl] = x0;
            mean[wl] = sum / (double)T;
        }
        __syncthreads();
        for (int i = tid; i < wt * T; i += BLOCK) {
            const int wl = i / T, t = i - wl * T;
            tile[(size_t)wl * Tp + t] = (tile[(size_t)wl * Tp + t] - first[wl]) - mean[wl];
        }
        __syncthreads();
        // the two split chains of every walker, from the centred values: mean, then squares about that mean
        if (n >= 2) {
            for (int j = tid; j < 2 * wt; j += BLOCK) {
                const int wl = j >> 1;
                const double* h = tile + (size_t)wl * Tp + ((j & 1) ? T - n : 0);
                double sum = 0.0;
                for (int t = 0; t < n; ++t) sum += h[t];
                const double m = sum / (double)n;
                double ss = 0.0;
                for (int t = 0; t < n; ++t) {
                    const double e = h[t] - m;
                    ss = fma(e, e, ss);
                }
                mu[2 * (size_t)(w0 + wl) + (j & 1)] = (first[wl] + mean[wl]) + m;
                s2[2 * (size_t)(w0 + wl) + (j & 1)] = ss / (double)(n - 1);
            }
        }
        // lags: item = (quad of 256 lags, walker group); a wavefront takes every fourth item
        for (int item = wave; item < nquads * GROUPS; item += WAVES) {
            const int q = item % nquads, g = item / nquads;
            const int k0 = q * ITEM_LAGS + lane;
            double* __restrict__ Ag = A + (size_t)g * K1;
            const int nj = min(LANE_LAGS, (K1 - q * ITEM_LAGS + 63) / 64);      // wave-uniform
            switch (nj) {
            case 1: lag_item<1>(tile, Ag, k0, T, K, Tp, w0, wt, g); break;
            case 2: lag_item<2>(tile, Ag, k0, T, K, Tp, w0, wt, g); break;
            case 3: lag_item<3>(tile, Ag, k0, T, K, Tp, w0, wt, g); break;
            default: lag_item<4>(tile, Ag, k0, T, K, Tp, w0, wt, g); break;
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < K1; k += BLOCK) A[k] = ((A[k] + A[K1 + k]) + A[2 * K1 + k]) + A[3 * K1 + k];
    __syncthreads();
    const double a0 = A[0];
    for (int k = tid + 1; k < K1; k += BLOCK) A[k] = A[k] / a0; // rho(k), k >= 1 (slot 0 keeps A(0))
    __syncthreads();
    if (wave != 0) return;

    // split R-hat: fixed-order sums over the 2 W chains by one wavefront
    double rhat = qnan();
    if (n >= 2) {
        const int nc = 2 * W;
        double p = 0.0, q = 0.0;
        for (int j = lane; j < nc; j += 64) {
            p += s2[j];
            q += mu[j];
        }
        const double Wv = wave_sum(p) / (double)nc;
        const double grand = wave_sum(q) / (double)nc;
        double r = 0.0;
        for (int j = lane; j < nc; j += 64) {
            const double e = mu[j] - grand;
            r = fma(e, e, r);
        }
        const double B = (double)n * (wave_sum(r) / (double)(nc - 1));
        if (Wv != 0.0) rhat = sqrt((((double)(n - 1) / (double)n) * Wv + B / (double)n) / Wv);
    }
    if (lane != 0) return;

    double* __restrict__ o = out + (size_t)pair * ISO_DIAG_NOUT;
    if (a0 != a0) {                                             // a NaN in the slab reaches every centred value of its walker
        for (int i = 0; i < ISO_DIAG_NOUT; ++i) o[i] = qnan();
        return;
    }
    double tau = qnan(), window = (double)K, ok = 0.0;
    if (a0 != 0.0) {
        double acc = 0.0;                                       // sum of rho(1..M)
        int M = 0;
        for (;; ++M) {
            if (M > 0) acc += A[M];
            tau = 1.0 + 2.0 * acc;
            if ((double)M >= P.c * tau) {
                ok = 1.0;
                break;
            }
            if (M == K) break;
        }
        window = (double)M;
    }
    o[ISO_DIAG_TAU] = tau;
    o[ISO_DIAG_WINDOW] = window;
    o[ISO_DIAG_WINDOW_OK] = ok;
    o[ISO_DIAG_ESS] = (double)W * (double)T / tau;
    o[ISO_DIAG_RHAT] = rhat;
}

int check_args(const char* who, const double* chain, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
               double c, int32_t max_lag, const double* out) {
    const ChainShape s{layout, nsteps, n_ens, W, ndim};
    const char* why = nullptr;
    if (!chain || !out) why = "null pointer";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES, s))) {}
    else if (!(c > 0.0) || !isfinite(c)) why = "c must be finite and > 0";
    else if (max_lag < 1) why = "max_lag must be at least 1";
    else if ((int64_t)n_ens * ndim > INT32_MAX) why = "more than 2^31 - 1 (ensemble, parameter) pairs (split the batch)";
    else why = chain_shape_error(CHAIN_CHECK_ROWS, s);
    return why ? fail(ISO_DIAG_ERR_INVALID, who, why) : 0;
}

// the definition on one slab y[w][t] (row stride T), plain ascending loops
void host_pair(std::vector<double>& y, int T, int W, int K, double c, double* o) {
    const double nan = NAN;
    const int n = T / 2;
    std::vector<double> mean(W);
    for (int w = 0; w < W; ++w) {
        double* row = &y[(size_t)w * T];
        const double x0 = row[0];
        double sum = 0.0;
        for (int t = 0; t < T; ++t) sum += row[t] - x0;
        const double md = sum / (double)T;
        mean[w] = x0 + md;
        for (int t = 0; t < T; ++t) row[t] = (row[t] - x0) - md;
    }
    std::vector<double> A(K + 1, 0.0);
    for (int k = 0; k <= K; ++k) {
        double acc = 0.0;
        for (int w = 0; w < W; ++w) {
            const double* row = &y[(size_t)w * T];
            for (int t = 0; t + k < T; ++t) acc += row[t] * row[t + k];
        }
        A[k] = acc;
    }
    const double a0 = A[0];
    if (a0 != a0) {
        for (int i = 0; i < ISO_DIAG_NOUT; ++i) o[i] = nan;
        return;
    }
    double rhat = nan;
    if (n >= 2) {
        const int nc = 2 * W;
        std::vector<double> mu(nc), s2(nc);
        for (int j = 0; j < nc; ++j) {
            const double* h = &y[(size_t)(j >> 1) * T + ((j & 1) ? T - n : 0)];
            double sum = 0.0;
            for (int t = 0; t < n; ++t) sum += h[t];
            const double m = sum / (double)n;
            double ss = 0.0;
            for (int t = 0; t < n; ++t) ss += (h[t] - m) * (h[t] - m);
            mu[j] = mean[j >> 1] + m;
            s2[j] = ss / (double)(n - 1);
        }
        double p = 0.0, q = 0.0;
        for (int j = 0; j < nc; ++j) {
            p += s2[j];
            q += mu[j];
        }
        const double Wv = p / (double)nc, grand = q / (double)nc;
        double r = 0.0;
        for (int j = 0; j < nc; ++j) r += (mu[j] - grand) * (mu[j] - grand);
        const double B = (double)n * (r / (double)(nc - 1));
        if (Wv != 0.0) rhat = sqrt((((double)(n - 1) / (double)n) * Wv + B / (double)n) / Wv);
    }
    double tau = nan, window = (double)K, ok = 0.0;
    if (a0 != 0.0) {
        double acc = 0.0;
        int M = 0;
        for (;; ++M) {
            if (M > 0) acc += A[M] / a0;
            tau = 1.0 + 2.0 * acc;
            if ((double)M >= c * tau) {
                ok = 1.0;
                break;
            }
            if (M == K) break;
        }
        window = (double)M;
    }
    o[ISO_DIAG_TAU] = tau;
    o[ISO_DIAG_WINDOW] = window;
    o[ISO_DIAG_WINDOW_OK] = ok;
    o[ISO_DIAG_ESS] = (double)W * (double)T / tau;
    o[ISO_DIAG_RHAT] = rhat;
}

}  // namespace

extern "C" {

const char* iso_diag_version(void) { return "isochrones_amd diag 1"; }

const char* iso_diag_last_error(void) { return g_err; }

int iso_diag_chain(const double* chain, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim, double c,
                   int32_t max_lag, double* out, void* stream) {
    g_err[0] = 0;
    const int rc = check_args("iso_diag_chain", chain, layout, nsteps, n_ens, W, ndim, c, max_lag, out);
    if (rc) return rc;
    // the staging scheme holds at least one whole walker series in LDS
    if (nsteps > (int64_t)(LDS_LIMIT / sizeof(double)))
        return fail(ISO_DIAG_ERR_INVALID, "iso_diag_chain: nsteps too large for the kernel's LDS staging (thin the chain)");
    Shape P;
    P.st = chain_strides(layout, (int64_t)n_ens * W, ndim);
    P.T = (int)nsteps;
    P.S = n_ens;
    P.W = W;
    P.D = ndim;
    P.K = (int)((nsteps - 1 < max_lag) ? nsteps - 1 : max_lag);
    P.Tp = P.T | 1;
    P.c = c;
    // tile: up to TILE_WALKERS walkers inside the 64 KB every launch gets; when fewer than four (one per wavefront
    // group) fit there, up to four inside the CU's 160 KB
    int wt = W < TILE_WALKERS ? W : TILE_WALKERS;
    while (wt > 1 && lds_doubles(W, P.K, wt, P.Tp) * sizeof(double) > LDS_PLAIN) --wt;
    size_t bytes = lds_doubles(W, P.K, wt, P.Tp) * sizeof(double);
    if (bytes > LDS_PLAIN || (wt < GROUPS && wt < W)) {
        wt = W < GROUPS ? W : GROUPS;
        while (wt > 1 && lds_doubles(W, P.K, wt, P.Tp) * sizeof(double) > LDS_LIMIT) --wt;
        bytes = lds_doubles(W, P.K, wt, P.Tp) * sizeof(double);
    }
    if (bytes > LDS_LIMIT)
        return fail(ISO_DIAG_ERR_INVALID,
                    "iso_diag_chain: 8 (4 (K + 1) + 4 W + (T | 1) + 2) bytes of LDS exceed a CU's 160 KB (thin the chain, "
                    "lower max_lag or split the walkers)");
    P.WT = wt;
    // function attributes are per device: raise the limit before every large launch, on whichever device is current
    if (bytes > LDS_PLAIN &&
        hipFuncSetAttribute((const void*)k_diag_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT) != hipSuccess)
        return fail(ISO_DIAG_ERR_HIP, "iso_diag_chain: hipFuncSetAttribute failed");
    hipLaunchKernelGGL(k_diag_chain, dim3((unsigned)(n_ens * ndim)), dim3(BLOCK), bytes, (hipStream_t)stream, chain, P, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_DIAG_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_diag_chain_host(const double* chain, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                        double c, int32_t max_lag, double* out, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_args("iso_diag_chain_host", chain, layout, nsteps, n_ens, W, ndim, c, max_lag, out);
    if (rc) return rc;
    if (nsteps > INT32_MAX) return fail(ISO_DIAG_ERR_INVALID, "iso_diag_chain_host: nsteps beyond 2^31 - 1");
    const ChainStrides st = chain_strides(layout, (int64_t)n_ens * W, ndim);
    const int T = (int)nsteps;
    const int K = (int)((nsteps - 1 < max_lag) ? nsteps - 1 : max_lag);
    std::vector<double> y((size_t)W * T);
    for (int s = 0; s < n_ens; ++s)
        for (int d = 0; d < ndim; ++d) {
            const double* base = chain + (int64_t)d * st.st_d + (int64_t)s * W * st.st_w;
            for (int w = 0; w < W; ++w)
                for (int t = 0; t < T; ++t) y[(size_t)w * T + t] = base[(int64_t)t * st.st_t + (int64_t)w * st.st_w];
            host_pair(y, T, W, K, c, out + ((size_t)s * ndim + d) * ISO_DIAG_NOUT);
        }
    return 0;
}

}  // extern "C"
