// The hierarchical (population) likelihood of a catalog from the stored chains of its stars for gfx950: per (hyper row,
// star) the log of the mean importance weight of the star's samples under the row's population density, and its effective
// sample size; per row their total.  See include/isochrones_amd_hier.h for the definition and the summation order,
// DESIGN.md section 17 for the mapping and the resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64:
//   k_hier_stars  one workgroup per (star, tile of ROW_TILE hyper rows).  The interim records, the tile's records and the
//                 column descriptors are staged in LDS (every lane reads the same address: a broadcast).  Lanes run
//                 along the sample axis m = t * W + w, so consecutive lanes read consecutive walkers of the
//                 parameter-major storage.  The star's samples are streamed twice per tile (maximum, then sums), never
//                 once per row; per sample and column x, ln x (only where a record of the column needs it), the interim
//                 term and the bad-sample test are computed once and serve the tile's rows, whose accumulators stay in
//                 registers.
//   k_hier_total  one workgroup per row: L and min_ess over the unmasked stars in a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "isochrones_amd_hier.h"
#include "../common/chain_view.h"
#include "../common/grid_cell.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int RT = ISO_HIER_ROW_TILE;
constexpr int MAXQ = ISO_HIER_MAX_COLS;
constexpr double LN10 = 2.302585092994046;
static_assert(ISO_HIER_ROW_MAJOR == CHAIN_ROW_MAJOR && ISO_HIER_PARAM_MAJOR == CHAIN_PARAM_MAJOR, "chain layouts");
static_assert(sizeof(iso_hier_record) == 72, "record layout");

typedef iso_hier_record Rec;

__host__ __device__ inline double neg_inf() {
    union { uint64_t u; double d; } x;
    x.u = 0xfff0000000000000ULL;
    return x.d;
}

__host__ __device__ inline bool needs_log(int kind) {
    return kind == ISO_HIER_POWERLAW || kind == ISO_HIER_LOGNORMAL || kind == ISO_HIER_CHABRIER;
}

// FehPrior._shape
__host__ __device__ inline double feh_shape(double halo_fraction, bool local, double feh) {
    double disk;
    if (local) {
        const double u = feh - 0.016, v = feh + 0.15;
        disk = 1.0 / 2.5066282746310007 *
               (0.8 / 0.15 * exp(-0.5 * (u * u) / (0.15 * 0.15)) + 0.2 / 0.22 * exp(-0.5 * (v * v) / (0.22 * 0.22)));
    } else {
        const double u = feh + 0.3;
        disk = 0.3989422804014327 / 0.3 * exp(-0.5 * (u * u) / (0.3 * 0.3));
    }
    const double h = feh + 1.5;
    const double halo = 0.99735570100358173 * exp(-0.5 * (h * h) / (0.4 * 0.4));   // 1 / sqrt(2 pi 0.4^2)
    return halo_fraction * halo + (1 - halo_fraction) * disk;
}

// ln f(x; R) of the header; lx = ln x where needs_log(R.kind), unused otherwise
__host__ __device__ inline double lnf(const Rec& R, double x, double lx) {
    const bool out = x < R.lo || x > R.hi;
    switch (R.kind) {
    case ISO_HIER_FLAT: return out ? neg_inf() : R.p[0];
    case ISO_HIER_FLATLOG: return out ? neg_inf() : R.p[0] + x * LN10;
    case ISO_HIER_POWERLAW: return out ? neg_inf() : R.p[0] + R.p[1] * lx;
    case ISO_HIER_GAUSS:
    case ISO_HIER_TRUNCGAUSS: {
        const double z = (x - R.p[0]) * R.p[3];
        return out ? neg_inf() : -(z * z) / 2.0 + R.p[2];
    }
    case ISO_HIER_LOGNORMAL: {
        const double l = lx - R.p[0], v = l * R.p[3];
        return (R.p[2] - l) - 0.5 * (v * v);
    }
    case ISO_HIER_CHABRIER: {
        if (x < R.p[5]) {
            const double l = lx - R.p[0], v = l * R.p[1];
            return (R.p[2] - l) - 0.5 * (v * v);
        }
        return out ? neg_inf() : R.p[4] + R.p[3] * lx;
    }
    case ISO_HIER_FEH: return out ? neg_inf() : log(feh_shape(R.p[0], R.p[2] != 0.0, x) / R.p[1]);
    }
    return qnan();
}

// one column as the kernel reads it: sample (t, w) of ensemble s at base[t * st_t + ((s - first) * W + w) * st_w]
struct DevCol {
    const double* base;                         // the storage's first double of the column
    int64_t st_t, st_w;
    int32_t first, pad;
};

struct Args {
    DevCol col[MAXQ];
    const Rec* interim;
    const Rec* rows;
    const int32_t* mask;
    double* ell;
    double* ess;
    int32_t* n_bad;
    int32_t Q, T, W, H, n_ens, ens_begin, ntiles, pad;
};

// xor butterflies over the 64 lanes, distances 32 .. 1: every lane ends with the same value, in a fixed order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ void __launch_bounds__(BLOCK) k_hier_stars(const Args A) {
    __shared__ Rec s_rec[(RT + 1) * MAXQ];      // [0][q]: interim; [1 + j][q]: row j of the tile
    __shared__ DevCol s_col[MAXQ];
    __shared__ double s_red[2 * RT * WAVES];
    __shared__ int s_bad[WAVES];
    __shared__ int s_log[MAXQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = A.Q, W = A.W, H = A.H;
    const int star = (int)(blockIdx.x / (unsigned)A.ntiles), tile = (int)(blockIdx.x - (unsigned)star * A.ntiles);
    const int s = A.ens_begin + star, h0 = tile * RT;
    const size_t ld = (size_t)A.n_ens;

    if (A.mask && A.mask[s] == 0) {             // workgroup-uniform
        if (tid < RT && h0 + tid < H) {
            A.ell[(size_t)(h0 + tid) * ld + s] = qnan();
            A.ess[(size_t)(h0 + tid) * ld + s] = qnan();
        }
        if (tile == 0 && tid == 0) A.n_bad[s] = 0;
        return;
    }

    // stage the records as 32-bit words; a tile that reaches past H repeats the last row (computed, never written)
    {
        constexpr int RW = (int)(sizeof(Rec) / 4);
        uint32_t* dst = (uint32_t*)s_rec;
        const uint32_t* src0 = (const uint32_t*)A.interim;
        for (int i = tid; i < Q * RW; i += BLOCK) dst[i] = src0[i];
        for (int i = tid; i < RT * Q * RW; i += BLOCK) {
            const int j = i / (Q * RW), k = i - j * (Q * RW);
            const int h = min(h0 + j, H - 1);
            dst[(1 + j) * MAXQ * RW + k] = ((const uint32_t*)(A.rows + (size_t)h * Q))[k];
        }
        if (tid == 0) {
            s_col[0] = A.col[0];
            s_col[1] = A.col[1];
            s_col[2] = A.col[2];
            s_col[3] = A.col[3];
        }
    }
    __syncthreads();
    if (tid < Q) {
        int need = 0;
        for (int j = 0; j <= RT; ++j) need |= needs_log(s_rec[j * MAXQ + tid].kind) ? 1 : 0;
        s_log[tid] = need;
    }
    __syncthreads();

    const int M = A.T * W;
    double mx[RT], s1[RT], s2[RT];
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        mx[j] = neg_inf();
        s1[j] = 0.0;
        s2[j] = 0.0;
    }
    int nbad = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int m = tid; m < M; m += BLOCK) {
            const int t = m / W, w = m - t * W;
            double r[RT];
#pragma unroll
            for (int j = 0; j < RT; ++j) r[j] = 0.0;
            bool good = true;
            for (int q = 0; q < Q; ++q) {
                const DevCol c = s_col[q];
                const double x = c.base[(int64_t)t * c.st_t + ((int64_t)(s - c.first) * W + w) * c.st_w];
                const double lx = s_log[q] ? log(x) : 0.0;      // workgroup-uniform choice
                const double l0 = lnf(s_rec[q], x, lx);
                good = good && x == x && l0 == l0 && l0 != neg_inf();
#pragma unroll
                for (int j = 0; j < RT; ++j) {
                    double lf = lnf(s_rec[(1 + j) * MAXQ + q], x, lx);
                    lf = (lf == lf) ? lf : neg_inf();
                    const double d = lf - l0;
                    r[j] = (q == 0) ? d : r[j] + d;
                }
            }
            if (pass == 0) {
                nbad += good ? 0 : 1;
#pragma unroll
                for (int j = 0; j < RT; ++j) mx[j] = good ? fmax(mx[j], r[j]) : mx[j];
            } else {
#pragma unroll
                for (int j = 0; j < RT; ++j) {
                    const double wgt = good ? exp(r[j] - mx[j]) : 0.0;
                    s1[j] += wgt;
                    s2[j] += wgt * wgt;
                }
            }
        }
        if (pass == 0) {
            // the maximum over the workgroup; a row with no support anywhere keeps -inf in s_red and subtracts 0
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                const double v = wave_max(mx[j]);
                if (lane == 0) s_red[j * WAVES + wave] = v;
            }
            const int b = wave_sum_int(nbad);
            if (lane == 0) s_bad[wave] = b;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                const double v = fmax(fmax(s_red[j * WAVES], s_red[j * WAVES + 1]),
                                      fmax(s_red[j * WAVES + 2], s_red[j * WAVES + 3]));
                mx[j] = (v == neg_inf()) ? 0.0 : v;
            }
            if (tile == 0 && tid == 0) A.n_bad[s] = ((s_bad[0] + s_bad[1]) + s_bad[2]) + s_bad[3];
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        const double a = wave_sum(s1[j]), b = wave_sum(s2[j]);
        if (lane == 0) {
            s_red[j * WAVES + wave] = a;
            s_red[(RT + j) * WAVES + wave] = b;
        }
    }
    __syncthreads();
    if (tid < RT && h0 + tid < H) {
        const int j = tid;
        const double S1 = ((s_red[j * WAVES] + s_red[j * WAVES + 1]) + s_red[j * WAVES + 2]) + s_red[j * WAVES + 3];
        const double S2 = ((s_red[(RT + j) * WAVES] + s_red[(RT + j) * WAVES + 1]) + s_red[(RT + j) * WAVES + 2]) +
                          s_red[(RT + j) * WAVES + 3];
        // mx[j] is the same in every lane; lane j needs row j's: take it through LDS order, not a dynamic register index
        double mxj = 0.0;
#pragma unroll
        for (int k = 0; k < RT; ++k) mxj = (k == j) ? mx[k] : mxj;
        const bool none = !(S1 > 0.0);
        A.ell[(size_t)(h0 + j) * ld + s] = none ? neg_inf() : (mxj + log(S1)) - log((double)M);
        A.ess[(size_t)(h0 + j) * ld + s] = none ? 0.0 : (S1 * S1) / S2;
    }
}

__global__ void __launch_bounds__(BLOCK) k_hier_total(const double* __restrict__ ell, const double* __restrict__ ess,
                                                      const int32_t* __restrict__ mask, int n_ens,
                                                      double* __restrict__ L, double* __restrict__ min_ess) {
    __shared__ double s_red[2 * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)blockIdx.x * (size_t)n_ens;
    double sum = 0.0, mn = HUGE_VAL;
    for (int s = tid; s < n_ens; s += BLOCK) {
        if (mask && mask[s] == 0) continue;
        sum += ell[row + s];
        mn = fmin(mn, ess[row + s]);
    }
    const double a = wave_sum(sum), b = wave_min(mn);
    if (lane == 0) {
        s_red[wave] = a;
        s_red[WAVES + wave] = b;
    }
    __syncthreads();
    if (tid == 0) {
        L[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        min_ess[blockIdx.x] = fmin(fmin(s_red[WAVES], s_red[WAVES + 1]), fmin(s_red[WAVES + 2], s_red[WAVES + 3]));
    }
}

int check_args(const char* who, const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens,
               int32_t W, int32_t ens_begin, int32_t n_ens_out, const Rec* interim, const Rec* rows, int32_t H,
               const double* ell, const double* ess, const int32_t* n_bad, const double* L, const double* min_ess) {
    ChainShape s{layout, nsteps, n_ens, W, 1};
    s.ens_begin = ens_begin;
    s.n_ens_out = n_ens_out;
    const char* why = nullptr;
    if (!columns || !interim || !rows || !ell || !ess || !n_bad) why = "null pointer";
    else if ((L == nullptr) != (min_ess == nullptr)) why = "L and min_ess go together (both or neither)";
    else if (Q < 1 || Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if (H < 1) why = "H must be at least 1";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (nsteps * (int64_t)W > INT32_MAX) why = "more than 2^31 - 1 samples per star (thin the chain)";
    else if ((int64_t)n_ens_out * ((H + RT - 1) / RT) > INT32_MAX) why = "more than 2^31 - 1 (star, row tile) pairs (split the call)";
    else
        for (int q = 0; q < Q && !why; ++q) {
            const iso_hier_column& c = columns[q];
            if (!c.base) why = "null column storage";
            else if (c.ncols < 1 || c.col < 0 || c.col >= c.ncols) why = "a column index is outside [0, ncols)";
            else if (c.n_ens < 1 || (int64_t)c.n_ens * W > INT32_MAX) why = "a column storage's n_ens must be at least 1 and n_ens * W below 2^31";
            else if (c.first < 0 || c.first > ens_begin || (int64_t)ens_begin + n_ens_out > (int64_t)c.first + c.n_ens)
                why = "a column storage does not hold the ensembles [ens_begin, ens_begin + n_ens_out)";
        }
    return why ? fail(ISO_HIER_ERR_INVALID, who, why) : 0;
}

DevCol dev_col(const iso_hier_column& c, int layout, int32_t W) {
    const ChainStrides st = chain_strides(layout, (int64_t)c.n_ens * W, c.ncols);
    return DevCol{c.base + (int64_t)c.col * st.st_d, st.st_t, st.st_w, c.first, 0};
}

}  // namespace

extern "C" {

const char* iso_hier_version(void) { return "isochrones_amd hier 1"; }

const char* iso_hier_last_error(void) { return g_err; }

int iso_hier_lnlike(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                    int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* rows,
                    int32_t H, const int32_t* mask, double* ell, double* ess, int32_t* n_bad, double* L, double* min_ess,
                    void* stream) {
    g_err[0] = 0;
    const int rc = check_args("iso_hier_lnlike", columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, rows,
                              H, ell, ess, n_bad, L, min_ess);
    if (rc) return rc;
    Args A;
    for (int q = 0; q < MAXQ; ++q) A.col[q] = dev_col(columns[q < Q ? q : 0], layout, W);
    A.interim = interim;
    A.rows = rows;
    A.mask = mask;
    A.ell = ell;
    A.ess = ess;
    A.n_bad = n_bad;
    A.Q = Q;
    A.T = (int32_t)nsteps;
    A.W = W;
    A.H = H;
    A.n_ens = n_ens;
    A.ens_begin = ens_begin;
    A.ntiles = (H + RT - 1) / RT;
    A.pad = 0;
    hipLaunchKernelGGL(k_hier_stars, dim3((unsigned)n_ens_out * (unsigned)A.ntiles), dim3(BLOCK), 0, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_HIER_ERR_HIP, hipGetErrorString(e));
    if (L) {
        hipLaunchKernelGGL(k_hier_total, dim3((unsigned)H), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)ell,
                           (const double*)ess, mask, (int)n_ens, L, min_ess);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(ISO_HIER_ERR_HIP, hipGetErrorString(e));
    }
    return 0;
}

int iso_hier_lnlike_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                         int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                         const iso_hier_record* rows, int32_t H, const int32_t* mask, double* ell, double* ess,
                         int32_t* n_bad, double* L, double* min_ess, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_args("iso_hier_lnlike_host", columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim,
                              rows, H, ell, ess, n_bad, L, min_ess);
    if (rc) return rc;
    DevCol col[MAXQ];
    for (int q = 0; q < Q; ++q) col[q] = dev_col(columns[q], layout, W);
    const int T = (int)nsteps, M = T * W;
    const size_t ld = (size_t)n_ens;
    std::vector<double> x((size_t)Q * M), lx((size_t)Q * M), l0((size_t)Q * M), r(M);
    std::vector<char> good(M);
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        if (mask && mask[s] == 0) {
            for (int h = 0; h < H; ++h) ell[(size_t)h * ld + s] = ess[(size_t)h * ld + s] = qnan();
            n_bad[s] = 0;
            continue;
        }
        int nb = 0;
        for (int m = 0; m < M; ++m) {
            const int t = m / W, w = m - t * W;
            bool g = true;
            for (int q = 0; q < Q; ++q) {
                const DevCol& c = col[q];
                const double v = c.base[(int64_t)t * c.st_t + ((int64_t)(s - c.first) * W + w) * c.st_w];
                const size_t i = (size_t)q * M + m;
                x[i] = v;
                lx[i] = log(v);
                l0[i] = lnf(interim[q], v, lx[i]);
                g = g && v == v && l0[i] == l0[i] && l0[i] != neg_inf();
            }
            good[m] = g;
            nb += g ? 0 : 1;
        }
        n_bad[s] = nb;
        for (int h = 0; h < H; ++h) {
            double mx = neg_inf();
            for (int m = 0; m < M; ++m) {
                double acc = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const size_t i = (size_t)q * M + m;
                    double lf = lnf(rows[(size_t)h * Q + q], x[i], lx[i]);
                    lf = (lf == lf) ? lf : neg_inf();
                    const double d = lf - l0[i];
                    acc = (q == 0) ? d : acc + d;
                }
                r[m] = acc;
                if (good[m]) mx = fmax(mx, acc);
            }
            const double sub = (mx == neg_inf()) ? 0.0 : mx;
            double S1 = 0.0, S2 = 0.0;
            for (int m = 0; m < M; ++m) {
                const double wgt = good[m] ? exp(r[m] - sub) : 0.0;
                S1 += wgt;
                S2 += wgt * wgt;
            }
            const bool none = !(S1 > 0.0);
            ell[(size_t)h * ld + s] = none ? neg_inf() : (sub + log(S1)) - log((double)M);
            ess[(size_t)h * ld + s] = none ? 0.0 : (S1 * S1) / S2;
        }
    }
    if (L)
        for (int h = 0; h < H; ++h) {
            double sum = 0.0, mn = HUGE_VAL;
            for (int s = 0; s < n_ens; ++s) {
                if (mask && mask[s] == 0) continue;
                sum += ell[(size_t)h * ld + s];
                mn = fmin(mn, ess[(size_t)h * ld + s]);
            }
            L[h] = sum;
            min_ess[h] = mn;
        }
    return 0;
}

int iso_hier_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, int64_t n, double* out) {
    g_err[0] = 0;
    if (!records || !x || !out) return fail(ISO_HIER_ERR_INVALID, "iso_hier_lnpdf_host", "null pointer");
    if (n_rec < 1 || n < 1) return fail(ISO_HIER_ERR_INVALID, "iso_hier_lnpdf_host", "n_rec and n must be at least 1");
    for (int32_t i = 0; i < n_rec; ++i)
        for (int64_t j = 0; j < n; ++j) out[(size_t)i * n + j] = lnf(records[i], x[j], log(x[j]));
    return 0;
}

}  // extern "C"
