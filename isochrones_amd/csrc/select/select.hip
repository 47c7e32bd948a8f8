// The detectable fraction of a population density from an injection set for gfx950: per hyper row the log of the mean
// importance weight of the injections, each weighted by its detection probability, and the effective sample size of that
// mean.  See include/isochrones_amd_select.h for the definition and the summation order, DESIGN.md section 18 for the
// mapping and the resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64:
//   k_select_partial  one workgroup per (chunk of ISO_SELECT_CHUNK injections, tile of ROW_TILE hyper rows).  The draw
//                     records and the tile's records are staged in LDS (every lane reads the same address: a broadcast).
//                     Lanes run along the injection axis, so consecutive lanes read consecutive doubles of a column.  The
//                     chunk is streamed twice per tile (maximum, then sums: the second read comes from the cache); per
//                     injection and column x, ln x (only where a record of the column needs it), the draw term and the
//                     bad-injection test are computed once and serve the tile's rows, whose accumulators stay in registers.
//                     It writes (mx_c, s1_c, s2_c) per (chunk, row) and the chunk's bad count to the workspace.
//   k_select_total    one workgroup per row: the chunks' partial sums rescaled to the global maximum and added in a fixed
//                     order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "isochrones_amd_select.h"
#include "../common/family_lnf.h"
#include "../common/last_error.h"
#include "../common/wave_reduce.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int RT = ISO_HIER_ROW_TILE;
constexpr int CHUNK = ISO_SELECT_CHUNK;
static_assert(sizeof(Rec) == 72, "record layout");
static_assert(CHUNK % BLOCK == 0, "a chunk is whole passes of the workgroup");

// the workspace: three planes [H][C] of doubles (mx_c, s1_c, s2_c), then C int32 bad counts
struct Args {
    const double* x;
    const double* lnd;
    const Rec* draw;
    const Rec* rows;
    double* ws;
    int64_t J;
    int32_t Q, H, C, ntiles;
};

__host__ __device__ inline int64_t n_chunks(int64_t J) { return (J + CHUNK - 1) / CHUNK; }

__global__ void __launch_bounds__(BLOCK) k_select_partial(const Args A) {
    __shared__ Rec s_rec[(RT + 1) * MAXQ];      // [0][q]: draw; [1 + k][q]: row k of the tile
    __shared__ double s_red[2 * RT * WAVES];
    __shared__ int s_bad[WAVES];
    __shared__ int s_log[MAXQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = A.Q, H = A.H;
    const int chunk = (int)(blockIdx.x / (unsigned)A.ntiles), tile = (int)(blockIdx.x - (unsigned)chunk * A.ntiles);
    const int h0 = tile * RT;
    const int64_t J = A.J, j0 = (int64_t)chunk * CHUNK;
    const int n = (int)((J - j0 < CHUNK) ? J - j0 : CHUNK);     // injections of this chunk, at least 1

    // stage the records as 32-bit words; a tile that reaches past H repeats the last row (computed, never written)
    {
        constexpr int RW = (int)(sizeof(Rec) / 4);
        uint32_t* dst = (uint32_t*)s_rec;
        const uint32_t* src0 = (const uint32_t*)A.draw;
        for (int i = tid; i < Q * RW; i += BLOCK) dst[i] = src0[i];
        for (int i = tid; i < RT * Q * RW; i += BLOCK) {
            const int k = i / (Q * RW), w = i - k * (Q * RW);
            const int h = min(h0 + k, H - 1);
            dst[(1 + k) * MAXQ * RW + w] = ((const uint32_t*)(A.rows + (size_t)h * Q))[w];
        }
    }
    __syncthreads();
    if (tid < Q) {
        int need = 0;
        for (int k = 0; k <= RT; ++k) need |= needs_log(s_rec[k * MAXQ + tid].kind) ? 1 : 0;
        s_log[tid] = need;
    }
    __syncthreads();

    double mx[RT], s1[RT], s2[RT];
#pragma unroll
    for (int k = 0; k < RT; ++k) {
        mx[k] = neg_inf();
        s1[k] = 0.0;
        s2[k] = 0.0;
    }
    int nbad = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = tid; i < n; i += BLOCK) {
            const int64_t j = j0 + i;
            double r[RT];
#pragma unroll
            for (int k = 0; k < RT; ++k) r[k] = 0.0;
            const double ld = A.lnd[j];
            bool good = ld <= 0.0;                              // false for NaN and for a positive lnd
            for (int q = 0; q < Q; ++q) {
                const double x = A.x[(size_t)q * (size_t)J + (size_t)j];
                const double lx = s_log[q] ? log(x) : 0.0;      // workgroup-uniform choice
                const double l0 = lnf(s_rec[q], x, lx);
                good = good && x == x && l0 == l0 && l0 != neg_inf();
#pragma unroll
                for (int k = 0; k < RT; ++k) {
                    double lf = lnf(s_rec[(1 + k) * MAXQ + q], x, lx);
                    lf = (lf == lf) ? lf : neg_inf();
                    const double d = lf - l0;
                    r[k] = (q == 0) ? d : r[k] + d;
                }
            }
            if (pass == 0) {
                nbad += good ? 0 : 1;
#pragma unroll
                for (int k = 0; k < RT; ++k) mx[k] = good ? fmax(mx[k], r[k] + ld) : mx[k];
            } else {
#pragma unroll
                for (int k = 0; k < RT; ++k) {
                    const double wgt = good ? exp((r[k] + ld) - mx[k]) : 0.0;
                    s1[k] += wgt;
                    s2[k] += wgt * wgt;
                }
            }
        }
        if (pass == 0) {
            // the maximum over the workgroup; a row with no support in the chunk subtracts 0 and writes -inf
#pragma unroll
            for (int k = 0; k < RT; ++k) {
                const double v = wave_max(mx[k]);
                if (lane == 0) s_red[k * WAVES + wave] = v;
            }
            const int b = wave_sum_int(nbad);
            if (lane == 0) s_bad[wave] = b;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < RT; ++k) {
                const double v = fmax(fmax(s_red[k * WAVES], s_red[k * WAVES + 1]),
                                      fmax(s_red[k * WAVES + 2], s_red[k * WAVES + 3]));
                mx[k] = (v == neg_inf()) ? 0.0 : v;
            }
            if (tile == 0 && tid == 0)
                ((int32_t*)(A.ws + (size_t)3 * H * A.C))[chunk] = ((s_bad[0] + s_bad[1]) + s_bad[2]) + s_bad[3];
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < RT; ++k) {
        const double a = wave_sum(s1[k]), b = wave_sum(s2[k]);
        if (lane == 0) {
            s_red[k * WAVES + wave] = a;
            s_red[(RT + k) * WAVES + wave] = b;
        }
    }
    __syncthreads();
    if (tid < RT && h0 + tid < H) {
        const int k = tid;
        const double S1 = ((s_red[k * WAVES] + s_red[k * WAVES + 1]) + s_red[k * WAVES + 2]) + s_red[k * WAVES + 3];
        const double S2 = ((s_red[(RT + k) * WAVES] + s_red[(RT + k) * WAVES + 1]) + s_red[(RT + k) * WAVES + 2]) +
                          s_red[(RT + k) * WAVES + 3];
        // mx[k] is the same in every lane; lane k needs row k's: a chain of selects, not a dynamic register index
        double mxk = 0.0;
#pragma unroll
        for (int m = 0; m < RT; ++m) mxk = (m == k) ? mx[m] : mxk;
        const bool none = !(S1 > 0.0);
        const size_t plane = (size_t)H * A.C, at = (size_t)(h0 + k) * A.C + chunk;
        A.ws[at] = none ? neg_inf() : mxk;
        A.ws[plane + at] = none ? 0.0 : S1;
        A.ws[2 * plane + at] = none ? 0.0 : S2;
    }
}

__global__ void __launch_bounds__(BLOCK) k_select_total(const double* __restrict__ ws, int C, int H, double lnJ,
                                                        double* __restrict__ ln_alpha, double* __restrict__ n_eff,
                                                        int32_t* __restrict__ n_bad) {
    __shared__ double s_red[2 * WAVES];
    __shared__ int s_bad[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x;
    const size_t plane = (size_t)H * C;
    const double* mxc = ws + (size_t)h * C;
    const double* s1c = mxc + plane;
    const double* s2c = s1c + plane;
    double mx = neg_inf();
    for (int c = tid; c < C; c += BLOCK) mx = fmax(mx, mxc[c]);
    mx = wave_max(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    const double MX = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
    __syncthreads();
    double a = 0.0, b = 0.0;
    if (MX != neg_inf())
        for (int c = tid; c < C; c += BLOCK) {
            const double d = mxc[c] - MX;                       // -inf for a chunk without support: exp gives 0
            a += s1c[c] * exp(d);
            b += s2c[c] * exp(2.0 * d);
        }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        s_red[wave] = a;
        s_red[WAVES + wave] = b;
    }
    if (h == 0) {                                               // workgroup-uniform
        const int32_t* bad = (const int32_t*)(ws + 3 * plane);
        int nb = 0;
        for (int c = tid; c < C; c += BLOCK) nb += bad[c];
        nb = wave_sum_int(nb);
        if (lane == 0) s_bad[wave] = nb;
    }
    __syncthreads();
    if (tid == 0) {
        const double S1 = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        const double S2 = ((s_red[WAVES] + s_red[WAVES + 1]) + s_red[WAVES + 2]) + s_red[WAVES + 3];
        const bool none = !(S1 > 0.0);
        ln_alpha[h] = none ? neg_inf() : (MX + log(S1)) - lnJ;
        n_eff[h] = none ? 0.0 : (S1 * S1) / S2;
        if (h == 0) n_bad[0] = ((s_bad[0] + s_bad[1]) + s_bad[2]) + s_bad[3];
    }
}

int check_args(const char* who, const double* x, int32_t Q, int64_t J, const double* lnd, const Rec* draw, const Rec* rows,
               int32_t H, const double* workspace, bool need_workspace, const double* ln_alpha, const double* n_eff,
               const int32_t* n_bad) {
    const char* why = nullptr;
    if (!x || !lnd || !draw || !rows || !ln_alpha || !n_eff || !n_bad || (need_workspace && !workspace)) why = "null pointer";
    else if (Q < 1 || Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if (H < 1) why = "H must be at least 1";
    else if (J < 1 || J > INT32_MAX) why = "J must be 1 to 2^31 - 1 injections";
    else if (n_chunks(J) * ((H + RT - 1) / RT) > INT32_MAX) why = "more than 2^31 - 1 (chunk, row tile) pairs (split the rows)";
    return why ? fail(ISO_SELECT_ERR_INVALID, who, why) : 0;
}

}  // namespace

extern "C" {

const char* iso_select_version(void) { return "isochrones_amd select 1"; }

const char* iso_select_last_error(void) { return g_err; }

int64_t iso_select_workspace_doubles(int64_t J, int32_t H) {
    if (J < 1 || H < 1) return 0;
    const int64_t C = n_chunks(J);
    return 3 * C * (int64_t)H + (C + 1) / 2;
}

int iso_select_alpha(const double* x, int32_t Q, int64_t J, const double* lnd, const iso_hier_record* draw,
                     const iso_hier_record* rows, int32_t H, double* workspace, double* ln_alpha, double* n_eff,
                     int32_t* n_bad, void* stream) {
    g_err[0] = 0;
    const int rc = check_args("iso_select_alpha", x, Q, J, lnd, draw, rows, H, workspace, true, ln_alpha, n_eff, n_bad);
    if (rc) return rc;
    Args A;
    A.x = x;
    A.lnd = lnd;
    A.draw = draw;
    A.rows = rows;
    A.ws = workspace;
    A.J = J;
    A.Q = Q;
    A.H = H;
    A.C = (int32_t)n_chunks(J);
    A.ntiles = (H + RT - 1) / RT;
    hipLaunchKernelGGL(k_select_partial, dim3((unsigned)A.C * (unsigned)A.ntiles), dim3(BLOCK), 0, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_SELECT_ERR_HIP, hipGetErrorString(e));
    hipLaunchKernelGGL(k_select_total, dim3((unsigned)H), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)workspace,
                       (int)A.C, (int)H, log((double)J), ln_alpha, n_eff, n_bad);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_SELECT_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_select_alpha_host(const double* x, int32_t Q, int64_t J, const double* lnd, const iso_hier_record* draw,
                          const iso_hier_record* rows, int32_t H, double* workspace, double* ln_alpha, double* n_eff,
                          int32_t* n_bad, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_args("iso_select_alpha_host", x, Q, J, lnd, draw, rows, H, workspace, false, ln_alpha, n_eff, n_bad);
    if (rc) return rc;
    const size_t n = (size_t)J;
    std::vector<double> lx((size_t)Q * n), l0((size_t)Q * n), t(n);
    std::vector<char> good(n);
    int nb = 0;
    for (size_t j = 0; j < n; ++j) {
        bool g = lnd[j] <= 0.0;
        for (int q = 0; q < Q; ++q) {
            const size_t i = (size_t)q * n + j;
            const double v = x[i];
            lx[i] = log(v);
            l0[i] = lnf(draw[q], v, lx[i]);
            g = g && v == v && l0[i] == l0[i] && l0[i] != neg_inf();
        }
        good[j] = g;
        nb += g ? 0 : 1;
    }
    n_bad[0] = nb;
    for (int h = 0; h < H; ++h) {
        double mx = neg_inf();
        for (size_t j = 0; j < n; ++j) {
            double acc = 0.0;
            for (int q = 0; q < Q; ++q) {
                const size_t i = (size_t)q * n + j;
                double lf = lnf(rows[(size_t)h * Q + q], x[i], lx[i]);
                lf = (lf == lf) ? lf : neg_inf();
                const double d = lf - l0[i];
                acc = (q == 0) ? d : acc + d;
            }
            t[j] = acc + lnd[j];
            if (good[j]) mx = fmax(mx, t[j]);
        }
        const double sub = (mx == neg_inf()) ? 0.0 : mx;
        double S1 = 0.0, S2 = 0.0;
        for (size_t j = 0; j < n; ++j) {
            const double wgt = good[j] ? exp(t[j] - sub) : 0.0;
            S1 += wgt;
            S2 += wgt * wgt;
        }
        const bool none = !(S1 > 0.0);
        ln_alpha[h] = none ? neg_inf() : (sub + log(S1)) - log((double)J);
        n_eff[h] = none ? 0.0 : (S1 * S1) / S2;
    }
    return 0;
}

int iso_select_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, int64_t n, double* out) {
    g_err[0] = 0;
    if (!records || !x || !out) return fail(ISO_SELECT_ERR_INVALID, "iso_select_lnpdf_host", "null pointer");
    if (n_rec < 1 || n < 1) return fail(ISO_SELECT_ERR_INVALID, "iso_select_lnpdf_host", "n_rec and n must be at least 1");
    for (int32_t i = 0; i < n_rec; ++i)
        for (int64_t j = 0; j < n; ++j) out[(size_t)i * n + j] = lnf(records[i], x[j], log(x[j]));
    return 0;
}

}  // extern "C"
