// The population-informed posterior of every star of a catalog under a binned population density for gfx950: per (star,
// cell) the sum over the hyper rows that every sample of the cell shares, with the posterior probability of the star lying
// in the cell, then per sample one weight from one exp.  See include/isochrones_amd_shrink.h for the definitions and the
// summation order, include/isochrones_amd_binned.h for the per-sample term, DESIGN.md section 22 for the mapping and the
// resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64:
//   k_shrink_cells    one workgroup per block of 256 stars, lane = star, as k_binned_rows: ell and A are read as consecutive
//                     doubles.  The cells go a tile of CELL_TILE at a time; per tile two passes over the rows (the maxima,
//                     then the sums), in which lnh[h][b] is the same address in every lane (a scalar load) and ell[h][s]
//                     is loaded once per row for the tile's cells.  The maxima are found in registers; between the passes
//                     they wait in the lane's own column of LDS, where the sums are kept too.
//   k_shrink_weights  one workgroup per star.  The records, the column descriptors, the edges and the star's B values of lnG
//                     are staged in LDS.  Lane i evaluates the samples i, i + 256, ... (sample_term of
//                     common/binned_sample.h, the host entry's own function), writes u and adds it to its sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_shrink.h"
#include "../common/family_lnf.h"
#include "../common/chain_view.h"
#include "../common/hier_columns.h"
#include "../common/wave_reduce.h"
#include "../common/binned_sample.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int CT = ISO_SHRINK_CELL_TILE;
static_assert(sizeof(Rec) == 72, "record layout");

__host__ __device__ inline bool is_finite(double v) { return v - v == 0.0; }

// lnG of the header from a cell's maximum and sum
__host__ __device__ inline double ln_g(double g, double sum, double mx) {
    if (mx != mx) return qnan();
    if (g == neg_inf() || mx == neg_inf()) return neg_inf();
    return g + log(sum);
}

// pc_b of the header
__host__ __device__ inline double cell_mass(double a, double lng) { return a > 0.0 ? exp(log(a) + lng) : 0.0; }

// g of the header for the cells [b0, b0 + CT) of star s, into the lane's column of LDS
__device__ __forceinline__ void tile_maxima(const double* __restrict__ lnh, const double* __restrict__ ell,
                                            double (*s_park)[BLOCK], int b0, int B, int H, size_t ld, int s, double mxs) {
    double g[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) g[j] = neg_inf();
    for (int h = 0; h < H; ++h) {
        const double e = ell[(size_t)h * ld + s];
        const bool le = is_finite(e);
        const double d = e - mxs;
        const double* row = lnh + (size_t)h * B;
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const double l = row[min(b0 + j, B - 1)];
            const bool live = le && l == l && l != neg_inf();
            g[j] = live ? fmax(g[j], l - d) : g[j];
        }
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) s_park[j][threadIdx.x] = g[j];
}

__global__ void __launch_bounds__(BLOCK) k_shrink_cells(const double* __restrict__ A, const double* __restrict__ mx,
                                                        const double* __restrict__ lnh, const double* __restrict__ ell,
                                                        const int32_t* __restrict__ mask, double* __restrict__ lnG,
                                                        double* __restrict__ cellp, int B, int H, int n_ens, int ens_begin,
                                                        int n_ens_out) {
    __shared__ double s_park[2 * CT][BLOCK];    // [j][lane]: a tile's maxima, [CT + j][lane]: its sums
    const int k = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (k >= n_ens_out) return;
    const int s = ens_begin + k;
    const size_t ld = (size_t)n_ens;
    if (mask && mask[s] == 0) {
        for (int b = 0; b < B; ++b) {
            lnG[(size_t)b * ld + s] = qnan();
            if (cellp) cellp[(size_t)b * ld + s] = qnan();
        }
        return;
    }
    const double mxs = mx[s];
    // A tile that reaches past B repeats the last cell (computed, never written).  A tile's maxima wait in LDS between the
    // passes and its sums are kept there (a lane's own column: no barrier, no bank conflict): held in registers next to an
    // exp or a log, whose constants the compiler hoists to the kernel's top (30 registers), they cost the kernel occupancy.
    for (int b0 = 0; b0 < B; b0 += CT) {
        tile_maxima(lnh, ell, s_park, b0, B, H, ld, s, mxs);
#pragma unroll
        for (int j = 0; j < CT; ++j) s_park[CT + j][threadIdx.x] = 0.0;
        for (int h = 0; h < H; ++h) {
            const double e = ell[(size_t)h * ld + s];
            const bool le = is_finite(e);
            const double d = e - mxs;
            const double* row = lnh + (size_t)h * B;
#pragma unroll 1
            for (int j = 0; j < CT; ++j) {      // one exp in flight
                const double l = row[min(b0 + j, B - 1)];
                const bool live = le && l == l && l != neg_inf();
                const double t = live ? exp((l - d) - s_park[j][threadIdx.x]) : 0.0;
                s_park[CT + j][threadIdx.x] = s_park[CT + j][threadIdx.x] + t;
            }
        }
        const int nj = min(CT, B - b0);
#pragma unroll 1
        for (int j = 0; j < nj; ++j)
            lnG[(size_t)(b0 + j) * ld + s] = ln_g(s_park[j][threadIdx.x], s_park[CT + j][threadIdx.x], mxs);
    }
    if (cellp) {
        // the star's cells once more: lnG as this lane wrote it above; pc_b waits in cellp for the star's total
        double tot = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const size_t at = (size_t)b * ld + s;
            const double pc = cell_mass(A[at], lnG[at]);
            cellp[at] = pc;
            tot += pc;
        }
        const bool ok = tot > 0.0 && tot != HUGE_VAL;
        for (int b = 0; b < B; ++b) {
            const size_t at = (size_t)b * ld + s;
            cellp[at] = ok ? cellp[at] / tot : qnan();
        }
    }
}

struct WArgs {
    DevCol col[MAXQ];
    Grid grid;
    const Rec* interim;
    const Rec* frozen;
    const double* edges;
    const double* mx;
    const double* lnG;
    const int32_t* mask;
    double* weights;
    double* wsum;
    double* ess;
    int32_t* n_bad;
    int32_t* n_out;
    int32_t T, W, n_ens, ens_begin;
};

__global__ void __launch_bounds__(BLOCK) k_shrink_weights(const WArgs A) {
    __shared__ Rec s_rec[2 * MAXQ];             // [q]: interim; [MAXQ + q]: frozen
    __shared__ DevCol s_col[MAXQ];
    __shared__ Grid s_grid;
    __shared__ int s_log[MAXQ];
    __shared__ double s_edge[MAX_EDGES];
    __shared__ double s_lng[MAXB];              // the star's lnG of every cell
    __shared__ double s_red[2 * WAVES];
    __shared__ int s_cnt[2 * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = A.grid.Q, B = A.grid.B, W = A.W;
    const int s = A.ens_begin + (int)blockIdx.x;
    const size_t ld = (size_t)A.n_ens;

    if (A.mask && A.mask[s] == 0) {             // workgroup-uniform
        if (tid == 0) {
            A.wsum[s] = qnan();
            A.ess[s] = qnan();
            A.n_bad[s] = 0;
            A.n_out[s] = 0;
        }
        return;
    }

    {   // stage the records as 32-bit words (a frozen record of an axis is carried along and never looked at)
        constexpr int RW = (int)(sizeof(Rec) / 4);
        uint32_t* dst = (uint32_t*)s_rec;
        const uint32_t* src0 = (const uint32_t*)A.interim;
        const uint32_t* src1 = (const uint32_t*)A.frozen;
        for (int i = tid; i < Q * RW; i += BLOCK) {
            dst[i] = src0[i];
            dst[MAXQ * RW + i] = src1[i];
        }
        for (int i = tid; i < A.grid.n_edges; i += BLOCK) s_edge[i] = A.edges[i];
        for (int b = tid; b < B; b += BLOCK) s_lng[b] = A.lnG[(size_t)b * ld + s];
        if (tid == 0) {
            s_col[0] = A.col[0];
            s_col[1] = A.col[1];
            s_col[2] = A.col[2];
            s_col[3] = A.col[3];
            s_grid = A.grid;
        }
    }
    __syncthreads();
    if (tid < Q)
        s_log[tid] = (needs_log(s_rec[tid].kind) || (s_grid.role[tid] == FROZEN && needs_log(s_rec[MAXQ + tid].kind))) ? 1 : 0;
    __syncthreads();

    const int M = A.T * W;
    const double mxs = A.mx[s];
    double* const u_row = A.weights + (size_t)blockIdx.x * (size_t)M;
    double s1 = 0.0, s2 = 0.0;
    int nbad = 0, nout = 0;
    for (int m = tid; m < M; m += BLOCK) {
        int cell, flag;
        const double c = sample_term(s_col, s_rec, s_rec + MAXQ, s_log, s_grid, s_edge, nullptr, s, W, M, m, cell, flag);
        nbad += flag == BAD ? 1 : 0;
        nout += flag == OUT ? 1 : 0;
        const double u = cell >= 0 ? exp((c - mxs) + s_lng[cell]) : 0.0;
        u_row[m] = u;
        s1 += u;
        s2 += u * u;
    }

    const double a = wave_sum(s1), b = wave_sum(s2);
    const int nb = wave_sum_int(nbad), no = wave_sum_int(nout);
    if (lane == 0) {
        s_red[wave] = a;
        s_red[WAVES + wave] = b;
        s_cnt[wave] = nb;
        s_cnt[WAVES + wave] = no;
    }
    __syncthreads();
    if (tid == 0) {
        const double S1 = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        const double S2 = ((s_red[WAVES] + s_red[WAVES + 1]) + s_red[WAVES + 2]) + s_red[WAVES + 3];
        A.wsum[s] = S1;
        A.ess[s] = (S1 == 0.0) ? 0.0 : (S1 * S1) / S2;
        A.n_bad[s] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        A.n_out[s] = ((s_cnt[WAVES] + s_cnt[WAVES + 1]) + s_cnt[WAVES + 2]) + s_cnt[WAVES + 3];
    }
}

int check_cells(const char* who, const double* A, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin,
                int32_t n_ens_out, const double* lnh, const double* ell, int32_t H, const double* lnG) {
    const char* why = nullptr;
    if (!A || !mx || !lnh || !ell || !lnG) why = "null pointer";
    else if (B < 1 || B > MAXB) why = "B must be 1 to 64 cells";
    else if (H < 1) why = "H must be at least 1";
    else if (n_ens < 1) why = "n_ens must be at least 1";
    else if (ens_begin < 0 || n_ens_out < 1 || (int64_t)ens_begin + n_ens_out > n_ens)
        why = "ensemble range [ens_begin, ens_begin + n_ens_out) must be non-empty and inside [0, n_ens)";
    return why ? fail(ISO_SHRINK_ERR_INVALID, who, why) : 0;
}

// the checks of iso_shrink_weights that need no look at device memory; fills G
int check_weights(const char* who, const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens,
                  int32_t W, int32_t ens_begin, int32_t n_ens_out, const Rec* interim, const Rec* frozen, int32_t n_frozen,
                  const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col, const int32_t* n_bins,
                  const double* edges, const double* mx, const double* lnG, const double* weights, const double* wsum,
                  const double* ess, const int32_t* n_bad, const int32_t* n_out, Grid& G) {
    ChainShape s{layout, nsteps, n_ens, W, 1};
    s.ens_begin = ens_begin;
    s.n_ens_out = n_ens_out;
    const char* why = nullptr;
    if (!columns || !interim || !frozen || !axis_col || !n_bins || !edges || !mx || !lnG || !weights || !wsum || !ess ||
        !n_bad || !n_out || (n_frozen > 0 && !frozen_col))
        why = "null pointer";
    else if (Q < 1 || Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    // iso_binned_compress's limit, whose tables the call reads
    else if (nsteps * (int64_t)W > INT32_MAX - BLOCK) why = "more than 2^31 - 257 samples per star (thin the chain)";
    else {
        for (int q = 0; q < Q && !why; ++q) why = column_error(columns[q], W, ens_begin, n_ens_out);
        if (!why) why = grid_error(Q, n_frozen, frozen_col, n_axes, axis_col, n_bins, G);
    }
    return why ? fail(ISO_SHRINK_ERR_INVALID, who, why) : 0;
}

}  // namespace

extern "C" {

const char* iso_shrink_version(void) { return "isochrones_amd shrink 1"; }

const char* iso_shrink_last_error(void) { return g_err; }

int iso_shrink_cells(const double* A, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin, int32_t n_ens_out,
                     const double* lnh, const double* ell, int32_t H, const int32_t* mask, double* lnG, double* cellp,
                     void* stream) {
    g_err[0] = 0;
    const int rc = check_cells("iso_shrink_cells", A, mx, B, n_ens, ens_begin, n_ens_out, lnh, ell, H, lnG);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n_ens_out + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_shrink_cells, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, A, mx, lnh, ell, mask, lnG, cellp,
                       (int)B, (int)H, (int)n_ens, (int)ens_begin, (int)n_ens_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_SHRINK_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_shrink_cells_host(const double* A, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin, int32_t n_ens_out,
                          const double* lnh, const double* ell, int32_t H, const int32_t* mask, double* lnG, double* cellp,
                          void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_shrink_cells_host";
    const int rc = check_cells(who, A, mx, B, n_ens, ens_begin, n_ens_out, lnh, ell, H, lnG);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)H * B; ++i)
        if (lnh[i] == HUGE_VAL) return fail(ISO_SHRINK_ERR_INVALID, who, "a log cell density is +inf");
    const size_t ld = (size_t)n_ens;
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        if (mask && mask[s] == 0) {
            for (int b = 0; b < B; ++b) {
                lnG[(size_t)b * ld + s] = qnan();
                if (cellp) cellp[(size_t)b * ld + s] = qnan();
            }
            continue;
        }
        double tot = 0.0;
        for (int b = 0; b < B; ++b) {
            double g = neg_inf(), sum = 0.0;
            for (int pass = 0; pass < 2; ++pass)
                for (int h = 0; h < H; ++h) {
                    const double e = ell[(size_t)h * ld + s], l = lnh[(size_t)h * B + b];
                    if (!(is_finite(e) && l == l && l != neg_inf())) continue;
                    const double a = l - (e - mx[s]);
                    if (pass == 0) g = fmax(g, a);
                    else sum += exp(a - g);
                }
            const size_t at = (size_t)b * ld + s;
            lnG[at] = ln_g(g, sum, mx[s]);
            if (cellp) {
                cellp[at] = cell_mass(A[at], lnG[at]);
                tot += cellp[at];
            }
        }
        if (cellp) {
            const bool ok = tot > 0.0 && tot != HUGE_VAL;
            for (int b = 0; b < B; ++b) {
                const size_t at = (size_t)b * ld + s;
                cellp[at] = ok ? cellp[at] / tot : qnan();
            }
        }
    }
    return 0;
}

int iso_shrink_weights(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                       int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* frozen,
                       int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col,
                       const int32_t* n_bins, const double* edges, const double* mx, const double* lnG, const int32_t* mask,
                       double* weights, double* wsum, double* ess, int32_t* n_bad, int32_t* n_out, void* stream) {
    g_err[0] = 0;
    WArgs K;
    const int rc = check_weights("iso_shrink_weights", columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim,
                                 frozen, n_frozen, frozen_col, n_axes, axis_col, n_bins, edges, mx, lnG, weights, wsum, ess,
                                 n_bad, n_out, K.grid);
    if (rc) return rc;
    for (int q = 0; q < MAXQ; ++q) K.col[q] = dev_col(columns[q < Q ? q : 0], layout, W);
    K.interim = interim;
    K.frozen = frozen;
    K.edges = edges;
    K.mx = mx;
    K.lnG = lnG;
    K.mask = mask;
    K.weights = weights;
    K.wsum = wsum;
    K.ess = ess;
    K.n_bad = n_bad;
    K.n_out = n_out;
    K.T = (int32_t)nsteps;
    K.W = W;
    K.n_ens = n_ens;
    K.ens_begin = ens_begin;
    hipLaunchKernelGGL(k_shrink_weights, dim3((unsigned)n_ens_out), dim3(BLOCK), 0, (hipStream_t)stream, K);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_SHRINK_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_shrink_weights_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                            int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                            const iso_hier_record* frozen, int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes,
                            const int32_t* axis_col, const int32_t* n_bins, const double* edges, const double* mx,
                            const double* lnG, const int32_t* mask, double* weights, double* wsum, double* ess,
                            int32_t* n_bad, int32_t* n_out, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_shrink_weights_host";
    Grid G;
    const int rc = check_weights(who, columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, frozen, n_frozen,
                                 frozen_col, n_axes, axis_col, n_bins, edges, mx, lnG, weights, wsum, ess, n_bad, n_out, G);
    if (rc) return rc;
    int logs[MAXQ] = {0, 0, 0, 0};
    const char* why = grid_values_error(G, edges, interim, frozen, logs);
    if (why) return fail(ISO_SHRINK_ERR_INVALID, who, why);
    DevCol col[MAXQ];
    for (int q = 0; q < Q; ++q) col[q] = dev_col(columns[q], layout, W);
    const int M = (int)nsteps * W;
    const size_t ld = (size_t)n_ens;
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        n_bad[s] = n_out[s] = 0;
        if (mask && mask[s] == 0) {
            wsum[s] = ess[s] = qnan();
            continue;
        }
        double* const u_row = weights + (size_t)(s - ens_begin) * (size_t)M;
        double S1 = 0.0, S2 = 0.0;
        for (int m = 0; m < M; ++m) {
            int cell, flag;
            const double c = sample_term(col, interim, frozen, logs, G, edges, nullptr, s, W, M, m, cell, flag);
            n_bad[s] += flag == BAD ? 1 : 0;
            n_out[s] += flag == OUT ? 1 : 0;
            const double u = cell >= 0 ? exp((c - mx[s]) + lnG[(size_t)cell * ld + s]) : 0.0;
            u_row[m] = u;
            S1 += u;
            S2 += u * u;
        }
        wsum[s] = S1;
        ess[s] = (S1 == 0.0) ? 0.0 : (S1 * S1) / S2;
    }
    return 0;
}

}  // extern "C"
