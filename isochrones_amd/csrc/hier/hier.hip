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
//   k_hier_total  one workgroup per row: L and min_ess over the unmasked stars in a fixed order (common/hier_block.h).
// The checks, the argument block, the launches and the host reference are common/hier_lnlike.h's, which csrc/relation/
// shares; the family arithmetic is common/family_lnf.h's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_hier.h"
#include "../common/family_lnf.h"
#include "../common/hier_lnlike.h"

namespace {

constexpr int RT = ISO_HIER_ROW_TILE;
constexpr LnlikeLib LIB{ISO_HIER_ERR_INVALID, ISO_HIER_ERR_HIP, RT};
static_assert(sizeof(iso_hier_record) == 72, "record layout");

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
                const double x = load(s_col[q], s, W, t, w);
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
    row_total(ell, ess, mask, n_ens, L, min_ess);
}

}  // namespace

extern "C" {

const char* iso_hier_version(void) { return "isochrones_amd hier 1"; }

const char* iso_hier_last_error(void) { return g_err; }

int iso_hier_lnlike(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                    int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* rows,
                    int32_t H, const int32_t* mask, double* ell, double* ess, int32_t* n_bad, double* L, double* min_ess,
                    void* stream) {
    return lnlike_launch("iso_hier_lnlike", LIB, k_hier_stars, k_hier_total,
                         LnlikeCall{columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, rows, H, mask, ell,
                                    ess, n_bad, L, min_ess, stream});
}

int iso_hier_lnlike_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                         int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                         const iso_hier_record* rows, int32_t H, const int32_t* mask, double* ell, double* ess,
                         int32_t* n_bad, double* L, double* min_ess, void* stream) {
    const LnlikeCall c{columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, rows, H, mask, ell, ess, n_bad,
                       L, min_ess, stream};
    const int rc = lnlike_check("iso_hier_lnlike_host", LIB, c);
    if (rc) return rc;
    return lnlike_host(c, [](const Rec& R, double x, double lx, const double*, int, int) { return lnf(R, x, lx); });
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
