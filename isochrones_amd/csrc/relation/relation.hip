// The hierarchical (population) likelihood of a catalog from the stored chains of its stars for gfx950, for population
// densities in which a column's Gaussian follows another column linearly: per (hyper row, star) the log of the mean
// importance weight and its effective sample size; per row their total.  See include/isochrones_amd_relation.h for the
// linked kind, include/isochrones_amd_hier.h for everything else, DESIGN.md section 20 for the mapping and the resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64, on the plan of csrc/hier/hier.hip and launched through the
// entry points it shares with it (common/hier_lnlike.h: the checks, the argument block, the host reference):
//   k_relation_stars  one workgroup per (star, tile of ROW_TILE hyper rows).  The interim records, the tile's records and
//                     the column descriptors are staged in LDS, and next to them per (row, column) of the tile whether the
//                     record is linked and to which parent.  A lane loads all Q values of its sample first (a linked term
//                     needs its parent's, whichever side of it the parent lies), then per column ln x, the interim term and
//                     the bad-sample test once, then the tile's rows.  Which rows of a column are linked is the same for the
//                     whole workgroup and is read into a scalar, one bit a row: a column without a link runs k_hier_stars's
//                     loop as it is; in a linked one the two erfc and the log of the per-sample normaliser run only for the
//                     linked rows, under a scalar branch, and the parent's value comes from a chain of selects on a scalar,
//                     not from a dynamic register index.
//   k_relation_total  one workgroup per row: L and min_ess over the unmasked stars in a fixed order (common/hier_block.h, as
//                     k_hier_total).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_relation.h"
#include "../common/relation_lnf.h"
#include "../common/hier_lnlike.h"

namespace {

constexpr int RT = ISO_RELATION_ROW_TILE;
constexpr LnlikeLib LIB{ISO_RELATION_ERR_INVALID, ISO_RELATION_ERR_HIP, RT};
constexpr int NOT_LINKED = -1, BAD_PARENT = -2; // s_par: else the parent column
static_assert(sizeof(Rec) == 72, "record layout");
static_assert(MAXQ == 4 && RT * MAXQ <= BLOCK, "the select chains and the staging below are written for four columns");

// the sample's value of column k, for a k that is the same in every lane
__device__ __forceinline__ double pick(double x0, double x1, double x2, double x3, int k) {
    double v = x0;
    v = (k == 1) ? x1 : v;
    v = (k == 2) ? x2 : v;
    v = (k == 3) ? x3 : v;
    return v;
}

__global__ void __launch_bounds__(BLOCK) k_relation_stars(const Args A) {
    __shared__ Rec s_rec[(RT + 1) * MAXQ];      // [0][q]: interim; [1 + j][q]: row j of the tile
    __shared__ DevCol s_col[MAXQ];
    __shared__ double s_red[2 * RT * WAVES];
    __shared__ int s_bad[WAVES];
    __shared__ int s_log[MAXQ];
    __shared__ int s_par[RT * MAXQ];            // [j][q]: NOT_LINKED, BAD_PARENT or the parent column of row j's record
    __shared__ int s_link[MAXQ];                // [q] bit j: row j's record of column q is linked
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
    if (tid < RT * MAXQ) {
        const int q = tid & (MAXQ - 1);
        int par = NOT_LINKED;
        if (q < Q) {
            const Rec& R = s_rec[MAXQ + tid];   // [1 + j][q], j = tid / MAXQ
            if (R.kind == ISO_RELATION_LINGAUSS) par = parent_ok(R.reserved, q, Q) ? R.reserved : BAD_PARENT;
        }
        s_par[tid] = par;
    }
    __syncthreads();
    if (tid < MAXQ) {
        int bits = 0;
        for (int j = 0; j < RT; ++j) bits |= (s_par[j * MAXQ + tid] != NOT_LINKED) ? 1 << j : 0;
        s_link[tid] = bits;
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
            // named scalars, not an array: the chains of selects below keep them in registers
            const double x0 = load(s_col[0], s, W, t, w);
            const double x1 = Q > 1 ? load(s_col[1], s, W, t, w) : 0.0;
            const double x2 = Q > 2 ? load(s_col[2], s, W, t, w) : 0.0;
            const double x3 = Q > 3 ? load(s_col[3], s, W, t, w) : 0.0;
            double r[RT];
#pragma unroll
            for (int j = 0; j < RT; ++j) r[j] = 0.0;
            bool good = true;
#pragma unroll 1
            for (int q = 0; q < Q; ++q) {
                const double x = pick(x0, x1, x2, x3, q);
                const double lx = s_log[q] ? log(x) : 0.0;      // workgroup-uniform choice
                const double l0 = lnf(s_rec[q], x, lx);
                good = good && x == x && l0 == l0 && l0 != neg_inf();
                // one scalar per column says which of the tile's rows are linked; a column without a link (most are) takes
                // k_hier_stars's loop as it is, with nothing between its rows
                const int linked = __builtin_amdgcn_readfirstlane(s_link[q]);
                if (linked == 0) {
#pragma unroll
                    for (int j = 0; j < RT; ++j) {
                        double lf = lnf(s_rec[(1 + j) * MAXQ + q], x, lx);
                        lf = (lf == lf) ? lf : neg_inf();
                        const double d = lf - l0;
                        r[j] = (q == 0) ? d : r[j] + d;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < RT; ++j) {
                        const Rec& R = s_rec[(1 + j) * MAXQ + q];
                        double lf;
                        if (linked >> j & 1) {
                            const int par = __builtin_amdgcn_readfirstlane(s_par[j * MAXQ + q]);
                            lf = par == BAD_PARENT ? qnan() : lingauss_lnf(R, x, pick(x0, x1, x2, x3, par));
                        } else {
                            lf = lnf(R, x, lx);
                        }
                        lf = (lf == lf) ? lf : neg_inf();
                        const double d = lf - l0;
                        r[j] = (q == 0) ? d : r[j] + d;
                    }
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
        // mx[j] is the same in every lane; lane j needs row j's: take it by a chain of selects, not a dynamic register index
        double mxj = 0.0;
#pragma unroll
        for (int k = 0; k < RT; ++k) mxj = (k == j) ? mx[k] : mxj;
        const bool none = !(S1 > 0.0);
        A.ell[(size_t)(h0 + j) * ld + s] = none ? neg_inf() : (mxj + log(S1)) - log((double)M);
        A.ess[(size_t)(h0 + j) * ld + s] = none ? 0.0 : (S1 * S1) / S2;
    }
}

__global__ void __launch_bounds__(BLOCK) k_relation_total(const double* __restrict__ ell, const double* __restrict__ ess,
                                                          const int32_t* __restrict__ mask, int n_ens,
                                                          double* __restrict__ L, double* __restrict__ min_ess) {
    row_total(ell, ess, mask, n_ens, L, min_ess);
}

}  // namespace

extern "C" {

const char* iso_relation_version(void) { return "isochrones_amd relation 1"; }

const char* iso_relation_last_error(void) { return g_err; }

int iso_relation_lnlike(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                        int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* rows,
                        int32_t H, const int32_t* mask, double* ell, double* ess, int32_t* n_bad, double* L,
                        double* min_ess, void* stream) {
    return lnlike_launch("iso_relation_lnlike", LIB, k_relation_stars, k_relation_total,
                         LnlikeCall{columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, rows, H, mask, ell,
                                    ess, n_bad, L, min_ess, stream});
}

int iso_relation_lnlike_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                             int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                             const iso_hier_record* rows, int32_t H, const int32_t* mask, double* ell, double* ess,
                             int32_t* n_bad, double* L, double* min_ess, void* stream) {
    const char* who = "iso_relation_lnlike_host";
    const LnlikeCall c{columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, rows, H, mask, ell, ess, n_bad,
                       L, min_ess, stream};
    const int rc = lnlike_check(who, LIB, c);
    if (rc) return rc;
    for (int q = 0; q < Q; ++q)
        if (interim[q].kind == ISO_RELATION_LINGAUSS)
            return fail(ISO_RELATION_ERR_INVALID, who, "an interim record is linked (interim records are of the kinds 1 to 8)");
    return lnlike_host(c, relation_lnf);
}

int iso_relation_lnpdf_host(const iso_hier_record* records, int32_t n_rec, const double* x, const double* xp, int64_t n,
                            double* out) {
    g_err[0] = 0;
    const char* who = "iso_relation_lnpdf_host";
    if (!records || !x || !out) return fail(ISO_RELATION_ERR_INVALID, who, "null pointer");
    if (n_rec < 1 || n < 1) return fail(ISO_RELATION_ERR_INVALID, who, "n_rec and n must be at least 1");
    for (int32_t i = 0; i < n_rec; ++i)
        if (records[i].kind == ISO_RELATION_LINGAUSS && !xp)
            return fail(ISO_RELATION_ERR_INVALID, who, "a linked record needs the parent values xp");
    for (int32_t i = 0; i < n_rec; ++i)
        for (int64_t j = 0; j < n; ++j)
            out[(size_t)i * n + j] = records[i].kind == ISO_RELATION_LINGAUSS ? lingauss_lnf(records[i], x[j], xp[j])
                                                                              : lnf(records[i], x[j], log(x[j]));
    return 0;
}

}  // extern "C"
