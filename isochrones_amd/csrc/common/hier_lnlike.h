// The entry points of the two libraries that take the likelihood of include/isochrones_amd_hier.h straight from the stored
// chains (csrc/hier/, csrc/relation/): the call's arguments and their checks with their messages, the kernel's argument
// block, the two launches, and the host reference over the library's per-column term.  The stars kernel, the row tile it is
// compiled for and the library's error codes come from the library.  Internal and of internal linkage.  The source writes
// no fused multiply-add; it is meant for -ffp-contract=off.
#ifndef ISO_COMMON_HIER_LNLIKE_H
#define ISO_COMMON_HIER_LNLIKE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "family_lnf.h"
#include "hier_columns.h"
#include "hier_block.h"

namespace {

// the arguments of iso_hier_lnlike (and _host, and iso_relation_lnlike's), in the order of the ABI
struct LnlikeCall {
    const iso_hier_column* columns;
    int32_t Q;
    int layout;
    int64_t nsteps;
    int32_t n_ens, W, ens_begin, n_ens_out;
    const Rec* interim;
    const Rec* rows;
    int32_t H;
    const int32_t* mask;
    double* ell;
    double* ess;
    int32_t* n_bad;
    double* L;
    double* min_ess;
    void* stream;
};

// what a library is and returns: ISO_<NAME>_ERR_INVALID, ISO_<NAME>_ERR_HIP, ISO_<NAME>_ROW_TILE
struct LnlikeLib {
    int err_invalid, err_hip, row_tile;
};

// the stars kernel's argument block
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

typedef void (*StarsKernel)(const Args);
typedef void (*TotalKernel)(const double*, const double*, const int32_t*, int, double*, double*);

// clears the library's last error; 0, or err_invalid with the first thing that is wrong as the last error
inline int lnlike_check(const char* who, const LnlikeLib& lib, const LnlikeCall& c) {
    g_err[0] = 0;
    const int RT = lib.row_tile;
    ChainShape s{c.layout, c.nsteps, c.n_ens, c.W, 1};
    s.ens_begin = c.ens_begin;
    s.n_ens_out = c.n_ens_out;
    const char* why = nullptr;
    if (!c.columns || !c.interim || !c.rows || !c.ell || !c.ess || !c.n_bad) why = "null pointer";
    else if ((c.L == nullptr) != (c.min_ess == nullptr)) why = "L and min_ess go together (both or neither)";
    else if (c.Q < 1 || c.Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if (c.H < 1) why = "H must be at least 1";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (c.nsteps * (int64_t)c.W > INT32_MAX) why = "more than 2^31 - 1 samples per star (thin the chain)";
    else if ((int64_t)c.n_ens_out * ((c.H + RT - 1) / RT) > INT32_MAX) why = "more than 2^31 - 1 (star, row tile) pairs (split the call)";
    else
        for (int q = 0; q < c.Q && !why; ++q) why = column_error(c.columns[q], c.W, c.ens_begin, c.n_ens_out);
    return why ? fail(lib.err_invalid, who, why) : 0;
}

// the device entry: the checks, then `stars` over (star, row tile) and, where L is asked for, `total` over the rows
inline int lnlike_launch(const char* who, const LnlikeLib& lib, StarsKernel stars, TotalKernel total, const LnlikeCall& c) {
    const int rc = lnlike_check(who, lib, c);
    if (rc) return rc;
    const int RT = lib.row_tile;
    Args A;
    for (int q = 0; q < MAXQ; ++q) A.col[q] = dev_col(c.columns[q < c.Q ? q : 0], c.layout, c.W);
    A.interim = c.interim;
    A.rows = c.rows;
    A.mask = c.mask;
    A.ell = c.ell;
    A.ess = c.ess;
    A.n_bad = c.n_bad;
    A.Q = c.Q;
    A.T = (int32_t)c.nsteps;
    A.W = c.W;
    A.H = c.H;
    A.n_ens = c.n_ens;
    A.ens_begin = c.ens_begin;
    A.ntiles = (c.H + RT - 1) / RT;
    A.pad = 0;
    hipLaunchKernelGGL(stars, dim3((unsigned)c.n_ens_out * (unsigned)A.ntiles), dim3(BLOCK), 0, (hipStream_t)c.stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(lib.err_hip, hipGetErrorString(e));
    if (c.L) {
        hipLaunchKernelGGL(total, dim3((unsigned)c.H), dim3(BLOCK), 0, (hipStream_t)c.stream, (const double*)c.ell,
                           (const double*)c.ess, c.mask, (int)c.n_ens, c.L, c.min_ess);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(lib.err_hip, hipGetErrorString(e));
    }
    return 0;
}

// the host reference of a call that lnlike_check has passed.  term(R, x, lx, xs, q, Q): the population term of column q of
// a Q-column model under the row's record R; xs: the sample's Q values
template <typename Term>
int lnlike_host(const LnlikeCall& c, Term term) {
    const int Q = c.Q, W = c.W, H = c.H;
    DevCol col[MAXQ];
    for (int q = 0; q < Q; ++q) col[q] = dev_col(c.columns[q], c.layout, W);
    const int T = (int)c.nsteps, M = T * W;
    const size_t ld = (size_t)c.n_ens;
    std::vector<double> x((size_t)Q * M), lx((size_t)Q * M), l0((size_t)Q * M), r(M);
    std::vector<char> good(M);
    for (int s = c.ens_begin; s < c.ens_begin + c.n_ens_out; ++s) {
        if (c.mask && c.mask[s] == 0) {
            for (int h = 0; h < H; ++h) c.ell[(size_t)h * ld + s] = c.ess[(size_t)h * ld + s] = qnan();
            c.n_bad[s] = 0;
            continue;
        }
        int nb = 0;
        for (int m = 0; m < M; ++m) {
            const int t = m / W, w = m - t * W;
            bool g = true;
            for (int q = 0; q < Q; ++q) {
                const double v = load(col[q], s, W, t, w);
                const size_t i = (size_t)q * M + m;
                x[i] = v;
                lx[i] = log(v);
                l0[i] = lnf(c.interim[q], v, lx[i]);
                g = g && v == v && l0[i] == l0[i] && l0[i] != neg_inf();
            }
            good[m] = g;
            nb += g ? 0 : 1;
        }
        c.n_bad[s] = nb;
        for (int h = 0; h < H; ++h) {
            double mx = neg_inf();
            for (int m = 0; m < M; ++m) {
                double xs[MAXQ] = {0.0, 0.0, 0.0, 0.0};
                for (int q = 0; q < Q; ++q) xs[q] = x[(size_t)q * M + m];
                double acc = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const size_t i = (size_t)q * M + m;
                    double lf = term(c.rows[(size_t)h * Q + q], x[i], lx[i], xs, q, Q);
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
            c.ell[(size_t)h * ld + s] = none ? neg_inf() : (sub + log(S1)) - log((double)M);
            c.ess[(size_t)h * ld + s] = none ? 0.0 : (S1 * S1) / S2;
        }
    }
    if (c.L) row_totals_host(c.ell, c.ess, c.mask, c.n_ens, H, c.L, c.min_ess);
    return 0;
}

}  // namespace

#endif
