// The per-sample term of include/isochrones_amd_binned.h for host and device code: the grid of bins, the bin of a value and
// c_m with its cell and its bad / out flag, and the checks of a grid's arguments with their messages.  Internal and of
// internal linkage.  The source writes no fused multiply-add; it is meant for -ffp-contract=off.
//
// This restates Grid, bracket() and sample_term() of csrc/binned/binned.hip line for line, for csrc/shrink/ alone.
// binned.hip keeps its own copy for now: the list of headers libiso_binned.so is built from is pinned by its library
// test, so moving it onto this header is a change of its own (DESIGN.md section 22 names it as the follow-up).  Until then
// tests/test_shrink_host_abi_cpu.py holds the two copies together bit for bit: the weights of this header summed per cell
// are the table of that one.
#ifndef ISO_COMMON_BINNED_SAMPLE_H
#define ISO_COMMON_BINNED_SAMPLE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_binned.h"
#include "family_lnf.h"
#include "hier_columns.h"

namespace {

constexpr int MAXB = ISO_BINNED_MAX_CELLS;
constexpr int MAXA = ISO_BINNED_MAX_AXES;
constexpr int MAX_EDGES = MAXB + 1 + 2;         // 64 x 1 bins: 65 + 2 edges
constexpr int FROZEN = -1;                      // Grid::role: else the axis number
constexpr int BAD = 1, OUT = 2;                 // sample_term's flag
static_assert(MAXB <= 64 && MAXA == 2, "two bin terms");

// the grid of bins; the same in every lane
struct Grid {
    int32_t Q, n_axes, B, n_edges;
    int32_t role[MAXQ];                         // FROZEN, or the axis the column is
    int32_t nb[MAXA], e0[MAXA], mul[MAXA];      // per axis: bins, where its edges start, the cell index's factor
};

// the bin of x on the edges e[0 .. K]: e[k] <= x < e[k + 1], x == e[K] in K - 1; -1 outside (x is no NaN)
__host__ __device__ inline int bracket(const double* e, int K, double x) {
    if (!(x >= e[0] && x <= e[K])) return -1;
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= e[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// c_m of the header for sample m of star s; cell: the sample's cell, or -1 if it weighs nothing (bad, out, or c = -inf);
// flag: 0, BAD or OUT.  logs[q]: a record of column q needs ln x
__host__ __device__ inline double sample_term(const DevCol* col, const Rec* interim, const Rec* frozen, const int* logs,
                                              const Grid& G, const double* edges, const double* extra, int s, int W, int M,
                                              int m, int& cell, int& flag) {
    const int t = m / W, w = m - t * W;
    double cf = 0.0, b0 = 0.0, b1 = 0.0;
    bool good = true, in = true;
    int idx = 0, seen = 0;
#pragma unroll 1
    for (int q = 0; q < G.Q; ++q) {
        const double x = load(col[q], s, W, t, w);
        const double lx = logs[q] ? log(x) : 0.0;
        const double l0 = lnf(interim[q], x, lx);
        good = good && x == x && l0 == l0 && l0 != neg_inf();
        const int a = G.role[q];
        if (a == FROZEN) {
            double lf = lnf(frozen[q], x, lx);
            lf = (lf == lf) ? lf : neg_inf();
            cf += lf - l0;
        } else {
            const int k = (x == x) ? bracket(edges + G.e0[a], G.nb[a], x) : -1;
            in = in && k >= 0;
            idx += (k < 0 ? 0 : k) * G.mul[a];
            b0 = seen == 0 ? l0 : b0;
            b1 = seen == 0 ? b1 : l0;
            ++seen;
        }
    }
    double cm = cf - b0;
    if (G.n_axes == 2) cm -= b1;
    if (extra) {
        const double ex = extra[(int64_t)s * M + m];
        good = good && ex == ex && !(ex > 0.0);
        cm += ex;
    }
    flag = good ? (in ? 0 : OUT) : BAD;
    cell = (good && in && cm > neg_inf()) ? idx : -1;
    return cm;
}

// what is wrong with the grid arguments of iso_binned_compress (the shape and the columns are checked by the caller), or
// nullptr; fills G
inline const char* grid_error(int32_t Q, int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col,
                              const int32_t* n_bins, Grid& G) {
    if (n_axes < 1 || n_axes > MAXA) return "a grid has 1 or 2 binned axes";
    if (n_frozen < 0 || n_frozen > Q) return "n_frozen must be 0 to Q";
    G = Grid{};
    G.Q = Q;
    G.n_axes = n_axes;
    int role[MAXQ] = {-2, -2, -2, -2};          // -2: not listed yet
    for (int a = 0; a < n_axes; ++a) {
        const int q = axis_col[a];
        if (q < 0 || q >= Q) return "a binned axis is no column (outside [0, Q))";
        if (role[q] != -2) return "a column is listed as a binned axis twice";
        if (n_bins[a] < 1) return "an axis needs at least 1 bin";
        role[q] = a;
    }
    for (int i = 0; i < n_frozen; ++i) {
        const int q = frozen_col[i];
        if (q < 0 || q >= Q) return "a frozen column is no column (outside [0, Q))";
        if (role[q] >= 0) return "a column is listed both as a binned axis and as frozen";
        if (role[q] == FROZEN) return "a column is listed as frozen twice";
        role[q] = FROZEN;
    }
    for (int q = 0; q < Q; ++q)
        if (role[q] == -2) return "a column is neither a binned axis nor frozen";
    if ((int64_t)n_bins[0] * (n_axes == 2 ? n_bins[1] : 1) > MAXB) return "more than 64 cells";
    for (int q = 0; q < MAXQ; ++q) G.role[q] = q < Q ? role[q] : FROZEN;
    G.nb[0] = n_bins[0];
    G.nb[1] = n_axes == 2 ? n_bins[1] : 1;
    G.e0[0] = 0;
    G.e0[1] = n_bins[0] + 1;
    G.mul[0] = G.nb[1];
    G.mul[1] = 1;
    G.B = G.nb[0] * G.nb[1];
    G.n_edges = n_bins[0] + 1 + (n_axes == 2 ? n_bins[1] + 1 : 0);
    return nullptr;
}

// the host entries see the edges and the records: what is wrong with them, or nullptr; fills logs[q]
inline const char* grid_values_error(const Grid& G, const double* edges, const Rec* interim, const Rec* frozen, int* logs) {
    for (int a = 0; a < G.n_axes; ++a)
        for (int k = 0; k <= G.nb[a]; ++k) {
            const double e = edges[G.e0[a] + k];
            if (!(e - e == 0.0) || (k > 0 && !(e > edges[G.e0[a] + k - 1])))
                return "the edges of an axis must be finite and strictly increasing";
        }
    for (int q = 0; q < G.Q; ++q) {
        const bool fr = G.role[q] == FROZEN;
        if (interim[q].kind < ISO_HIER_FLAT || interim[q].kind > ISO_HIER_TRUNCGAUSS ||
            (fr && (frozen[q].kind < ISO_HIER_FLAT || frozen[q].kind > ISO_HIER_TRUNCGAUSS)))
            return "an interim or frozen record is not of the kinds 1 to 8";
        logs[q] = (needs_log(interim[q].kind) || (fr && needs_log(frozen[q].kind))) ? 1 : 0;
    }
    return nullptr;
}

}  // namespace

#endif
