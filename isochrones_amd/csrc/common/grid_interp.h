// The one definition of a grid cell's interpolation for the libraries that read the packed 3-D model grid
// (csrc/derived/, csrc/predict/, csrc/population/) and the packed 4-D bolometric-correction grid (csrc/predict/,
// csrc/population/): the on-axis rule, the brackets (grid_cell.h), the weight products with their parentheses, the corner
// order, the offsets and the NaN fill.  The public headers state the arithmetic; a value is the same bits in these
// libraries, kernel and host entry, because every one of them compiles these lines with -ffp-contract=off.  What a kernel
// keeps to itself is its shape: what is unrolled, how many corners are in flight, which brackets it reuses.
//
// A table is any struct with the fields of the public ones: (cols, ax0, ax1, axk, n0, n1, nk) for a model grid packed
// [n0][n1][nk][Q], (bc, axT, axg, axf, axA, nT, ng, nf, nA, B) for a BC grid packed [nT][ng][nf][nA][B].  Internal.
#ifndef ISO_COMMON_GRID_INTERP_H
#define ISO_COMMON_GRID_INTERP_H

#include "grid_cell.h"

namespace {

// ---- the 3-D cell: corners 000 .. 111 of (ax0, ax1, axk), the last axis fastest; weight (f0 * f1) * fk ----

// off[j]: corner j from the cell's first node, in doubles; w[j]: its weight
__host__ __device__ inline void cell3_corners(int n1, int nk, int Q, double t0, double t1, double tk, int (&off)[8],
                                              double (&w)[8]) {
    const double u0 = 1 - t0, u1 = 1 - t1, uk = 1 - tk;
    const int sk = Q, s1 = nk * Q, s0 = n1 * nk * Q;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b0 = (j >> 2) & 1, b1 = (j >> 1) & 1, bk = j & 1;
        off[j] = b0 * s0 + b1 * s1 + bk * sk;
        w[j] = ((b0 ? t0 : u0) * (b1 ? t1 : u1)) * (bk ? tk : uk);
    }
}

template <class Table>
__host__ __device__ inline bool on_grid3(const Table& M, double x0, double x1, double xk) {
    return on_axis(M.ax0, M.n0, x0) && on_axis(M.ax1, M.n1, x1) && on_axis(M.axk, M.nk, xk);
}

// the three brackets and the corners; returns the cell's first node in doubles.  Inside the table for every x (bracket()
// stays on its axis); whether the cell counts is on_grid3()'s to say.
template <class Table>
__host__ __device__ inline int cell3_at(const Table& M, int Q, double x0, double x1, double xk, int (&off)[8],
                                        double (&w)[8]) {
    int i0, i1, ik;
    double t0, t1, tk;
    bracket(M.ax0, M.n0, x0, i0, t0);
    bracket(M.ax1, M.n1, x1, i1, t1);
    bracket(M.axk, M.nk, xk, ik, tk);
    cell3_corners(M.n1, M.nk, Q, t0, t1, tk, off, w);
    return ((i0 * M.n1 + i1) * M.nk + ik) * Q;
}

// The plain statement: v[q], q < Q, each accumulated from 0.0 over the corners in order; qnan() off the grid.
template <class Table>
__host__ __device__ inline void cell3(const Table& M, int Q, double x0, double x1, double xk, double* __restrict__ v) {
    if (!on_grid3(M, x0, x1, xk)) {
        for (int q = 0; q < Q; ++q) v[q] = qnan();
        return;
    }
    int off[8];
    double w[8];
    const double* __restrict__ p = M.cols + cell3_at(M, Q, x0, x1, xk, off, w);
    for (int q = 0; q < Q; ++q) v[q] = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double* __restrict__ c = p + off[j];
        for (int q = 0; q < Q; ++q) v[q] = v[q] + c[q] * w[j];
    }
}

// one corner of W adjacent columns into the accumulators; PAIR: two doubles per load (p is 16-byte aligned, W even)
template <int W, bool PAIR>
__device__ __forceinline__ void corner(const double* __restrict__ p, double w, double (&v)[W]) {
    if constexpr (PAIR) {
        const double2* __restrict__ p2 = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int j = 0; j < W / 2; ++j) {
            const double2 d = p2[j];
            v[2 * j] = v[2 * j] + d.x * w;
            v[2 * j + 1] = v[2 * j + 1] + d.y * w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = v[j] + p[j] * w;
    }
}

// W adjacent columns of a cell (p: its first node at the first of them), all eight corners in flight
template <int W, bool PAIR>
__device__ __forceinline__ void cell3_columns(const double* __restrict__ p, const int (&off)[8], const double (&w)[8],
                                              double (&v)[W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) corner<W, PAIR>(p + off[j], w[j], v);
}

// ---- the 4-D BC cell: corners 0000 .. 1111 of (T, g, f, A), A fastest; weight ((fT * fg) * ff) * fA ----

struct BcCell {                                 // where (T, g, f) sits: one set feeds every lookup along A
    int node;                                   // (iT, ig, jf, 0), band 0, in doubles
    double tT, tg, tf, uT, ug, uf;
};

template <class Table>
__host__ __device__ inline bool bc_on_grid(const Table& T, double xT, double xg, double xf) {
    return on_axis(T.axT, T.nT, xT) && on_axis(T.axg, T.ng, xg) && on_axis(T.axf, T.nf, xf);
}

// the three brackets; inside the table for every x, as cell3_at()
template <class Table>
__host__ __device__ inline BcCell bc_bracket(const Table& T, double xT, double xg, double xf) {
    BcCell c;
    int iT, ig, jf;
    bracket(T.axT, T.nT, xT, iT, c.tT);
    bracket(T.axg, T.ng, xg, ig, c.tg);
    bracket(T.axf, T.nf, xf, jf, c.tf);
    c.uT = 1 - c.tT, c.ug = 1 - c.tg, c.uf = 1 - c.tf;
    c.node = ((iT * T.ng + ig) * T.nf + jf) * (T.nA * T.B);
    return c;
}

// corner k = (bT bg bf) of the (T, g, f) cell: its weight (fT * fg) * ff ...
__host__ __device__ inline double bc_weight(const BcCell& c, int k) {
    const int bT = (k >> 2) & 1, bg = (k >> 1) & 1, bf = k & 1;
    return ((bT ? c.tT : c.uT) * (bg ? c.tg : c.ug)) * (bf ? c.tf : c.uf);
}

// ... and its row of nA * B doubles, in doubles from c.node
template <class Table>
__host__ __device__ inline int bc_offset(const Table& T, int k) {
    const int bT = (k >> 2) & 1, bg = (k >> 1) & 1, bf = k & 1;
    const int sf = T.nA * T.B, sg = T.nf * sf, sT = T.ng * sg;
    return bT * sT + bg * sg + bf * sf;
}

// The bands [b0, b0 + nb), nb <= CH, at (T, g, f, A): v[j] accumulated from 0.0 over the sixteen corners in order; qnan()
// off the grid.  The two slow bits as a loop: four corners of CH bands in flight at a time.
template <int CH, class Table>
__host__ __device__ inline void bc_chunk(const Table& T, double xT, double xg, double xf, double xA, int b0, int nb,
                                         double (&v)[CH]) {
    if (!(bc_on_grid(T, xT, xg, xf) && on_axis(T.axA, T.nA, xA))) {
#pragma unroll
        for (int j = 0; j < CH; ++j) v[j] = qnan();
        return;
    }
    const BcCell c = bc_bracket(T, xT, xg, xf);
    int iA;
    double tA;
    bracket(T.axA, T.nA, xA, iA, tA);
    const double uA = 1 - tA;
    const double* __restrict__ p0 = T.bc + (c.node + iA * T.B + b0);
#pragma unroll
    for (int j = 0; j < CH; ++j) v[j] = 0.0;
#pragma nounroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = kk * 2 + (m >> 1), bA = m & 1;
            const double w = bc_weight(c, k) * (bA ? tA : uA);
            const double* __restrict__ p = p0 + (bc_offset(T, k) + bA * T.B);
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (j < nb) v[j] = v[j] + p[j] * w;
        }
    }
}

}  // namespace

#endif
