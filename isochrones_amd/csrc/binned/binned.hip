// The hierarchical (population) likelihood of a catalog for a population density that is piecewise constant on a grid of
// bins over one or two columns, for gfx950: the stored chains compressed once to a table of B numbers per star, then per
// (hyper row, star) the contraction of that table with the row's cell heights.  See include/isochrones_amd_binned.h for the
// definitions, include/isochrones_amd_hier.h for the records and columns, DESIGN.md section 21 for the mapping and the
// resources.
//
// Three kernels, 256-thread workgroups (four wavefronts), float64:
//   k_binned_compress  one workgroup per star.  The records, the column descriptors and the edges are staged in LDS.  Pass 1:
//                      lane i evaluates the samples i, i + 256, ... (sample_term below, the host entry's own function) for
//                      the star's maximum and the bad and out counts.  Pass 2: the same samples a tile of 256 at a time; a
//                      lane stages (cell or -1, exp(c - mx)) in LDS, then lane b < B walks the tile in ascending order and
//                      adds what falls in cell b to its two register sums.  The walk's LDS reads are the same address in
//                      every lane: broadcasts.
//   k_binned_rows      one workgroup per (tile of ROW_TILE rows, block of 256 stars), lane = star: the tile's
//                      u = exp(lnh - hmx) and u * u in LDS, then per cell one load of A and A2 and eight multiplies and adds.
//                      A (row, star) whose s1 is below ISO_BINNED_RESCUE_BELOW is taken again by its lane after the tile's
//                      stores, with the star's own reference height (the header's rescue): rare, and no part of the loop.
//   k_binned_total     one workgroup per row: L and min_ess over the unmasked stars in a fixed order (common/hier_block.h, as
//                      k_hier_total).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "isochrones_amd_binned.h"
#include "../common/family_lnf.h"
#include "../common/chain_view.h"
#include "../common/hier_columns.h"
#include "../common/hier_block.h"

namespace {

constexpr int RT = ISO_BINNED_ROW_TILE;
constexpr int MAXB = ISO_BINNED_MAX_CELLS;
constexpr int MAXA = ISO_BINNED_MAX_AXES;
constexpr int MAX_EDGES = MAXB + 1 + 2;         // 64 x 1 bins: 65 + 2 edges
constexpr int FROZEN = -1;                      // Grid::role: else the axis number
constexpr int BAD = 1, OUT = 2;                 // sample_term's flag
static_assert(sizeof(Rec) == 72, "record layout");
static_assert(MAXB <= 64 && MAXA == 2, "the owners of the cells are the lanes of the first wavefront; two bin terms");

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

struct CArgs {
    DevCol col[MAXQ];
    Grid grid;
    const Rec* interim;
    const Rec* frozen;
    const double* edges;
    const double* extra;
    const int32_t* mask;
    double* A;
    double* A2;
    double* mx;
    int32_t* n_bad;
    int32_t* n_out;
    int32_t T, W, n_ens, ens_begin;
};

__global__ void __launch_bounds__(BLOCK) k_binned_compress(const CArgs A) {
    __shared__ Rec s_rec[2 * MAXQ];             // [q]: interim; [MAXQ + q]: frozen
    __shared__ DevCol s_col[MAXQ];
    __shared__ Grid s_grid;
    __shared__ int s_log[MAXQ];
    __shared__ double s_edge[MAX_EDGES];
    __shared__ double s_w[BLOCK];               // a tile's weights and cells, in the order of the samples
    __shared__ int s_cell[BLOCK];
    __shared__ double s_red[WAVES];
    __shared__ int s_cnt[2 * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = A.grid.Q, B = A.grid.B, W = A.W;
    const int s = A.ens_begin + (int)blockIdx.x;
    const size_t ld = (size_t)A.n_ens;

    if (A.mask && A.mask[s] == 0) {             // workgroup-uniform
        if (tid < B) {
            A.A[(size_t)tid * ld + s] = 0.0;
            A.A2[(size_t)tid * ld + s] = 0.0;
        }
        if (tid == 0) {
            A.mx[s] = qnan();
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
    double mx = neg_inf();
    int nbad = 0, nout = 0;
    for (int m = tid; m < M; m += BLOCK) {
        int cell, flag;
        const double c = sample_term(s_col, s_rec, s_rec + MAXQ, s_log, s_grid, s_edge, A.extra, s, W, M, m, cell, flag);
        nbad += flag == BAD ? 1 : 0;
        nout += flag == OUT ? 1 : 0;
        mx = cell >= 0 ? fmax(mx, c) : mx;
    }
    {
        const double v = wave_max(mx);
        const int nb = wave_sum_int(nbad), no = wave_sum_int(nout);
        if (lane == 0) {
            s_red[wave] = v;
            s_cnt[wave] = nb;
            s_cnt[WAVES + wave] = no;
        }
    }
    __syncthreads();
    mx = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
    if (tid == 0) {
        A.mx[s] = mx;
        A.n_bad[s] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        A.n_out[s] = ((s_cnt[WAVES] + s_cnt[WAVES + 1]) + s_cnt[WAVES + 2]) + s_cnt[WAVES + 3];
    }

    // pass 2; with mx = -inf no sample has a cell, so nothing is exponentiated
    double a1 = 0.0, a2 = 0.0;
    for (int m0 = 0; m0 < M; m0 += BLOCK) {     // the same trips in every lane: the barriers below
        const int m = m0 + tid;
        int cell = -1, flag;
        double wgt = 0.0;
        if (m < M) {
            const double c = sample_term(s_col, s_rec, s_rec + MAXQ, s_log, s_grid, s_edge, A.extra, s, W, M, m, cell, flag);
            wgt = cell >= 0 ? exp(c - mx) : 0.0;
        }
        s_cell[tid] = cell;
        s_w[tid] = wgt;
        __syncthreads();
        if (tid < B) {                          // the owner of cell tid: the tile's samples in ascending m
            const int n = min(BLOCK, M - m0);
            for (int i = 0; i < n; ++i) {
                const double v = s_w[i];
                const bool mine = s_cell[i] == tid;
                a1 = mine ? a1 + v : a1;
                a2 = mine ? a2 + v * v : a2;
            }
        }
        __syncthreads();
    }
    if (tid < B) {
        A.A[(size_t)tid * ld + s] = a1;
        A.A2[(size_t)tid * ld + s] = a2;
    }
}

// the contraction of one (row, star) taken again with the star's own reference height (the header's rescue): ref is the
// largest lnh_b over the cells the star has weight in.  Host and device run this one function
__host__ __device__ inline void rescue_pair(const double* A, const double* A2, size_t ld, int s, const double* row, int B,
                                            double mx, double lnM, double& ell, double& ess) {
    double ref = neg_inf();
    for (int b = 0; b < B; ++b) {
        const double l = row[b];
        if (A[(size_t)b * ld + s] > 0.0 && l > neg_inf()) ref = fmax(ref, l);       // a NaN is a cell of height 0
    }
    ell = neg_inf();
    ess = 0.0;
    if (!(ref > neg_inf())) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double a = A[(size_t)b * ld + s], l = row[b];
        if (a > 0.0 && l > neg_inf()) {
            const double u = exp(l - ref);
            s1 += u * a;
            s2 += (u * u) * A2[(size_t)b * ld + s];
        }
    }
    ell = ((mx + ref) + log(s1)) - lnM;
    ess = (s1 * s1) / s2;
}

struct RArgs {
    const double* A;
    const double* A2;
    const double* mx;
    const double* lnh;
    const int32_t* mask;
    double* ell;
    double* ess;
    int64_t M;
    int32_t B, H, n_ens, ens_begin, n_ens_out, nsb;
};

__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) k_binned_rows(const RArgs R) {
    __shared__ double s_u[RT * MAXB];           // [j][b]: exp(lnh - hmx) of row j of the tile
    __shared__ double s_uu[RT * MAXB];
    __shared__ double s_hmx[RT];
    const int tid = threadIdx.x;
    const int B = R.B, H = R.H;
    const int tile = (int)(blockIdx.x / (unsigned)R.nsb), sb = (int)(blockIdx.x - (unsigned)tile * R.nsb);
    const int h0 = tile * RT;
    const size_t ld = (size_t)R.n_ens;

    // a tile that reaches past H repeats the last row (computed, never written)
    if (tid < RT) {
        const double* row = R.lnh + (size_t)min(h0 + tid, H - 1) * B;
        double v = neg_inf();
        for (int b = 0; b < B; ++b) {
            const double l = row[b];
            v = fmax(v, (l == l) ? l : neg_inf());
        }
        s_hmx[tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < RT * B; i += BLOCK) {
        const int j = i / B, b = i - j * B;
        const double l = R.lnh[(size_t)min(h0 + j, H - 1) * B + b];
        const double u = (l > neg_inf()) ? exp(l - s_hmx[j]) : 0.0;     // a NaN is a cell of height 0
        s_u[j * MAXB + b] = u;
        s_uu[j * MAXB + b] = u * u;
    }
    __syncthreads();

    const int k = sb * BLOCK + tid;
    if (k >= R.n_ens_out) return;
    const int s = R.ens_begin + k;
    if (R.mask && R.mask[s] == 0) {
#pragma unroll
        for (int j = 0; j < RT; ++j)
            if (h0 + j < H) {
                R.ell[(size_t)(h0 + j) * ld + s] = qnan();
                R.ess[(size_t)(h0 + j) * ld + s] = qnan();
            }
        return;
    }
    double s1[RT], s2[RT];
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        s1[j] = 0.0;
        s2[j] = 0.0;
    }
    for (int b = 0; b < B; ++b) {
        const double a = R.A[(size_t)b * ld + s], a2 = R.A2[(size_t)b * ld + s];
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            s1[j] += s_u[j * MAXB + b] * a;
            s2[j] += s_uu[j * MAXB + b] * a2;
        }
    }
    const double mx = R.mx[s], lnM = log((double)R.M);
    unsigned again = 0u;                        // the rows of the tile whose s1 is below the rescue's threshold (0 included)
#pragma unroll
    for (int j = 0; j < RT; ++j)
        if (h0 + j < H) {
            const bool none = !(s1[j] > 0.0);
            R.ell[(size_t)(h0 + j) * ld + s] = none ? neg_inf() : ((mx + s_hmx[j]) + log(s1[j])) - lnM;
            R.ess[(size_t)(h0 + j) * ld + s] = none ? 0.0 : (s1[j] * s1[j]) / s2[j];
            again |= (s1[j] < ISO_BINNED_RESCUE_BELOW) ? (1u << j) : 0u;      // not a NaN
        }
    // rare: the pair is taken again from the tables, by the lane that owns it, in the same ascending order
    while (again) {
        const int j = __ffs(again) - 1;
        again &= again - 1u;
        double ell, ess;
        rescue_pair(R.A, R.A2, ld, s, R.lnh + (size_t)(h0 + j) * B, B, mx, lnM, ell, ess);
        R.ell[(size_t)(h0 + j) * ld + s] = ell;
        R.ess[(size_t)(h0 + j) * ld + s] = ess;
    }
}

__global__ void __launch_bounds__(BLOCK) k_binned_total(const double* __restrict__ ell, const double* __restrict__ ess,
                                                        const int32_t* __restrict__ mask, int n_ens,
                                                        double* __restrict__ L, double* __restrict__ min_ess) {
    row_total(ell, ess, mask, n_ens, L, min_ess);
}

// the checks of iso_binned_compress that need no look at device memory; fills G
int check_compress(const char* who, const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens,
                   int32_t W, int32_t ens_begin, int32_t n_ens_out, const Rec* interim, const Rec* frozen, int32_t n_frozen,
                   const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col, const int32_t* n_bins,
                   const double* edges, const double* A, const double* A2, const double* mx, const int32_t* n_bad,
                   const int32_t* n_out, Grid& G) {
    ChainShape s{layout, nsteps, n_ens, W, 1};
    s.ens_begin = ens_begin;
    s.n_ens_out = n_ens_out;
    const char* why = nullptr;
    if (!columns || !interim || !frozen || !axis_col || !n_bins || !edges || !A || !A2 || !mx || !n_bad || !n_out ||
        (n_frozen > 0 && !frozen_col))
        why = "null pointer";
    else if (Q < 1 || Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    // the kernel's tile counter runs to the first multiple of 256 at or past M, in an int
    else if (nsteps * (int64_t)W > INT32_MAX - BLOCK) why = "more than 2^31 - 257 samples per star (thin the chain)";
    else if (n_axes < 1 || n_axes > MAXA) why = "a grid has 1 or 2 binned axes";
    else if (n_frozen < 0 || n_frozen > Q) why = "n_frozen must be 0 to Q";
    else
        for (int q = 0; q < Q && !why; ++q) why = column_error(columns[q], W, ens_begin, n_ens_out);
    if (why) return fail(ISO_BINNED_ERR_INVALID, who, why);
    G = Grid{};
    G.Q = Q;
    G.n_axes = n_axes;
    int role[MAXQ] = {-2, -2, -2, -2};          // -2: not listed yet
    for (int a = 0; a < n_axes && !why; ++a) {
        const int q = axis_col[a];
        if (q < 0 || q >= Q) why = "a binned axis is no column (outside [0, Q))";
        else if (role[q] != -2) why = "a column is listed as a binned axis twice";
        else if (n_bins[a] < 1) why = "an axis needs at least 1 bin";
        else role[q] = a;
    }
    for (int i = 0; i < n_frozen && !why; ++i) {
        const int q = frozen_col[i];
        if (q < 0 || q >= Q) why = "a frozen column is no column (outside [0, Q))";
        else if (role[q] >= 0) why = "a column is listed both as a binned axis and as frozen";
        else if (role[q] == FROZEN) why = "a column is listed as frozen twice";
        else role[q] = FROZEN;
    }
    for (int q = 0; q < Q && !why; ++q)
        if (role[q] == -2) why = "a column is neither a binned axis nor frozen";
    if (!why) {
        const int64_t B = (int64_t)n_bins[0] * (n_axes == 2 ? n_bins[1] : 1);
        if (B > MAXB) why = "more than 64 cells";
    }
    if (why) return fail(ISO_BINNED_ERR_INVALID, who, why);
    for (int q = 0; q < MAXQ; ++q) G.role[q] = q < Q ? role[q] : FROZEN;
    G.nb[0] = n_bins[0];
    G.nb[1] = n_axes == 2 ? n_bins[1] : 1;
    G.e0[0] = 0;
    G.e0[1] = n_bins[0] + 1;
    G.mul[0] = G.nb[1];
    G.mul[1] = 1;
    G.B = G.nb[0] * G.nb[1];
    G.n_edges = n_bins[0] + 1 + (n_axes == 2 ? n_bins[1] + 1 : 0);
    return 0;
}

int check_lnlike(const char* who, const double* A, const double* A2, const double* mx, int32_t B, int32_t n_ens,
                 int32_t ens_begin, int32_t n_ens_out, int64_t M, const double* lnh, int32_t H, const double* ell,
                 const double* ess, const double* L, const double* min_ess) {
    const char* why = nullptr;
    if (!A || !A2 || !mx || !lnh || !ell || !ess) why = "null pointer";
    else if ((L == nullptr) != (min_ess == nullptr)) why = "L and min_ess go together (both or neither)";
    else if (B < 1 || B > MAXB) why = "B must be 1 to 64 cells";
    else if (H < 1) why = "H must be at least 1";
    else if (M < 1) why = "M must be at least 1";
    else if (n_ens < 1) why = "n_ens must be at least 1";
    else if (ens_begin < 0 || n_ens_out < 1 || (int64_t)ens_begin + n_ens_out > n_ens)
        why = "ensemble range [ens_begin, ens_begin + n_ens_out) must be non-empty and inside [0, n_ens)";
    else if ((int64_t)((n_ens_out + BLOCK - 1) / BLOCK) * ((H + RT - 1) / RT) > INT32_MAX)
        why = "more than 2^31 - 1 (row tile, star block) pairs (split the call)";
    return why ? fail(ISO_BINNED_ERR_INVALID, who, why) : 0;
}

}  // namespace

extern "C" {

const char* iso_binned_version(void) { return "isochrones_amd binned 1"; }

const char* iso_binned_last_error(void) { return g_err; }

int iso_binned_compress(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                        int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim, const iso_hier_record* frozen,
                        int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes, const int32_t* axis_col,
                        const int32_t* n_bins, const double* edges, const double* extra, const int32_t* mask, double* A,
                        double* A2, double* mx, int32_t* n_bad, int32_t* n_out, void* stream) {
    g_err[0] = 0;
    CArgs K;
    const int rc = check_compress("iso_binned_compress", columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim,
                                  frozen, n_frozen, frozen_col, n_axes, axis_col, n_bins, edges, A, A2, mx, n_bad, n_out,
                                  K.grid);
    if (rc) return rc;
    for (int q = 0; q < MAXQ; ++q) K.col[q] = dev_col(columns[q < Q ? q : 0], layout, W);
    K.interim = interim;
    K.frozen = frozen;
    K.edges = edges;
    K.extra = extra;
    K.mask = mask;
    K.A = A;
    K.A2 = A2;
    K.mx = mx;
    K.n_bad = n_bad;
    K.n_out = n_out;
    K.T = (int32_t)nsteps;
    K.W = W;
    K.n_ens = n_ens;
    K.ens_begin = ens_begin;
    hipLaunchKernelGGL(k_binned_compress, dim3((unsigned)n_ens_out), dim3(BLOCK), 0, (hipStream_t)stream, K);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_BINNED_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_binned_compress_host(const iso_hier_column* columns, int32_t Q, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                             int32_t ens_begin, int32_t n_ens_out, const iso_hier_record* interim,
                             const iso_hier_record* frozen, int32_t n_frozen, const int32_t* frozen_col, int32_t n_axes,
                             const int32_t* axis_col, const int32_t* n_bins, const double* edges, const double* extra,
                             const int32_t* mask, double* A, double* A2, double* mx, int32_t* n_bad, int32_t* n_out,
                             void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_binned_compress_host";
    Grid G;
    const int rc = check_compress(who, columns, Q, layout, nsteps, n_ens, W, ens_begin, n_ens_out, interim, frozen, n_frozen,
                                  frozen_col, n_axes, axis_col, n_bins, edges, A, A2, mx, n_bad, n_out, G);
    if (rc) return rc;
    for (int a = 0; a < n_axes; ++a)
        for (int k = 0; k <= G.nb[a]; ++k) {
            const double e = edges[G.e0[a] + k];
            if (!(e - e == 0.0) || (k > 0 && !(e > edges[G.e0[a] + k - 1])))
                return fail(ISO_BINNED_ERR_INVALID, who, "the edges of an axis must be finite and strictly increasing");
        }
    int logs[MAXQ] = {0, 0, 0, 0};
    for (int q = 0; q < Q; ++q) {
        const bool fr = G.role[q] == FROZEN;
        if (interim[q].kind < ISO_HIER_FLAT || interim[q].kind > ISO_HIER_TRUNCGAUSS ||
            (fr && (frozen[q].kind < ISO_HIER_FLAT || frozen[q].kind > ISO_HIER_TRUNCGAUSS)))
            return fail(ISO_BINNED_ERR_INVALID, who, "an interim or frozen record is not of the kinds 1 to 8");
        logs[q] = (needs_log(interim[q].kind) || (fr && needs_log(frozen[q].kind))) ? 1 : 0;
    }
    DevCol col[MAXQ];
    for (int q = 0; q < Q; ++q) col[q] = dev_col(columns[q], layout, W);
    const int M = (int)nsteps * W, B = G.B;
    const size_t ld = (size_t)n_ens;
    std::vector<double> c(M);
    std::vector<int> cell(M);
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        for (int b = 0; b < B; ++b) A[(size_t)b * ld + s] = A2[(size_t)b * ld + s] = 0.0;
        n_bad[s] = n_out[s] = 0;
        if (mask && mask[s] == 0) {
            mx[s] = qnan();
            continue;
        }
        double top = neg_inf();
        for (int m = 0; m < M; ++m) {
            int flag;
            c[m] = sample_term(col, interim, frozen, logs, G, edges, extra, s, W, M, m, cell[m], flag);
            n_bad[s] += flag == BAD ? 1 : 0;
            n_out[s] += flag == OUT ? 1 : 0;
            if (cell[m] >= 0) top = fmax(top, c[m]);
        }
        mx[s] = top;
        for (int m = 0; m < M; ++m)
            if (cell[m] >= 0) {
                const double v = exp(c[m] - top);
                A[(size_t)cell[m] * ld + s] += v;
                A2[(size_t)cell[m] * ld + s] += v * v;
            }
    }
    return 0;
}

int iso_binned_lnlike(const double* A, const double* A2, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin,
                      int32_t n_ens_out, int64_t M, const double* lnh, int32_t H, const int32_t* mask, double* ell,
                      double* ess, double* L, double* min_ess, void* stream) {
    g_err[0] = 0;
    const int rc = check_lnlike("iso_binned_lnlike", A, A2, mx, B, n_ens, ens_begin, n_ens_out, M, lnh, H, ell, ess, L, min_ess);
    if (rc) return rc;
    RArgs R;
    R.A = A;
    R.A2 = A2;
    R.mx = mx;
    R.lnh = lnh;
    R.mask = mask;
    R.ell = ell;
    R.ess = ess;
    R.M = M;
    R.B = B;
    R.H = H;
    R.n_ens = n_ens;
    R.ens_begin = ens_begin;
    R.n_ens_out = n_ens_out;
    R.nsb = (n_ens_out + BLOCK - 1) / BLOCK;
    const unsigned blocks = (unsigned)R.nsb * (unsigned)((H + RT - 1) / RT);
    hipLaunchKernelGGL(k_binned_rows, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_BINNED_ERR_HIP, hipGetErrorString(e));
    if (L) {
        hipLaunchKernelGGL(k_binned_total, dim3((unsigned)H), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)ell,
                           (const double*)ess, mask, (int)n_ens, L, min_ess);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(ISO_BINNED_ERR_HIP, hipGetErrorString(e));
    }
    return 0;
}

int iso_binned_lnlike_host(const double* A, const double* A2, const double* mx, int32_t B, int32_t n_ens, int32_t ens_begin,
                           int32_t n_ens_out, int64_t M, const double* lnh, int32_t H, const int32_t* mask, double* ell,
                           double* ess, double* L, double* min_ess, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_binned_lnlike_host";
    const int rc = check_lnlike(who, A, A2, mx, B, n_ens, ens_begin, n_ens_out, M, lnh, H, ell, ess, L, min_ess);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)H * B; ++i)
        if (lnh[i] == HUGE_VAL) return fail(ISO_BINNED_ERR_INVALID, who, "a log cell density is +inf");
    const size_t ld = (size_t)n_ens;
    const double lnM = log((double)M);
    std::vector<double> u(B), uu(B);
    for (int h = 0; h < H; ++h) {
        double hmx = neg_inf();
        for (int b = 0; b < B; ++b) {
            const double l = lnh[(size_t)h * B + b];
            hmx = fmax(hmx, (l == l) ? l : neg_inf());
        }
        for (int b = 0; b < B; ++b) {
            const double l = lnh[(size_t)h * B + b];
            u[b] = (l > neg_inf()) ? exp(l - hmx) : 0.0;
            uu[b] = u[b] * u[b];
        }
        for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
            if (mask && mask[s] == 0) {
                ell[(size_t)h * ld + s] = ess[(size_t)h * ld + s] = qnan();
                continue;
            }
            double s1 = 0.0, s2 = 0.0;
            for (int b = 0; b < B; ++b) {
                s1 += u[b] * A[(size_t)b * ld + s];
                s2 += uu[b] * A2[(size_t)b * ld + s];
            }
            const bool none = !(s1 > 0.0);
            ell[(size_t)h * ld + s] = none ? neg_inf() : ((mx[s] + hmx) + log(s1)) - lnM;
            ess[(size_t)h * ld + s] = none ? 0.0 : (s1 * s1) / s2;
            if (s1 < ISO_BINNED_RESCUE_BELOW)
                rescue_pair(A, A2, ld, s, lnh + (size_t)h * B, B, mx[s], lnM, ell[(size_t)h * ld + s],
                            ess[(size_t)h * ld + s]);
        }
    }
    if (L) row_totals_host(ell, ess, mask, n_ens, H, L, min_ess);
    return 0;
}

}  // extern "C"
