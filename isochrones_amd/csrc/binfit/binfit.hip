// The moments of the stars' posterior cell probabilities under a binned population density for gfx950: per hyper row the
// expected number of stars in every cell and the sum over the stars of the outer products of their cell probabilities,
// from the per-star tables of libiso_binned.so.  See include/isochrones_amd_binfit.h for the definition and the summation
// order, DESIGN.md section 24 for the mapping and the resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64, after the plan of k_select_partial / k_select_total:
//   k_binfit_partial  one workgroup per (chunk of ISO_BINFIT_CHUNK stars, hyper row).  The row's u = exp(lnh - hmx) is
//                     staged in LDS once.  The chunk is taken a tile of ISO_BINFIT_TILE stars at a time: lanes run along
//                     the stars when they load A (consecutive doubles of a cell's row), the tile's p[star][cell] is staged
//                     in LDS, and then every output's one owner lane walks the tile's stars in ascending order: lane 64 + b
//                     the count of cell b, lane k < 253 the pairs of block k of 3 x 3 cells (six 64-bit LDS reads for
//                     nine products a star; one pair a read pair would be eighteen).  A tile row
//                     is LDP = 65 doubles: at the same star the 64 cells fall into the 64 banks two by two, which is what a
//                     64-bit read allows, and at the same cell (the staging writes) consecutive stars are 130 words apart,
//                     again two a bank; with a row of 64 doubles every star of a cell would share one bank.  The pad, column
//                     64 of row b, keeps cell b's height as a mantissa for the rescue of the header (split_m below).
//   k_binfit_total    one workgroup per row: every output's owner adds the chunks in ascending order, a pair's sum goes to
//                     both halves of C, and the chunks' live counts are added.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "isochrones_amd_binfit.h"
#include "../common/last_error.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int MAXB = ISO_BINNED_MAX_CELLS;
constexpr int CHUNK = ISO_BINFIT_CHUNK;
constexpr int TILE = ISO_BINFIT_TILE;
constexpr int LDP = MAXB + 1;                   // doubles per star of the tile in LDS (see above)
constexpr int SIDE = 3;                         // a lane owns the pairs of SIDE x SIDE cells: 9
constexpr int CPW = MAXB / WAVES;               // cells a wavefront stages per star: 16
static_assert(TILE == 64, "one wavefront adds the tile's s1, a lane a star");
static_assert(CHUNK % TILE == 0, "a chunk is whole tiles");
static_assert(MAXB % WAVES == 0, "the wavefronts share the cells evenly");
static_assert(((MAXB + SIDE - 1) / SIDE) * ((MAXB + SIDE - 1) / SIDE + 1) / 2 <= BLOCK, "a block of pairs per lane");

__host__ __device__ inline double neg_inf() { return -HUGE_VAL; }
__host__ __device__ inline int n_chunks(int n_ens) { return (n_ens + CHUNK - 1) / CHUNK; }
__host__ __device__ inline int n_pairs(int B) { return B * (B + 1) / 2; }

// pair k of the upper triangle, numbered row by row: (b, b2) with b <= b2
__host__ __device__ inline void pair_of(int k, int B, int& b, int& b2) {
    b = 0;
    for (; k >= B - b; ++b) k -= B - b;
    b2 = b + k;
}

// the number of the pair (b, b2), b <= b2
__host__ __device__ inline int pair_number(int b, int b2, int B) { return b * B - b * (b - 1) / 2 + (b2 - b); }

constexpr int NO_TERM = INT32_MIN;              // the largest power of two of a star without weight under the row
constexpr double LN2_HI = 0x1.62e42feep-1;      // ln 2 in two parts: k * LN2_HI is exact for |k| < 2^21
constexpr double LN2_LO = 0x1.a39ef35793c76p-33;

// u = exp(l - hmx) as m * 2^k for the header's rescue: k = rint((l - hmx) / ln 2), at least -2^30; m = u / 2^k (exact) where
// u is a normal number, the exp of the rest where it is not; m is in [0.70, 1.42], or 0.0 for a cell of height 0 (and for one
// more than 2^30 powers of two below the row's top)
__host__ __device__ inline int split_k(double l, double hmx, double& kd) {
    kd = fmax(rint((l - hmx) * 1.4426950408889634), -1073741824.0);
    return (int)kd;
}

__host__ __device__ inline double split_m(double l, double hmx, double u) {
    if (!(l > neg_inf())) return 0.0;
    double kd;
    const int k = split_k(l, hmx, kd);
    return (u >= 0x1p-1022) ? ldexp(u, -k) : exp(((l - hmx) - kd * LN2_HI) - kd * LN2_LO);
}

// the header's rescue of one star under one row: p_b = m_b * 2^(k_b - kmax) * A[b][s] with 2^kmax the largest power of two
// over the cells the star has weight in, written to p[0 .. B); returns their sum over ascending b from 0.0 (0.0: no such
// cell).  m[b * stride]: the row's split_m.  Host and device run this one function
__host__ __device__ inline double rescue_star(const double* A, size_t ld, size_t s, const double* row, double hmx,
                                              const double* m, int stride, int B, double* p) {
    double kd;
    int kmax = NO_TERM;
#pragma unroll 1
    for (int b = 0; b < B; ++b)
        if (A[(size_t)b * ld + s] > 0.0 && m[b * stride] > 0.0) kmax = max(kmax, split_k(row[b], hmx, kd));
    double s1 = 0.0;
#pragma unroll 1
    for (int b = 0; b < B; ++b) {
        const double a = A[(size_t)b * ld + s], mb = m[b * stride];
        const double v = (a > 0.0 && mb > 0.0) ? ldexp(mb, split_k(row[b], hmx, kd) - kmax) * a : 0.0;
        p[b] = v;
        s1 += v;
    }
    return s1;
}

// the workspace: [H][nc][B + NP] doubles (NP = 0 without pairs), then [H][nc] int32 live counts
struct Args {
    const double* A;
    const double* lnh;
    const int32_t* mask;
    double* ws;
    int32_t B, n_ens, H, nc, pairs;
};

__global__ void __launch_bounds__(BLOCK) k_binfit_partial(const Args P) {
    __shared__ double s_p[TILE * LDP];          // [star of the tile][cell]
    __shared__ double s_u[MAXB];
    __shared__ double s_s1[TILE];               // a live star's s1, 0.0 for a star that is not live
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = P.B, nc = P.nc;
    const int h = (int)(blockIdx.x / (unsigned)nc), chunk = (int)(blockIdx.x - (unsigned)h * nc);
    const int NP = P.pairs ? n_pairs(B) : 0;
    const size_t ld = (size_t)P.n_ens;

    // the row's heights (isochrones_amd_binned.h's u: a NaN is a cell of height 0)
    const double* row = P.lnh + (size_t)h * B;
    double hmx = neg_inf();
    for (int b = 0; b < B; ++b) {
        const double l = row[b];
        hmx = fmax(hmx, (l == l) ? l : neg_inf());
    }
    if (tid < B) {
        const double l = row[tid];
        s_u[tid] = (l > neg_inf()) ? exp(l - hmx) : 0.0;
        s_p[tid * LDP + MAXB] = split_m(l, hmx, s_u[tid]);           // for the rescue, in the tile's pad column
    }
    // the lane's block of pairs: the cells [SIDE * I, SIDE * I + SIDE) x [SIDE * J, SIDE * J + SIDE), I <= J, the blocks
    // numbered row by row.  A cell past B is read as cell B - 1 (computed, never written)
    const int G = (B + SIDE - 1) / SIDE;
    const bool has_block = NP > 0 && tid < G * (G + 1) / 2;
    int I = 0, J = 0;
    if (has_block) pair_of(tid, G, I, J);
    int ri[SIDE], ci[SIDE];
#pragma unroll
    for (int i = 0; i < SIDE; ++i) {
        ri[i] = min(SIDE * I + i, B - 1);
        ci[i] = min(SIDE * J + i, B - 1);
    }
    // cell b's count belongs to lane 64 + b: wavefront 1, since wavefront 0 adds the tiles' s1
    const bool has_cell = wave == 1 && lane < B;
    double accN = 0.0, acc[SIDE][SIDE];
#pragma unroll
    for (int i = 0; i < SIDE; ++i)
#pragma unroll
        for (int j = 0; j < SIDE; ++j) acc[i][j] = 0.0;
    int nlive = 0;                              // wavefront 0 counts

    const int s0 = chunk * CHUNK;
    const int n = min(CHUNK, P.n_ens - s0);     // stars of this chunk, at least 1
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int nt = min(TILE, n - t0);
        const int s = s0 + t0 + lane;
        const bool in = lane < nt;
        // the lane's star, the cells wave, wave + 4, ...: every load issued before the first product
        double a[CPW];
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int b = wave + j * WAVES;
            a[j] = (b < B && in) ? P.A[(size_t)b * ld + (size_t)s] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int b = wave + j * WAVES;
            if (b < B) s_p[lane * LDP + b] = s_u[b] * a[j];             // 0.0 past the chunk's end
        }
        __syncthreads();
        if (wave == 0) {
            double s1 = 0.0;
#pragma unroll 8
            for (int b = 0; b < B; ++b) s1 += s_p[lane * LDP + b];
            const bool on = in && (!P.mask || P.mask[s] != 0);
            bool live = on && s1 > 0.0;
            // rare: a star whose s1 is below the threshold (0 included) is taken again relative to its own largest height
            if (__ballot(on && s1 < ISO_BINNED_RESCUE_BELOW) != 0ull) {             // the same branch for the wavefront
                if (on && s1 < ISO_BINNED_RESCUE_BELOW) {                           // not a NaN
                    s1 = rescue_star(P.A, ld, (size_t)s, row, hmx, s_p + MAXB, LDP, B, s_p + lane * LDP);
                    live = s1 > 0.0;
                }
            }
            s_s1[lane] = live ? s1 : 0.0;
            nlive += __popcll(__ballot(live));
        }
        __syncthreads();
        const double d = s_s1[lane];
#pragma unroll 2
        for (int b = wave; b < B; b += WAVES) {         // not unrolled further: sixteen divisions in flight cost registers
            const double v = s_p[lane * LDP + b];
            s_p[lane * LDP + b] = (d > 0.0) ? v / d : 0.0;
        }
        __syncthreads();
        if (has_cell) {
#pragma unroll 8
            for (int t = 0; t < nt; ++t) accN += s_p[t * LDP + lane];
        }
        if (has_block) {
#pragma unroll 2
            for (int t = 0; t < nt; ++t) {
                const double* pt = s_p + t * LDP;
                double r[SIDE], c[SIDE];
#pragma unroll
                for (int i = 0; i < SIDE; ++i) {
                    r[i] = pt[ri[i]];
                    c[i] = pt[ci[i]];
                }
#pragma unroll
                for (int i = 0; i < SIDE; ++i)
#pragma unroll
                    for (int j = 0; j < SIDE; ++j) {
                        const double w = r[i] * c[j];
                        acc[i][j] += w;
                    }
            }
        }
        __syncthreads();
    }

    const size_t stride = (size_t)(B + NP);
    double* out = P.ws + ((size_t)h * nc + chunk) * stride;
    if (has_cell) out[lane] = accN;
    if (has_block) {
#pragma unroll
        for (int i = 0; i < SIDE; ++i)
#pragma unroll
            for (int j = 0; j < SIDE; ++j) {
                const int b = SIDE * I + i, b2 = SIDE * J + j;
                if (b <= b2 && b2 < B) out[B + pair_number(b, b2, B)] = acc[i][j];
            }
    }
    if (tid == 0) ((int32_t*)(P.ws + (size_t)P.H * nc * stride))[(size_t)h * nc + chunk] = nlive;
}

__global__ void __launch_bounds__(BLOCK) k_binfit_total(const double* __restrict__ ws, int B, int nc, int H, int pairs,
                                                        double* __restrict__ N, double* __restrict__ C,
                                                        int32_t* __restrict__ n_live) {
    const int tid = threadIdx.x;
    const int h = blockIdx.x;
    const int NP = pairs ? n_pairs(B) : 0;
    const size_t stride = (size_t)(B + NP);
    const double* base = ws + (size_t)h * nc * stride;
    for (int o = tid; o < B + NP; o += BLOCK) {
        double a = 0.0;
        for (int c = 0; c < nc; ++c) a += base[(size_t)c * stride + o];
        if (o < B) {
            N[(size_t)h * B + o] = a;
        } else {
            int b, b2;
            pair_of(o - B, B, b, b2);
            C[((size_t)h * B + b) * B + b2] = a;
            C[((size_t)h * B + b2) * B + b] = a;
        }
    }
    if (tid == 0) {
        const int32_t* lv = (const int32_t*)(ws + (size_t)H * nc * stride) + (size_t)h * nc;
        int tot = 0;
        for (int c = 0; c < nc; ++c) tot += lv[c];
        n_live[h] = tot;
    }
}

int check_args(const char* who, const double* A, int32_t B, int32_t n_ens, const double* lnh, int32_t H, const double* N,
               const int32_t* n_live, const double* workspace, bool need_workspace) {
    const char* why = nullptr;
    if (!A || !lnh || !N || !n_live || (need_workspace && !workspace)) why = "null pointer";
    else if (B < 1 || B > MAXB) why = "B must be 1 to 64 cells";
    else if (n_ens < 1) why = "n_ens must be at least 1";
    else if (H < 1) why = "H must be at least 1";
    else if ((int64_t)n_chunks(n_ens) * H > INT32_MAX) why = "more than 2^31 - 1 (chunk, row) pairs (split the rows)";
    return why ? fail(ISO_BINFIT_ERR_INVALID, who, why) : 0;
}

}  // namespace

extern "C" {

const char* iso_binfit_version(void) { return "isochrones_amd binfit 1"; }

const char* iso_binfit_last_error(void) { return g_err; }

int64_t iso_binfit_workspace_doubles(int32_t B, int32_t n_ens, int32_t H, int with_pairs) {
    if (B < 1 || B > MAXB || n_ens < 1 || H < 1) return 0;
    const int64_t cells = (int64_t)H * n_chunks(n_ens);
    return cells * (B + (with_pairs ? n_pairs(B) : 0)) + (cells + 1) / 2;
}

int iso_binfit_moments(const double* A, int32_t B, int32_t n_ens, const double* lnh, int32_t H, const int32_t* mask,
                       double* N, double* C, int32_t* n_live, double* workspace, void* stream) {
    g_err[0] = 0;
    const int rc = check_args("iso_binfit_moments", A, B, n_ens, lnh, H, N, n_live, workspace, true);
    if (rc) return rc;
    Args P;
    P.A = A;
    P.lnh = lnh;
    P.mask = mask;
    P.ws = workspace;
    P.B = B;
    P.n_ens = n_ens;
    P.H = H;
    P.nc = n_chunks(n_ens);
    P.pairs = C ? 1 : 0;
    hipLaunchKernelGGL(k_binfit_partial, dim3((unsigned)P.nc * (unsigned)H), dim3(BLOCK), 0, (hipStream_t)stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_BINFIT_ERR_HIP, hipGetErrorString(e));
    hipLaunchKernelGGL(k_binfit_total, dim3((unsigned)H), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)workspace,
                       (int)B, (int)P.nc, (int)H, (int)P.pairs, N, C, n_live);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_BINFIT_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_binfit_moments_host(const double* A, int32_t B, int32_t n_ens, const double* lnh, int32_t H, const int32_t* mask,
                            double* N, double* C, int32_t* n_live, double* workspace, void* stream) {
    (void)workspace;
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_binfit_moments_host";
    const int rc = check_args(who, A, B, n_ens, lnh, H, N, n_live, workspace, false);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)H * B; ++i)
        if (lnh[i] == HUGE_VAL) return fail(ISO_BINFIT_ERR_INVALID, who, "a log cell density is +inf");
    const size_t ld = (size_t)n_ens;
    std::vector<double> u(B), p(B), um(B);
    for (int h = 0; h < H; ++h) {
        double hmx = neg_inf();
        for (int b = 0; b < B; ++b) {
            const double l = lnh[(size_t)h * B + b];
            hmx = fmax(hmx, (l == l) ? l : neg_inf());
        }
        for (int b = 0; b < B; ++b) {
            const double l = lnh[(size_t)h * B + b];
            u[b] = (l > neg_inf()) ? exp(l - hmx) : 0.0;
            um[b] = split_m(l, hmx, u[b]);
        }
        double* Nh = N + (size_t)h * B;
        double* Ch = C ? C + (size_t)h * B * B : nullptr;
        for (int b = 0; b < B; ++b) Nh[b] = 0.0;
        if (Ch)
            for (int i = 0; i < B * B; ++i) Ch[i] = 0.0;
        int live = 0;
        for (int s = 0; s < n_ens; ++s) {
            if (mask && mask[s] == 0) continue;
            double s1 = 0.0;
            for (int b = 0; b < B; ++b) {
                p[b] = u[b] * A[(size_t)b * ld + s];
                s1 += p[b];
            }
            if (s1 < ISO_BINNED_RESCUE_BELOW) s1 = rescue_star(A, ld, (size_t)s, lnh + (size_t)h * B, hmx, um.data(), 1, B, p.data());
            if (!(s1 > 0.0)) continue;
            ++live;
            for (int b = 0; b < B; ++b) {
                p[b] = p[b] / s1;
                Nh[b] += p[b];
            }
            if (Ch)
                for (int b = 0; b < B; ++b)
                    for (int b2 = 0; b2 < B; ++b2) {
                        const double w = p[b] * p[b2];
                        Ch[(size_t)b * B + b2] += w;
                    }
        }
        n_live[h] = live;
    }
    return 0;
}

}  // extern "C"
