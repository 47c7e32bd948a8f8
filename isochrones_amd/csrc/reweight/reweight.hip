// The population-informed posterior of every star of a catalog from its stored chain for gfx950: per sample the weight
// under the hyper rows of a fitted population, per star the weights' sum and effective sample size, per (star, value
// column) the weighted mean, standard deviation and quantiles.  See include/isochrones_amd_reweight.h for the definition
// and the summation order, DESIGN.md section 19 for the mapping and the resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64:
//   k_reweight_weights  one workgroup per star.  The interim records, a tile of ROW_TILE hyper rows' records and the
//                       star's ln_norm of those rows are staged in LDS (every lane reads the same address: a
//                       broadcast).  Lanes run along the sample axis m = t * W + w, so consecutive lanes read consecutive
//                       walkers of the parameter-major storage; per sample x, ln x (only where a record of the column
//                       needs it), the interim term and the bad-sample test are computed once, then the tile's rows run
//                       innermost and add into one register.  More rows than a tile: u waits in `weights` between tiles.
//   k_reweight_summary  one workgroup per (star, value column): two lane-strided passes over (y, u) for the moments, then
//                       per probability a 16-pass weighted radix select (4 bits a pass, 16 bins a lane in registers,
//                       filled by a chain of selects: a lane's own LDS column instead was measured slower).
//                       (y, u) are read from memory in every pass: a star's 16 * M bytes stay in the cache.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "isochrones_amd_reweight.h"
#include "../common/family_lnf.h"
#include "../common/chain_view.h"
#include "../common/hier_columns.h"
#include "../common/wave_reduce.h"

namespace {

constexpr int BLOCK = 256;                      // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int TILE = ISO_REWEIGHT_ROW_TILE;
constexpr int MAXV = ISO_REWEIGHT_MAX_VALUES;
constexpr int MAXK = ISO_REWEIGHT_MAX_PROBS;
constexpr int NBIN = 16, DIGIT_BITS = 4, NPASS = 64 / DIGIT_BITS;
constexpr uint64_t SIGN = 0x8000000000000000ULL;
static_assert(sizeof(Rec) == 72, "record layout");

struct WArgs {
    DevCol col[MAXQ];
    const Rec* interim;
    const Rec* rows;
    const double* ln_norm;
    const int32_t* mask;
    double* weights;
    double* wsum;
    double* ess;
    int32_t* n_bad;
    int32_t Q, T, W, H, n_ens, ens_begin;
};

struct SArgs {
    DevCol val[MAXV];
    double probs[MAXK];
    const double* weights;
    const int32_t* mask;
    double* mean;
    double* sd;
    double* quant;
    int32_t* n_nan;
    int32_t V, K, T, W, ens_begin, pad;
};

// the order-preserving key of a double that is not NaN; -0 has been made +0 by the caller (y + 0.0)
__host__ __device__ inline uint64_t key_of(double y) {
    union { double d; uint64_t u; } x;
    x.d = y;
    return (x.u & SIGN) ? ~x.u : (x.u ^ SIGN);
}

__host__ __device__ inline double value_of(uint64_t key) {
    union { double d; uint64_t u; } x;
    x.u = (key & SIGN) ? (key ^ SIGN) : ~key;
    return x.d;
}

__global__ void __launch_bounds__(BLOCK) k_reweight_weights(const WArgs A) {
    __shared__ Rec s_rec[(TILE + 1) * MAXQ];    // [0][q]: interim; [1 + j][q]: row j of the tile
    __shared__ double s_ln[TILE];               // the star's ln_norm of the tile's rows
    __shared__ DevCol s_col[MAXQ];
    __shared__ double s_red[2 * WAVES];
    __shared__ int s_bad[WAVES];
    __shared__ int s_log[MAXQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = A.Q, W = A.W, H = A.H;
    const int s = A.ens_begin + (int)blockIdx.x;
    const size_t ld = (size_t)A.n_ens;

    if (A.mask && A.mask[s] == 0) {             // workgroup-uniform
        if (tid == 0) {
            A.wsum[s] = qnan();
            A.ess[s] = qnan();
            A.n_bad[s] = 0;
        }
        return;
    }

    constexpr int RW = (int)(sizeof(Rec) / 4);
    {
        uint32_t* dst = (uint32_t*)s_rec;
        const uint32_t* src0 = (const uint32_t*)A.interim;
        for (int i = tid; i < Q * RW; i += BLOCK) dst[i] = src0[i];
        if (tid == 0) {
            s_col[0] = A.col[0];
            s_col[1] = A.col[1];
            s_col[2] = A.col[2];
            s_col[3] = A.col[3];
        }
    }

    const int M = A.T * W;
    double* const u_row = A.weights + (size_t)blockIdx.x * (size_t)M;
    double s1 = 0.0, s2 = 0.0;
    int nbad = 0;
    for (int h0 = 0; h0 < H; h0 += TILE) {
        const int nrows = min(TILE, H - h0);
        const bool first = h0 == 0, last = h0 + TILE >= H;
        __syncthreads();                        // the tile before this one has been read by every lane
        {
            uint32_t* dst = (uint32_t*)s_rec;
            for (int i = tid; i < nrows * Q * RW; i += BLOCK) {
                const int j = i / (Q * RW), k = i - j * (Q * RW);
                dst[(1 + j) * MAXQ * RW + k] = ((const uint32_t*)(A.rows + (size_t)(h0 + j) * Q))[k];
            }
            for (int j = tid; j < nrows; j += BLOCK) s_ln[j] = A.ln_norm[(size_t)(h0 + j) * ld + s];
        }
        __syncthreads();
        if (tid < Q) {
            int need = 0;
            for (int j = 0; j <= nrows; ++j) need |= needs_log(s_rec[j * MAXQ + tid].kind) ? 1 : 0;
            s_log[tid] = need;
        }
        __syncthreads();

        for (int m = tid; m < M; m += BLOCK) {
            const int t = m / W, w = m - t * W;
            // the sample's columns stay in registers; q is a run-time index (one inlined family evaluation, not four), so
            // a column is put in and taken out by a chain of selects, not by a dynamic register index
            double x[MAXQ], lx[MAXQ], l0[MAXQ];
#pragma unroll
            for (int k = 0; k < MAXQ; ++k) x[k] = lx[k] = l0[k] = 0.0;
            bool good = true;
#pragma unroll 1
            for (int q = 0; q < Q; ++q) {
                const double xv = load(s_col[q], s, W, t, w);
                const double lv = s_log[q] ? log(xv) : 0.0;         // workgroup-uniform choice
                const double l = lnf(s_rec[q], xv, lv);
                good = good && xv == xv && l == l && l != neg_inf();
#pragma unroll
                for (int k = 0; k < MAXQ; ++k) {
                    x[k] = (k == q) ? xv : x[k];
                    lx[k] = (k == q) ? lv : lx[k];
                    l0[k] = (k == q) ? l : l0[k];
                }
            }
            double u = 0.0;
            if (good) {
                u = first ? 0.0 : u_row[m];     // written by this lane in the tile before
                for (int j = 0; j < nrows; ++j) {
                    double r = 0.0;
#pragma unroll 1
                    for (int q = 0; q < Q; ++q) {
                        double xv = x[0], lv = lx[0], l = l0[0];
#pragma unroll
                        for (int k = 1; k < MAXQ; ++k) {
                            xv = (k == q) ? x[k] : xv;
                            lv = (k == q) ? lx[k] : lv;
                            l = (k == q) ? l0[k] : l;
                        }
                        double lf = lnf(s_rec[(1 + j) * MAXQ + q], xv, lv);
                        lf = (lf == lf) ? lf : neg_inf();
                        const double d = lf - l;
                        r = (q == 0) ? d : r + d;
                    }
                    const double ln = s_ln[j];
                    const bool live = ln == ln && ln != neg_inf();
                    const double th = exp(r - ln);
                    u += live ? th : 0.0;
                }
            }
            u_row[m] = u;
            if (last) {
                nbad += good ? 0 : 1;
                s1 += u;
                s2 += u * u;
            }
        }
    }

    const double a = wave_sum(s1), b = wave_sum(s2);
    const int nb = wave_sum_int(nbad);
    if (lane == 0) {
        s_red[wave] = a;
        s_red[WAVES + wave] = b;
        s_bad[wave] = nb;
    }
    __syncthreads();
    if (tid == 0) {
        const double S1 = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        const double S2 = ((s_red[WAVES] + s_red[WAVES + 1]) + s_red[WAVES + 2]) + s_red[WAVES + 3];
        A.wsum[s] = S1;
        A.ess[s] = (S1 == 0.0) ? 0.0 : (S1 * S1) / S2;
        A.n_bad[s] = ((s_bad[0] + s_bad[1]) + s_bad[2]) + s_bad[3];
    }
}

// the workgroup's sum in the header's order, in every lane; s_red is free again on return
__device__ __forceinline__ double block_sum(double v, double* s_red, int lane, int wave) {
    v = wave_sum(v);
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    const double out = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return out;
}

// (y, u) of sample m of a star as every pass sees it: a NaN y (returns true) has weight 0 and the value +0.0; -0 is +0
__device__ __forceinline__ bool load_yu(const double* yb, const DevCol& c, const double* u_row, int W, int m, double& y,
                                        double& u) {
    const int t = m / W, w = m - t * W;
    const double y0 = yb[(int64_t)t * c.st_t + (int64_t)w * c.st_w];
    const bool isn = y0 != y0;
    y = isn ? 0.0 : y0 + 0.0;
    u = isn ? 0.0 : u_row[m];
    return isn;
}

__global__ void __launch_bounds__(BLOCK) k_reweight_summary(const SArgs A) {
    __shared__ double s_red[NBIN * WAVES];
    __shared__ int s_cnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = A.V, K = A.K, W = A.W;
    const int star = (int)(blockIdx.x / (unsigned)V), v = (int)(blockIdx.x - (unsigned)star * V);
    const int s = A.ens_begin + star;
    const size_t at = (size_t)s * V + v;

    if (A.mask && A.mask[s] == 0) {             // workgroup-uniform
        if (tid == 0) {
            A.mean[at] = qnan();
            A.sd[at] = qnan();
            A.n_nan[at] = 0;
        }
        if (tid < K) A.quant[at * K + tid] = qnan();
        return;
    }

    const DevCol c = A.val[v];
    const double* const yb = c.base + (int64_t)(s - c.first) * W * c.st_w;
    const int M = A.T * W;
    const double* const u_row = A.weights + (size_t)star * (size_t)M;

    double a = 0.0, b = 0.0;
    int nn = 0;
    for (int m = tid; m < M; m += BLOCK) {
        double y, u;
        nn += load_yu(yb, c, u_row, W, m, y, u) ? 1 : 0;
        a += u;
        b += u * y;
    }
    const double tot = block_sum(a, s_red, lane, wave);
    const double sy = block_sum(b, s_red, lane, wave);
    nn = wave_sum_int(nn);
    if (lane == 0) s_cnt[wave] = nn;
    __syncthreads();
    if (tid == 0) A.n_nan[at] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];

    if (!(tot > 0.0) || tot == HUGE_VAL) {      // workgroup-uniform: nothing to summarise
        if (tid == 0) {
            A.mean[at] = qnan();
            A.sd[at] = qnan();
        }
        if (tid < K) A.quant[at * K + tid] = qnan();
        return;
    }

    const double mean = sy / tot;
    double q2 = 0.0;
    for (int m = tid; m < M; m += BLOCK) {
        double y, u;
        load_yu(yb, c, u_row, W, m, y, u);
        const double d = y - mean;
        q2 += u * (d * d);
    }
    const double var = block_sum(q2, s_red, lane, wave) / tot;
    if (tid == 0) {
        A.mean[at] = mean;
        A.sd[at] = sqrt(var);
    }

    for (int k = 0; k < K; ++k) {
        const double target = A.probs[k] * tot;
        uint64_t prefix = 0;
        double below = 0.0;
        for (int pass = 0; pass < NPASS; ++pass) {
            const int shift = 64 - DIGIT_BITS * (pass + 1);
            double bin[NBIN];
#pragma unroll
            for (int d = 0; d < NBIN; ++d) bin[d] = 0.0;
            for (int m = tid; m < M; m += BLOCK) {
                double y, u;
        load_yu(yb, c, u_row, W, m, y, u);
                const uint64_t key = key_of(y);
                // the digits found so far: the bits above shift + 4 (none in the first pass)
                const bool match = pass == 0 || ((key ^ prefix) >> (shift + DIGIT_BITS)) == 0;
                const int digit = (int)(key >> shift) & (NBIN - 1);
#pragma unroll
                for (int d = 0; d < NBIN; ++d) bin[d] += (match && digit == d) ? u : 0.0;
            }
#pragma unroll
            for (int d = 0; d < NBIN; ++d) {
                const double r = wave_sum(bin[d]);
                if (lane == 0) s_red[d * WAVES + wave] = r;
            }
            __syncthreads();
            // every lane walks the 16 bins alike
            double cum = below, at_pick = below, at_last = below;
            int pick = -1, lastpos = 0;
#pragma unroll
            for (int d = 0; d < NBIN; ++d) {
                const double B = ((s_red[d * WAVES] + s_red[d * WAVES + 1]) + s_red[d * WAVES + 2]) + s_red[d * WAVES + 3];
                const double next = cum + B;
                if (B > 0.0) {
                    if (pick < 0 && next >= target) {
                        pick = d;
                        at_pick = cum;
                    }
                    lastpos = d;
                    at_last = cum;
                }
                cum = next;
            }
            __syncthreads();
            if (pick < 0) {
                pick = lastpos;
                at_pick = at_last;
            }
            prefix |= (uint64_t)pick << shift;
            below = at_pick;
        }
        if (tid == 0) A.quant[at * K + k] = value_of(prefix);
    }
}

int check_args(const char* who, const iso_hier_column* columns, int32_t Q, const iso_hier_column* values, int32_t V,
               int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ens_begin, int32_t n_ens_out, const Rec* interim,
               const Rec* rows, int32_t H, const double* ln_norm, const double* probs, int32_t K, const double* weights,
               const double* wsum, const double* ess, const int32_t* n_bad, const double* mean, const double* sd,
               const double* quant, const int32_t* n_nan) {
    ChainShape s{layout, nsteps, n_ens, W, 1};
    s.ens_begin = ens_begin;
    s.n_ens_out = n_ens_out;
    const char* why = nullptr;
    if (!columns || !values || !interim || !rows || !ln_norm || !probs || !weights || !wsum || !ess || !n_bad || !mean || !sd ||
        !quant || !n_nan)
        why = "null pointer";
    else if (Q < 1 || Q > MAXQ) why = "Q must be 1 to 4 columns";
    else if (V < 1 || V > MAXV) why = "V must be 1 to 8 value columns";
    else if (K < 1 || K > MAXK) why = "K must be 1 to 8 probabilities";
    else if (H < 1) why = "H must be at least 1";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (nsteps * (int64_t)W > INT32_MAX) why = "more than 2^31 - 1 samples per star (thin the chain)";
    else if ((int64_t)n_ens_out * V > INT32_MAX) why = "more than 2^31 - 1 (star, value column) pairs (split the call)";
    else {
        for (int k = 0; k < K && !why; ++k)
            if (!(probs[k] > 0.0 && probs[k] < 1.0)) why = "a probability is outside (0, 1)";
        for (int q = 0; q < Q && !why; ++q) why = column_error(columns[q], W, ens_begin, n_ens_out);
        for (int v = 0; v < V && !why; ++v) why = column_error(values[v], W, ens_begin, n_ens_out);
    }
    return why ? fail(ISO_REWEIGHT_ERR_INVALID, who, why) : 0;
}

// the checks of iso_reweight_summary: check_args's, of what the summaries alone take
int check_summary(const char* who, const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t n_ens,
                  int32_t W, int32_t ens_begin, int32_t n_ens_out, const double* probs, int32_t K, const double* weights,
                  const double* mean, const double* sd, const double* quant, const int32_t* n_nan) {
    ChainShape s{layout, nsteps, n_ens, W, 1};
    s.ens_begin = ens_begin;
    s.n_ens_out = n_ens_out;
    const char* why = nullptr;
    if (!values || !probs || !weights || !mean || !sd || !quant || !n_nan) why = "null pointer";
    else if (V < 1 || V > MAXV) why = "V must be 1 to 8 value columns";
    else if (K < 1 || K > MAXK) why = "K must be 1 to 8 probabilities";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES | CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (nsteps * (int64_t)W > INT32_MAX) why = "more than 2^31 - 1 samples per star (thin the chain)";
    else if ((int64_t)n_ens_out * V > INT32_MAX) why = "more than 2^31 - 1 (star, value column) pairs (split the call)";
    else {
        for (int k = 0; k < K && !why; ++k)
            if (!(probs[k] > 0.0 && probs[k] < 1.0)) why = "a probability is outside (0, 1)";
        for (int v = 0; v < V && !why; ++v) why = column_error(values[v], W, ens_begin, n_ens_out);
    }
    return why ? fail(ISO_REWEIGHT_ERR_INVALID, who, why) : 0;
}

// k_reweight_summary on the weights of the stars [ens_begin, ens_begin + n_ens_out): the second launch of
// iso_reweight_stars and the only one of iso_reweight_summary
int launch_summary(const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t W, int32_t ens_begin,
                   int32_t n_ens_out, const int32_t* mask, const double* probs, int32_t K, const double* weights,
                   double* mean, double* sd, double* quant, int32_t* n_nan, void* stream) {
    SArgs B;
    for (int v = 0; v < MAXV; ++v) B.val[v] = dev_col(values[v < V ? v : 0], layout, W);
    for (int k = 0; k < MAXK; ++k) B.probs[k] = probs[k < K ? k : 0];
    B.weights = weights;
    B.mask = mask;
    B.mean = mean;
    B.sd = sd;
    B.quant = quant;
    B.n_nan = n_nan;
    B.V = V;
    B.K = K;
    B.T = (int32_t)nsteps;
    B.W = W;
    B.ens_begin = ens_begin;
    B.pad = 0;
    hipLaunchKernelGGL(k_reweight_summary, dim3((unsigned)n_ens_out * (unsigned)V), dim3(BLOCK), 0, (hipStream_t)stream, B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_REWEIGHT_ERR_HIP, hipGetErrorString(e));
    return 0;
}

// the summaries of a masked star
void summary_masked_host(int s, int V, int K, double* mean, double* sd, double* quant, int32_t* n_nan) {
    for (int v = 0; v < V; ++v) {
        const size_t at = (size_t)s * V + v;
        mean[at] = sd[at] = qnan();
        n_nan[at] = 0;
        for (int k = 0; k < K; ++k) quant[at * K + k] = qnan();
    }
}

// the summaries of the unmasked star s under its weights u[0 .. M), with plain ascending loops and a stable sort; y, uy
// ([M]) and order are the caller's, so that a call allocates them once
void summary_star_host(const DevCol* val, int V, int K, const double* probs, int s, int W, int M, const double* u,
                       double* mean, double* sd, double* quant, int32_t* n_nan, std::vector<double>& y,
                       std::vector<double>& uy, std::vector<int>& order) {
    for (int v = 0; v < V; ++v) {
        const DevCol& c = val[v];
        const size_t at = (size_t)s * V + v;
        double tot = 0.0, sy = 0.0;
        int nn = 0;
        for (int m = 0; m < M; ++m) {
            const int t = m / W, w = m - t * W;
            const double y0 = load(c, s, W, t, w);
            const bool isn = y0 != y0;
            nn += isn ? 1 : 0;
            y[m] = isn ? 0.0 : y0 + 0.0;
            uy[m] = isn ? 0.0 : u[m];
            tot += uy[m];
            sy += uy[m] * y[m];
        }
        n_nan[at] = nn;
        if (!(tot > 0.0) || tot == HUGE_VAL) {
            mean[at] = sd[at] = qnan();
            for (int k = 0; k < K; ++k) quant[at * K + k] = qnan();
            continue;
        }
        const double mu = sy / tot;
        double q2 = 0.0;
        for (int m = 0; m < M; ++m) {
            const double d = y[m] - mu;
            q2 += uy[m] * (d * d);
        }
        mean[at] = mu;
        sd[at] = sqrt(q2 / tot);
        // the samples of positive weight in ascending y, equal values in sample order
        order.clear();
        for (int m = 0; m < M; ++m)
            if (uy[m] > 0.0) order.push_back(m);
        std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return y[i] < y[j]; });
        for (int k = 0; k < K; ++k) {
            const double target = probs[k] * tot;
            double cum = 0.0, ystar = y[order.back()];
            for (size_t i = 0; i < order.size(); ++i) {
                cum += uy[order[i]];
                const bool group_end = i + 1 == order.size() || y[order[i + 1]] != y[order[i]];
                if (group_end && cum >= target) {
                    ystar = y[order[i]];
                    break;
                }
            }
            quant[at * K + k] = ystar;
        }
    }
}

}  // namespace

extern "C" {

const char* iso_reweight_version(void) { return "isochrones_amd reweight 1"; }

const char* iso_reweight_last_error(void) { return g_err; }

int iso_reweight_stars(const iso_hier_column* columns, int32_t Q, const iso_hier_column* values, int32_t V, int layout,
                       int64_t nsteps, int32_t n_ens, int32_t W, int32_t ens_begin, int32_t n_ens_out,
                       const iso_hier_record* interim, const iso_hier_record* rows, int32_t H, const double* ln_norm,
                       const int32_t* mask, const double* probs, int32_t K, double* weights, double* wsum, double* ess,
                       int32_t* n_bad, double* mean, double* sd, double* quant, int32_t* n_nan, void* stream) {
    g_err[0] = 0;
    const int rc = check_args("iso_reweight_stars", columns, Q, values, V, layout, nsteps, n_ens, W, ens_begin, n_ens_out,
                              interim, rows, H, ln_norm, probs, K, weights, wsum, ess, n_bad, mean, sd, quant, n_nan);
    if (rc) return rc;
    WArgs A;
    for (int q = 0; q < MAXQ; ++q) A.col[q] = dev_col(columns[q < Q ? q : 0], layout, W);
    A.interim = interim;
    A.rows = rows;
    A.ln_norm = ln_norm;
    A.mask = mask;
    A.weights = weights;
    A.wsum = wsum;
    A.ess = ess;
    A.n_bad = n_bad;
    A.Q = Q;
    A.T = (int32_t)nsteps;
    A.W = W;
    A.H = H;
    A.n_ens = n_ens;
    A.ens_begin = ens_begin;
    hipLaunchKernelGGL(k_reweight_weights, dim3((unsigned)n_ens_out), dim3(BLOCK), 0, (hipStream_t)stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_REWEIGHT_ERR_HIP, hipGetErrorString(e));
    return launch_summary(values, V, layout, nsteps, W, ens_begin, n_ens_out, mask, probs, K, weights, mean, sd, quant, n_nan,
                          stream);
}

int iso_reweight_stars_host(const iso_hier_column* columns, int32_t Q, const iso_hier_column* values, int32_t V, int layout,
                            int64_t nsteps, int32_t n_ens, int32_t W, int32_t ens_begin, int32_t n_ens_out,
                            const iso_hier_record* interim, const iso_hier_record* rows, int32_t H, const double* ln_norm,
                            const int32_t* mask, const double* probs, int32_t K, double* weights, double* wsum,
                            double* ess, int32_t* n_bad, double* mean, double* sd, double* quant, int32_t* n_nan,
                            void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_args("iso_reweight_stars_host", columns, Q, values, V, layout, nsteps, n_ens, W, ens_begin,
                              n_ens_out, interim, rows, H, ln_norm, probs, K, weights, wsum, ess, n_bad, mean, sd, quant, n_nan);
    if (rc) return rc;
    DevCol col[MAXQ], val[MAXV];
    for (int q = 0; q < Q; ++q) col[q] = dev_col(columns[q], layout, W);
    for (int v = 0; v < V; ++v) val[v] = dev_col(values[v], layout, W);
    const int T = (int)nsteps, M = T * W;
    const size_t ld = (size_t)n_ens;
    std::vector<double> y(M), uy(M);
    std::vector<int> order;
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        if (mask && mask[s] == 0) {
            wsum[s] = ess[s] = qnan();
            n_bad[s] = 0;
            summary_masked_host(s, V, K, mean, sd, quant, n_nan);
            continue;
        }
        double* const u = weights + (size_t)(s - ens_begin) * (size_t)M;
        int nb = 0;
        double S1 = 0.0, S2 = 0.0;
        for (int m = 0; m < M; ++m) {
            const int t = m / W, w = m - t * W;
            double x[MAXQ], lx[MAXQ], l0[MAXQ];
            bool good = true;
            for (int q = 0; q < Q; ++q) {
                x[q] = load(col[q], s, W, t, w);
                lx[q] = log(x[q]);
                l0[q] = lnf(interim[q], x[q], lx[q]);
                good = good && x[q] == x[q] && l0[q] == l0[q] && l0[q] != neg_inf();
            }
            double acc = 0.0;
            if (good)
                for (int h = 0; h < H; ++h) {
                    double r = 0.0;
                    for (int q = 0; q < Q; ++q) {
                        double lf = lnf(rows[(size_t)h * Q + q], x[q], lx[q]);
                        lf = (lf == lf) ? lf : neg_inf();
                        const double d = lf - l0[q];
                        r = (q == 0) ? d : r + d;
                    }
                    const double ln = ln_norm[(size_t)h * ld + s];
                    if (ln == ln && ln != neg_inf()) acc += exp(r - ln);
                }
            u[m] = acc;
            nb += good ? 0 : 1;
            S1 += acc;
            S2 += acc * acc;
        }
        wsum[s] = S1;
        ess[s] = (S1 == 0.0) ? 0.0 : (S1 * S1) / S2;
        n_bad[s] = nb;
        summary_star_host(val, V, K, probs, s, W, M, u, mean, sd, quant, n_nan, y, uy, order);
    }
    return 0;
}

int iso_reweight_summary(const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                         int32_t ens_begin, int32_t n_ens_out, const int32_t* mask, const double* probs, int32_t K,
                         const double* weights, double* mean, double* sd, double* quant, int32_t* n_nan, void* stream) {
    g_err[0] = 0;
    const int rc = check_summary("iso_reweight_summary", values, V, layout, nsteps, n_ens, W, ens_begin, n_ens_out, probs, K,
                                 weights, mean, sd, quant, n_nan);
    if (rc) return rc;
    return launch_summary(values, V, layout, nsteps, W, ens_begin, n_ens_out, mask, probs, K, weights, mean, sd, quant, n_nan,
                          stream);
}

int iso_reweight_summary_host(const iso_hier_column* values, int32_t V, int layout, int64_t nsteps, int32_t n_ens, int32_t W,
                              int32_t ens_begin, int32_t n_ens_out, const int32_t* mask, const double* probs, int32_t K,
                              const double* weights, double* mean, double* sd, double* quant, int32_t* n_nan,
                              void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_summary("iso_reweight_summary_host", values, V, layout, nsteps, n_ens, W, ens_begin, n_ens_out, probs,
                                 K, weights, mean, sd, quant, n_nan);
    if (rc) return rc;
    DevCol val[MAXV];
    for (int v = 0; v < V; ++v) val[v] = dev_col(values[v], layout, W);
    const int M = (int)nsteps * W;
    std::vector<double> y(M), uy(M);
    std::vector<int> order;
    for (int s = ens_begin; s < ens_begin + n_ens_out; ++s) {
        if (mask && mask[s] == 0) {
            summary_masked_host(s, V, K, mean, sd, quant, n_nan);
            continue;
        }
        summary_star_host(val, V, K, probs, s, W, M, weights + (size_t)(s - ens_begin) * (size_t)M, mean, sd, quant, n_nan,
                          y, uy, order);
    }
    return 0;
}

}  // extern "C"
