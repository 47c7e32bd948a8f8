// A batch of weighted EM fits of the cell masses of a binned population density for gfx950, and the star weights of a
// bootstrap: every replicate is one fit on the per-star tables of libiso_binned.so under its own weight per star.  See
// include/isochrones_amd_emfit.h for the definition and the summation order, DESIGN.md section 25 for the mapping and the
// resources.
//
// Two kernels, 256-thread workgroups (four wavefronts), float64:
//   k_emfit_run<BP>   one workgroup per replicate, the loop over the EM steps inside.  The current heights v = g * scale
//                     live in LDS: the kernel rewrites g as it goes, so nothing it iterates on is read through the scalar
//                     cache or a read-only pointer, and the state of an earlier launch (g, Q, t, the status) comes in
//                     through volatile vector loads.  Lanes run along the stars (consecutive doubles of a cell's row).  A
//                     lane keeps one sum per cell in registers, BP of them (the grid padded to 8, 16, 32 or 64 cells, so
//                     that every index is a constant); a star's s1 is taken in a first pass over the cells and its terms
//                     in a second pass that reads the star's column again from the cache, eight cells' loads at a
//                     time, so no table value is held from pass to pass.  A star whose s1 is below
//                     ISO_BINNED_RESCUE_BELOW goes through the same two passes with its products scaled by a power of two
//                     (the header's rescue; a cell's mantissa and exponent wait in LDS next to v).  Every lane takes the
//                     stop / step decision from the same LDS words, so the whole workgroup leaves the loop in the same
//                     iteration and every barrier is met by all of it.
//   k_emfit_weights   one lane per (replicate, star): one Philox call, a count or a logarithm, one store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "isochrones_amd_emfit.h"
#include "../common/last_error.h"
#include "../common/philox.h"
#include "../common/wave_reduce.h"

namespace {

constexpr int BLOCK = ISO_EMFIT_LANES;          // four wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int MAXB = ISO_BINNED_MAX_CELLS;
constexpr int GROUP = 8;                        // cells of the second pass whose loads are issued together
static_assert(BLOCK == 256 && MAXB == 64 && MAXB + 3 <= BLOCK, "a lane per cell, and three more for Q, W and the live count");

struct Args {
    const double* A;
    const double* scale;
    const double* w;
    const int32_t* mask;
    const double* g0;
    double* g;
    double* objective;
    int32_t* n_iter;
    int32_t* status;
    int32_t* n_live;
    double* wsum;
    double tol;
    int32_t B, n_ens, g0_stride, max_iter, steps, first;
};

// the stop of step 5 of the definition, from the evaluation at t
__host__ __device__ inline int decide(int live, int t, double Q, double Qprev, double tol, int max_iter) {
    if (live == 0) return ISO_EMFIT_EMPTY;
    if (t >= 1 && Q - Qprev < tol) return ISO_EMFIT_CONVERGED;
    if (t == max_iter) return ISO_EMFIT_MAX_ITER;
    return ISO_EMFIT_RUNNING;
}

// the header's rescue works on g_b * scale_b * A[b][s] as a mantissa and a power of two, so that no factor and no product
// leaves float64's range: the cell's part, taken once per step (m in [0.25, 1), or 0 for a cell without height)
__host__ __device__ inline void split_height(double g, double scale, double& m, int& e) {
    int eg, es;
    const double mg = frexp(g, &eg), ms = frexp(scale, &es);
    m = mg * ms;
    e = eg + es;
}

// m * 2^e * a as a power of two: its exponent, for a product that is not 0
__host__ __device__ inline int term_exponent(int e, double a) {
    int ea;
    (void)frexp(a, &ea);
    return e + ea;
}

// m * 2^e * a / 2^emax; 0.0 if either factor is 0.0, or if the product lies more than 1074 powers of two below 2^emax
__host__ __device__ inline double scaled_term(double m, int e, double a, int emax) {
    int ea;
    const double ma = frexp(a, &ea);
    return ldexp(m * ma, e + ea - emax);
}

constexpr int NO_TERM = INT32_MIN;              // the largest exponent of a star without a product above 0
constexpr double LN2 = 0.6931471805599453;      // float64's nearest to ln 2

template <int BP>
__global__ void __launch_bounds__(BLOCK, 2) k_emfit_run(const Args P) {
    __shared__ double s_v[MAXB];                // g_b * scale_b of the current step
    __shared__ double s_vm[MAXB];               // the same heights as a mantissa and a power of two, for the rescue
    __shared__ int s_ve[MAXB];
    __shared__ double s_N[MAXB];
    __shared__ double s_part[WAVES][MAXB + 2];  // the wavefronts' totals: the cells, then Q and W
    __shared__ double s_Q, s_W, s_prev;
    __shared__ int s_nl[WAVES], s_live, s_t, s_status;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = P.B, n_ens = P.n_ens;
    const size_t r = blockIdx.x, ld = (size_t)n_ens;

    if (tid == 0) {
        if (P.first) {
            s_t = 0;
            s_status = ISO_EMFIT_RUNNING;
            s_prev = 0.0;
        } else {
            s_t = *(const volatile int32_t*)(P.n_iter + r);
            s_status = *(const volatile int32_t*)(P.status + r);
            s_prev = *(const volatile double*)(P.objective + r);
        }
    }
    double g_mine = 0.0;                        // g of cell tid
    if (tid < B) {
        const double* from = P.first ? P.g0 + r * (size_t)P.g0_stride : P.g + r * (size_t)B;
        const double gb = *(const volatile double*)(from + tid);
        g_mine = gb;
        s_v[tid] = gb * P.scale[tid];
        split_height(gb, P.scale[tid], s_vm[tid], s_ve[tid]);
    } else if (tid < MAXB) {
        s_v[tid] = 0.0;                         // the cells past the grid that a group of the second pass reads
        s_vm[tid] = 0.0;
        s_ve[tid] = 0;
    }
    __syncthreads();
    if (s_status != ISO_EMFIT_RUNNING) return;  // the same word for every lane
    int t = s_t, done = 0, status = ISO_EMFIT_RUNNING, live = 0;
    double Qprev = s_prev, Q = Qprev;
    const double* wr = P.w ? P.w + r * ld : nullptr;

    for (;;) {
        double acc[BP];
#pragma unroll
        for (int b = 0; b < BP; ++b) acc[b] = 0.0;
        double q = 0.0, ws = 0.0;
        int nl = 0;
        for (int s = tid; s < n_ens; s += BLOCK) {
            const double* col = P.A + s;
            double s1 = 0.0;
            const double* pc = col;
#pragma unroll 8
            for (int b = 0; b < B; ++b, pc += ld) {
                const double p = s_v[b] * *pc;
                s1 += p;
            }
            const double wt = wr ? wr[s] : 1.0;
            const bool counts = (!P.mask || P.mask[s] != 0) && wt > 0.0;
            if (counts && s1 >= ISO_BINNED_RESCUE_BELOW) {
                const double term = wt * log(s1);
                q += term;
                ws += wt;
                ++nl;
                const double ratio = wt / s1;
                pc = col;
                // the heights of the second pass: left alone the compiler lifts all BP of them out of the star loop into
                // registers, which the BP sums need.  Above 16 cells the read is pinned to the star by an index the
                // compiler cannot see through (no instruction), and each height comes from LDS as in the first pass
                int at = 0;
                if (BP > 16) asm volatile("" : "+v"(at));
                // likewise the BP comparisons with B would be lifted out as BP lane masks: B is taken as a scalar the
                // compiler cannot see through, and each comparison is one scalar compare where it is used
                int nb = B;
                asm volatile("" : "+s"(nb));
                // eight cells at a time, so that eight loads are in flight: a group is entered if its first cell exists,
                // and a cell past the grid reads the last row again into a sum that is never used
                const int last = nb - 1;
#pragma unroll
                for (int b0 = 0; b0 < BP; b0 += GROUP) {
                    if (b0 < nb) {
                        double a[GROUP];
#pragma unroll
                        for (int j = 0; j < GROUP; ++j) a[j] = col[(size_t)min(b0 + j, last) * ld];
#pragma unroll
                        for (int j = 0; j < GROUP; ++j) {
                            const double p = s_v[at + b0 + j] * a[j];
                            const double add = p * ratio;
                            acc[b0 + j] += add;
                        }
                    }
                }
            } else if (counts && s1 < ISO_BINNED_RESCUE_BELOW) {
                // rare: s1 is below the threshold (0 included; a NaN is not, and adds nothing).  The star's products are taken again relative to its
                // largest one, 2^emax, in the same order and into the same sums
                int emax = NO_TERM;
                pc = col;
#pragma unroll 1
                for (int b = 0; b < B; ++b, pc += ld) {
                    const double a = *pc;
                    if (a > 0.0 && s_vm[b] > 0.0) emax = max(emax, term_exponent(s_ve[b], a));
                }
                if (emax != NO_TERM) {
                    double r1 = 0.0;
                    pc = col;
#pragma unroll 1
                    for (int b = 0; b < B; ++b, pc += ld) {
                        const double p = scaled_term(s_vm[b], s_ve[b], *pc, emax);
                        r1 += p;
                    }
                    const double term = wt * (log(r1) + (double)emax * LN2);
                    q += term;
                    ws += wt;
                    ++nl;
                    const double ratio = wt / r1;
                    int at = 0;
                    asm volatile("" : "+v"(at));
                    int nb = B;
                    asm volatile("" : "+s"(nb));
                    const int last = nb - 1;
#pragma unroll
                    for (int b0 = 0; b0 < BP; b0 += GROUP) {
                        if (b0 < nb) {
                            double a[GROUP];
#pragma unroll
                            for (int j = 0; j < GROUP; ++j) a[j] = col[(size_t)min(b0 + j, last) * ld];
#pragma unroll
                            for (int j = 0; j < GROUP; ++j) {
                                const double p = scaled_term(s_vm[at + b0 + j], s_ve[at + b0 + j], a[j], emax);
                                const double add = p * ratio;
                                acc[b0 + j] += add;
                            }
                        }
                    }
                }
            }
        }
        int nb = B;
        asm volatile("" : "+s"(nb));
#pragma unroll
        for (int b = 0; b < BP; ++b) {
            if (b < nb) {
                const double tot = wave_sum(acc[b]);
                if (lane == 0) s_part[wave][b] = tot;
            }
        }
        q = wave_sum(q);
        ws = wave_sum(ws);
        nl = wave_sum_int(nl);
        if (lane == 0) {
            s_part[wave][MAXB] = q;
            s_part[wave][MAXB + 1] = ws;
            s_nl[wave] = nl;
        }
        __syncthreads();
        if (tid < B) s_N[tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
        if (tid == MAXB) s_Q = ((s_part[0][MAXB] + s_part[1][MAXB]) + s_part[2][MAXB]) + s_part[3][MAXB];
        if (tid == MAXB + 1) s_W = ((s_part[0][MAXB + 1] + s_part[1][MAXB + 1]) + s_part[2][MAXB + 1]) + s_part[3][MAXB + 1];
        if (tid == MAXB + 2) s_live = ((s_nl[0] + s_nl[1]) + s_nl[2]) + s_nl[3];
        __syncthreads();
        Q = s_Q;
        live = s_live;
        status = decide(live, t, Q, Qprev, P.tol, P.max_iter);
        if (status != ISO_EMFIT_RUNNING) break;
        if (tid < B) {
            double T = 0.0;
            for (int b = 0; b < B; ++b) T += s_N[b];
            const double gb = s_N[tid] / T;
            g_mine = gb;
            s_v[tid] = gb * P.scale[tid];
            split_height(gb, P.scale[tid], s_vm[tid], s_ve[tid]);
        }
        Qprev = Q;
        ++t;
        ++done;
        __syncthreads();
        if (done == P.steps && t < P.max_iter) break;   // the next launch goes on from the outputs
    }

    if (tid < B) P.g[r * (size_t)B + tid] = g_mine;
    if (tid == 0) {
        P.objective[r] = Q;
        P.n_iter[r] = t;
        P.status[r] = status;
        P.n_live[r] = live;
        P.wsum[r] = s_W;
    }
}

__host__ __device__ inline double weight_of(int32_t kind, uint64_t seed, uint32_t replicate, uint32_t s) {
    uint32_t x[4];
    philox4x32_10(s, replicate, 0u, (uint32_t)ISO_EMFIT_PHILOX_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    const double u = philox_uniform53(x[0], x[1]);
    if (kind == ISO_EMFIT_EXP) return -log(u);
    const double c[ISO_EMFIT_POISSON_TERMS] = {ISO_EMFIT_POISSON_CDF};
    int k = 0;
#pragma unroll
    for (int j = 0; j < ISO_EMFIT_POISSON_TERMS; ++j) k += (u >= c[j]) ? 1 : 0;
    return (double)k;
}

__global__ void __launch_bounds__(BLOCK) k_emfit_weights(int32_t kind, uint64_t seed, int32_t first, int64_t total,
                                                         int32_t n_ens, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / n_ens;
    out[i] = weight_of(kind, seed, (uint32_t)(first + r), (uint32_t)(i - r * n_ens));
}

int check_run(const char* who, const double* A, int32_t B, int32_t n_ens, const double* scale, int32_t R, const double* g0,
              int32_t g0_stride, int32_t max_iter, double tol, int32_t steps_per_launch, const double* g,
              const double* objective, const int32_t* n_iter, const int32_t* status, const int32_t* n_live,
              const double* wsum) {
    const char* why = nullptr;
    if (!A || !scale || !g0 || !g || !objective || !n_iter || !status || !n_live || !wsum) why = "null pointer";
    else if (B < 1 || B > MAXB) why = "B must be 1 to 64 cells";
    else if (n_ens < 1) why = "n_ens must be at least 1";
    else if (R < 1) why = "R must be at least 1";
    else if (g0_stride != 0 && g0_stride < B) why = "g0_stride must be 0 (one shared row) or at least B";
    else if (max_iter < 0) why = "max_iter must not be negative";
    else if (tol != tol) why = "tol is not a number";
    else if (steps_per_launch < 0) why = "steps_per_launch must not be negative";
    return why ? fail(ISO_EMFIT_ERR_INVALID, who, why) : 0;
}

int check_weights(const char* who, int32_t kind, int32_t first, int32_t R, int32_t n_ens, const double* out) {
    const char* why = nullptr;
    if (!out) why = "null pointer";
    else if (kind != ISO_EMFIT_POISSON && kind != ISO_EMFIT_EXP) why = "kind must be ISO_EMFIT_POISSON or ISO_EMFIT_EXP";
    else if (first < 0) why = "first_replicate must not be negative";
    else if (R < 1) why = "R must be at least 1";
    else if (n_ens < 1) why = "n_ens must be at least 1";
    else if ((int64_t)first + R > INT32_MAX) why = "first_replicate + R must stay below 2^31";
    else if (((int64_t)R * n_ens + BLOCK - 1) / BLOCK > INT32_MAX) why = "more than 2^31 - 1 workgroups (split the replicates)";
    return why ? fail(ISO_EMFIT_ERR_INVALID, who, why) : 0;
}

bool bad_value(double x) { return !(x >= 0.0) || x == HUGE_VAL; }   // negative, NaN or infinite

template <int BP>
void launch(const Args& P, int32_t R, hipStream_t stream) {
    hipLaunchKernelGGL(k_emfit_run<BP>, dim3((unsigned)R), dim3(BLOCK), 0, stream, P);
}

}  // namespace

extern "C" {

const char* iso_emfit_version(void) { return "isochrones_amd emfit 1"; }

const char* iso_emfit_last_error(void) { return g_err; }

int iso_emfit_run(const double* A, int32_t B, int32_t n_ens, const double* scale, const double* w, int32_t R,
                  const int32_t* mask, const double* g0, int32_t g0_stride, int32_t max_iter, double tol,
                  int32_t steps_per_launch, double* g, double* objective, int32_t* n_iter, int32_t* status,
                  int32_t* n_live, double* wsum, void* stream) {
    g_err[0] = 0;
    const int rc = check_run("iso_emfit_run", A, B, n_ens, scale, R, g0, g0_stride, max_iter, tol, steps_per_launch, g,
                             objective, n_iter, status, n_live, wsum);
    if (rc) return rc;
    int64_t steps = steps_per_launch;
    if (steps <= 0) {
        steps = (int64_t)ISO_EMFIT_LAUNCH_WORK / ((int64_t)n_ens * B);
        if (steps < 1) steps = 1;
    }
    if (steps > INT32_MAX) steps = INT32_MAX;
    int64_t launches = ((int64_t)max_iter + steps - 1) / steps;
    if (launches < 1) launches = 1;             // max_iter == 0 still evaluates Q at g0
    Args P;
    P.A = A;
    P.scale = scale;
    P.w = w;
    P.mask = mask;
    P.g0 = g0;
    P.g = g;
    P.objective = objective;
    P.n_iter = n_iter;
    P.status = status;
    P.n_live = n_live;
    P.wsum = wsum;
    P.tol = tol;
    P.B = B;
    P.n_ens = n_ens;
    P.g0_stride = g0_stride;
    P.max_iter = max_iter;
    P.steps = (int32_t)steps;
    for (int64_t k = 0; k < launches; ++k) {
        P.first = k == 0 ? 1 : 0;
        if (B <= 8) launch<8>(P, R, (hipStream_t)stream);
        else if (B <= 16) launch<16>(P, R, (hipStream_t)stream);
        else if (B <= 32) launch<32>(P, R, (hipStream_t)stream);
        else launch<64>(P, R, (hipStream_t)stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(ISO_EMFIT_ERR_HIP, hipGetErrorString(e));
    }
    return 0;
}

int iso_emfit_run_host(const double* A, int32_t B, int32_t n_ens, const double* scale, const double* w, int32_t R,
                       const int32_t* mask, const double* g0, int32_t g0_stride, int32_t max_iter, double tol,
                       int32_t steps_per_launch, double* g, double* objective, int32_t* n_iter, int32_t* status,
                       int32_t* n_live, double* wsum, void* stream) {
    (void)stream;
    g_err[0] = 0;
    const char* who = "iso_emfit_run_host";
    const int rc = check_run(who, A, B, n_ens, scale, R, g0, g0_stride, max_iter, tol, steps_per_launch, g, objective,
                             n_iter, status, n_live, wsum);
    if (rc) return rc;
    const size_t ld = (size_t)n_ens;
    for (int b = 0; b < B; ++b)
        if (bad_value(scale[b])) return fail(ISO_EMFIT_ERR_INVALID, who, "scale must be finite and not negative");
    if (w)
        for (size_t i = 0; i < (size_t)R * ld; ++i)
            if (bad_value(w[i])) return fail(ISO_EMFIT_ERR_INVALID, who, "w must be finite and not negative");
    for (int r = 0; r < (g0_stride == 0 ? 1 : R); ++r) {
        double sum = 0.0;
        for (int b = 0; b < B; ++b) {
            const double x = g0[(size_t)r * g0_stride + b];
            if (bad_value(x)) return fail(ISO_EMFIT_ERR_INVALID, who, "g0 must be finite and not negative");
            sum += x;
        }
        if (!(sum > 0.0)) return fail(ISO_EMFIT_ERR_INVALID, who, "a row of g0 must sum to something above 0");
    }
    std::vector<double> gr(B), v(B), N(B), vm(B);
    std::vector<int> ve(B);
    for (int r = 0; r < R; ++r) {
        for (int b = 0; b < B; ++b) gr[b] = g0[(size_t)r * g0_stride + b];
        const double* wr = w ? w + (size_t)r * ld : nullptr;
        double Qprev = 0.0, Q = 0.0, W = 0.0;
        int t = 0, st = ISO_EMFIT_RUNNING, live = 0;
        for (;;) {
            for (int b = 0; b < B; ++b) {
                v[b] = gr[b] * scale[b];
                split_height(gr[b], scale[b], vm[b], ve[b]);
                N[b] = 0.0;
            }
            Q = 0.0;
            W = 0.0;
            live = 0;
            for (int s = 0; s < n_ens; ++s) {
                double s1 = 0.0;
                for (int b = 0; b < B; ++b) {
                    const double p = v[b] * A[(size_t)b * ld + s];
                    s1 += p;
                }
                const double wt = wr ? wr[s] : 1.0;
                if (!((!mask || mask[s] != 0) && wt > 0.0)) continue;
                if (s1 != s1) continue;
                if (s1 < ISO_BINNED_RESCUE_BELOW) {
                    int emax = NO_TERM;
                    for (int b = 0; b < B; ++b) {
                        const double a = A[(size_t)b * ld + s];
                        if (a > 0.0 && vm[b] > 0.0) emax = std::max(emax, term_exponent(ve[b], a));
                    }
                    if (emax == NO_TERM) continue;
                    double r1 = 0.0;
                    for (int b = 0; b < B; ++b) {
                        const double p = scaled_term(vm[b], ve[b], A[(size_t)b * ld + s], emax);
                        r1 += p;
                    }
                    const double term = wt * (log(r1) + (double)emax * LN2);
                    Q += term;
                    W += wt;
                    ++live;
                    const double ratio = wt / r1;
                    for (int b = 0; b < B; ++b) {
                        const double p = scaled_term(vm[b], ve[b], A[(size_t)b * ld + s], emax);
                        const double add = p * ratio;
                        N[b] += add;
                    }
                    continue;
                }
                const double term = wt * log(s1);
                Q += term;
                W += wt;
                ++live;
                const double ratio = wt / s1;
                for (int b = 0; b < B; ++b) {
                    const double p = v[b] * A[(size_t)b * ld + s];
                    const double add = p * ratio;
                    N[b] += add;
                }
            }
            st = decide(live, t, Q, Qprev, tol, max_iter);
            if (st != ISO_EMFIT_RUNNING) break;
            double T = 0.0;
            for (int b = 0; b < B; ++b) T += N[b];
            for (int b = 0; b < B; ++b) gr[b] = N[b] / T;
            Qprev = Q;
            ++t;
        }
        for (int b = 0; b < B; ++b) g[(size_t)r * B + b] = gr[b];
        objective[r] = Q;
        n_iter[r] = t;
        status[r] = st;
        n_live[r] = live;
        wsum[r] = W;
    }
    return 0;
}

int iso_emfit_weights(int32_t kind, uint64_t seed, int32_t first_replicate, int32_t R, int32_t n_ens, double* out,
                      void* stream) {
    g_err[0] = 0;
    const int rc = check_weights("iso_emfit_weights", kind, first_replicate, R, n_ens, out);
    if (rc) return rc;
    const int64_t total = (int64_t)R * n_ens;
    hipLaunchKernelGGL(k_emfit_weights, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       kind, seed, first_replicate, total, n_ens, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_EMFIT_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_emfit_weights_host(int32_t kind, uint64_t seed, int32_t first_replicate, int32_t R, int32_t n_ens, double* out,
                           void* stream) {
    (void)stream;
    g_err[0] = 0;
    const int rc = check_weights("iso_emfit_weights_host", kind, first_replicate, R, n_ens, out);
    if (rc) return rc;
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < n_ens; ++s)
            out[(size_t)r * n_ens + s] = weight_of(kind, seed, (uint32_t)(first_replicate + r), (uint32_t)s);
    return 0;
}

}  // extern "C"
