// A batch of coeval systems of one or two stars evaluated on a model grid and a bolometric-correction grid, for gfx950.
// See include/isochrones_amd_population.h for the definition and the order of the arithmetic, DESIGN.md section 16 for
// the mapping and what bounds the kernel.
//
// One kernel, one system per lane, float64:
//   k_population_eval  lanes run along the system index i, the contiguous axis of every input and output, so each load
//                      of a coordinate, distance or AV and each store of an output row is one contiguous run of a
//                      wavefront; workgroups stride over the batch.  A lane walks its system's components in a loop.
//                      First the model cell: three brackets, eight weights, then the Q columns eight at a time (the
//                      width is a compile-time constant inside each branch of a wave-uniform switch, so the accumulators
//                      stay in registers; two columns per load when Q is even); the four columns the magnitudes need are
//                      picked out of the walk by wave-uniform selects.  Then the BC cell, eight adjacent bands at a time:
//                      the T, g and f brackets and the eight (T, g, f) corner weights are made once and feed the lookup at
//                      AV and the one at AV = 0, which differ in the A bracket alone.  The pow and log10 of a binary's
//                      combined light run as loops over sixteen values a lane keeps in LDS, not as sixteen inlined copies.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_population.h"
#include "../common/grid_interp.h"
#include "../common/last_error.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = ISO_POPULATION_MAX_BLOCKS;   // a gather-bound stream: eight workgroups per CU, the rest by striding
constexpr int MAXC = ISO_POPULATION_MAX_COMPS;
constexpr int GQ = 8;                           // model columns per pass
constexpr int CH = 8;                           // bands per pass

struct Args {
    iso_population_model_table M;
    iso_population_bc_table T;
    const double* coords;
    const double* distance;
    const double* AV;
    iso_population_out O;
    int64_t N;
    int32_t C;
};

__host__ __device__ inline double pos_inf() {
    union { uint64_t u; double d; } x;
    x.u = 0x7ff0000000000000ULL;
    return x.d;
}

// The columns [q0, q0 + W) of one component: interpolated (p: the cell's first corner at column q0; off[j], w[j]: the
// corners' offsets and weights in the header's order), stored to o[j * N] unless o is null, and the hot ones kept in hv.
template <int W, bool PAIR>
__device__ __forceinline__ void column_group(const iso_population_model_table& M, bool ok, const double* __restrict__ p,
                                             const int (&off)[8], const double (&w)[8], int q0, double* __restrict__ o,
                                             int64_t N, double (&hv)[4]) {
    double v[W];
    if (ok) {
        cell3_columns<W, PAIR>(p, off, w, v);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = qnan();
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int want = M.hot[h] - q0;                         // wave-uniform
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (want == j) hv[h] = v[j];
    }
    if (o) {
#pragma unroll
        for (int j = 0; j < W; ++j) o[(int64_t)j * N] = v[j];
    }
}

template <int W>
__device__ __forceinline__ void column_group(const iso_population_model_table& M, bool pair, bool ok,
                                             const double* __restrict__ p, const int (&off)[8], const double (&w)[8],
                                             int q0, double* __restrict__ o, int64_t N, double (&hv)[4]) {
    if constexpr (W % 2 == 0) {
        if (pair) {
            column_group<W, true>(M, ok, p, off, w, q0, o, N, hv);
            return;
        }
    }
    column_group<W, false>(M, ok, p, off, w, q0, o, N, hv);
}

__global__ void __launch_bounds__(BLOCK) k_population_eval(const Args A) {
    __shared__ double s_wk[2 * CH][BLOCK];                      // a lane's sixteen values on their way through pow / log10
    const iso_population_model_table& M = A.M;
    const iso_population_bc_table& T = A.T;
    const int64_t N = A.N;
    const int Q = M.Q, B = T.B, C = A.C, lane = (int)threadIdx.x;
    const bool pair = Q % 2 == 0;                               // a node's columns start on 16 bytes: read two at a time
    const bool want_sys = A.O.sys_mag || A.O.sys_A;
    const bool want_mags = want_sys || A.O.mag_out || A.O.A_out;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + lane; i < N; i += (int64_t)gridDim.x * BLOCK) {
        // ---- step 1: the model columns of every component; (Teff, logg, feh, Mbol) kept ----
        double hv0[4] = {0.0, 0.0, 0.0, 0.0}, hv1[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < C; ++c) {
            const double* __restrict__ x = A.coords + (int64_t)c * 3 * N + i;
            const double x0 = x[0], x1 = x[N], xk = x[2 * N];
            const bool ok = on_grid3(M, x0, x1, xk);
            int off[8];
            double w[8];
            const double* __restrict__ p = M.cols + cell3_at(M, Q, x0, x1, xk, off, w);
            double* __restrict__ o = A.O.cols_out ? A.O.cols_out + (int64_t)c * Q * N + i : nullptr;
            double hv[4] = {0.0, 0.0, 0.0, 0.0};
            int q0 = 0;
            for (; q0 + GQ <= Q; q0 += GQ)
                column_group<GQ>(M, pair, ok, p + q0, off, w, q0, o ? o + (int64_t)q0 * N : nullptr, N, hv);
            double* __restrict__ oq = o ? o + (int64_t)q0 * N : nullptr;
            switch (Q - q0) {                                   // wave-uniform
            case 1: column_group<1>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 2: column_group<2>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 3: column_group<3>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 4: column_group<4>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 5: column_group<5>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 6: column_group<6>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            case 7: column_group<7>(M, pair, ok, p + q0, off, w, q0, oq, N, hv); break;
            default: break;
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if (c == 0) hv0[h] = hv[h];
                else hv1[h] = hv[h];
            }
        }
        if (!want_mags) continue;
        // ---- steps 2 and 3, and the system ----
        const double dist = A.distance[i], av = A.AV[i];
        const double dm = 5 * log10(dist / 10.0);
        int iA, iA0;
        double tA, tA0;
        const bool okA = on_axis(T.axA, T.nA, av), okA0 = on_axis(T.axA, T.nA, 0.0);
        bracket(T.axA, T.nA, av, iA, tA);
        bracket(T.axA, T.nA, 0.0, iA0, tA0);
        const double uA = 1 - tA, uA0 = 1 - tA0;
        for (int b0 = 0; b0 < B; b0 += CH) {
            const int nb = B - b0 < CH ? B - b0 : CH;
            double sum[CH], sumt[CH];                           // the two sums of the system (C = 2)
#pragma unroll
            for (int j = 0; j < CH; ++j) sum[j] = sumt[j] = 0.0;
            for (int c = 0; c < C; ++c) {
                const double xT = c == 0 ? hv0[0] : hv1[0], xg = c == 0 ? hv0[1] : hv1[1];
                const double xf = c == 0 ? hv0[2] : hv1[2], mbol = c == 0 ? hv0[3] : hv1[3];
                const bool okb = bc_on_grid(T, xT, xg, xf);
                double acc[CH], acc0[CH];
#pragma unroll
                for (int j = 0; j < CH; ++j) acc[j] = acc0[j] = 0.0;
                if (okb) {
                    const BcCell cell = bc_bracket(T, xT, xg, xf);
                    const double* __restrict__ pb = T.bc + cell.node + b0;
                    // corner order 0000 .. 1111 with bA fastest: the three slow bits as a loop, whose (T, g, f) weight both
                    // lookups share
#pragma nounroll
                    for (int k = 0; k < 8; ++k) {
                        const double wTgf = bc_weight(cell, k);
                        const double* __restrict__ pk = pb + bc_offset(T, k);
#pragma unroll
                        for (int bA = 0; bA < 2; ++bA) {
                            const double wa = wTgf * (bA ? tA : uA), wa0 = wTgf * (bA ? tA0 : uA0);
                            const double* __restrict__ ca = pk + (iA + bA) * B;
                            const double* __restrict__ ca0 = pk + (iA0 + bA) * B;
#pragma unroll
                            for (int j = 0; j < CH; ++j)
                                if (j < nb) {
                                    acc[j] = acc[j] + ca[j] * wa;
                                    acc0[j] = acc0[j] + ca0[j] * wa0;
                                }
                        }
                    }
                }
                const bool ok1 = okb && okA, ok0 = okb && okA0;
                const double base = mbol + dm;
                double* __restrict__ om = A.O.mag_out ? A.O.mag_out + (int64_t)(c * B + b0) * N + i : nullptr;
                double* __restrict__ oa = A.O.A_out ? A.O.A_out + (int64_t)(c * B + b0) * N + i : nullptr;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j >= nb) continue;
                    const double mag = base - (ok1 ? acc[j] : qnan());
                    const double tru = base - (ok0 ? acc0[j] : qnan());
                    const double a = mag - tru;
                    if (om) om[(int64_t)j * N] = mag;
                    if (oa) oa[(int64_t)j * N] = a;
                    if (!want_sys) continue;
                    if (C == 1) {
                        if (A.O.sys_mag) A.O.sys_mag[(int64_t)(b0 + j) * N + i] = mag;
                        if (A.O.sys_A) A.O.sys_A[(int64_t)(b0 + j) * N + i] = a;
                    } else if (c == 0) {
                        s_wk[j][lane] = -0.4 * mag;
                        s_wk[CH + j][lane] = -0.4 * (mag - a);
                    } else {
                        const double m1 = mag != mag ? pos_inf() : mag, a1 = a != a ? 0.0 : a;
                        s_wk[j][lane] = -0.4 * m1;
                        s_wk[CH + j][lane] = -0.4 * (m1 - a1);
                    }
                }
                if (want_sys && C > 1) {
#pragma nounroll
                    for (int h = 0; h < 2; ++h)
#pragma nounroll
                        for (int j = 0; j < nb; ++j) s_wk[h * CH + j][lane] = pow(10.0, s_wk[h * CH + j][lane]);
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        if (j >= nb) continue;
                        sum[j] = sum[j] + s_wk[j][lane];
                        sumt[j] = sumt[j] + s_wk[CH + j][lane];
                    }
                }
            }
            if (want_sys && C > 1) {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j >= nb) continue;
                    s_wk[j][lane] = sum[j];
                    s_wk[CH + j][lane] = sumt[j];
                }
#pragma nounroll
                for (int h = 0; h < 2; ++h)
#pragma nounroll
                    for (int j = 0; j < nb; ++j) s_wk[h * CH + j][lane] = -2.5 * log10(s_wk[h * CH + j][lane]);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j >= nb) continue;
                    const double sm = s_wk[j][lane];
                    if (A.O.sys_mag) A.O.sys_mag[(int64_t)(b0 + j) * N + i] = sm;
                    if (A.O.sys_A) A.O.sys_A[(int64_t)(b0 + j) * N + i] = sm - s_wk[CH + j][lane];
                }
            }
        }
    }
}

// arguments checked; device = the checks only the kernel needs
int prepare(const char* who, bool device, const iso_population_model_table* m, const iso_population_bc_table* bc,
            const double* coords, const double* distance, const double* AV, int64_t N, int32_t C,
            const iso_population_out* out, Args& A) {
    const char* why = nullptr;
    if (!m || !m->cols || !m->ax0 || !m->ax1 || !m->axk) why = "null model table pointer";
    else if (!bc || !bc->bc || !bc->axT || !bc->axg || !bc->axf || !bc->axA) why = "null BC table pointer";
    else if (!coords || !distance || !AV || !out) why = "null pointer";
    else if (m->Q < 4 || m->Q > ISO_POPULATION_MAX_COLS) why = "Q must be 4 to 32 columns";
    else if (m->hot[0] < 0 || m->hot[0] >= m->Q || m->hot[1] < 0 || m->hot[1] >= m->Q || m->hot[2] < 0 ||
             m->hot[2] >= m->Q || m->hot[3] < 0 || m->hot[3] >= m->Q)
        why = "a hot column index is outside [0, Q)";
    else if (bc->B < 1 || bc->B > ISO_POPULATION_MAX_BANDS) why = "B must be 1 to 32 bands";
    else if (C < 1 || C > MAXC) why = "C must be 1 or 2 components";
    else if (N < 0) why = "N must not be negative";
    else if (N > INT32_MAX) why = "more than 2^31 - 1 systems (split the batch)";
    else if (m->n0 < 2 || m->n1 < 2 || m->nk < 2) why = "every model axis needs at least 2 nodes";
    else if (bc->nT < 2 || bc->ng < 2 || bc->nf < 2 || bc->nA < 2) why = "every BC axis needs at least 2 nodes";
    else if ((double)m->n0 * m->n1 * m->nk * m->Q > (double)INT32_MAX) why = "model table too large (more than 2^31 - 1 entries)";
    else if ((double)bc->nT * bc->ng * bc->nf * bc->nA * bc->B > (double)INT32_MAX)
        why = "BC table too large (more than 2^31 - 1 entries)";
    else if (device && m->Q % 2 == 0 && ((uintptr_t)m->cols & 15)) why = "cols must be 16-byte aligned for an even Q";
    if (why) return fail(ISO_POPULATION_ERR_INVALID, who, why);
    A.M = *m;
    A.T = *bc;
    A.coords = coords;
    A.distance = distance;
    A.AV = AV;
    A.O = *out;
    A.N = N;
    A.C = C;
    return 0;
}

// steps 1 to 3 of the header for one component on the host: v[Q], mag[B], a[B]
void component_host(const Args& A, int64_t i, int c, double* v, double* mag, double* a) {
    const iso_population_model_table& M = A.M;
    const iso_population_bc_table& T = A.T;
    const int Q = M.Q, B = T.B;
    const int64_t N = A.N;
    const double x0 = A.coords[((int64_t)c * 3 + 0) * N + i], x1 = A.coords[((int64_t)c * 3 + 1) * N + i],
                 xk = A.coords[((int64_t)c * 3 + 2) * N + i];
    cell3(M, Q, x0, x1, xk, v);
    const double mbol = v[M.hot[3]], dm = 5 * log10(A.distance[i] / 10.0), base = mbol + dm;
    double val[2][ISO_POPULATION_MAX_BANDS];                    // bc_c at AV, bc0_c at 0.0
    for (int pass = 0; pass < 2; ++pass)
        for (int b0 = 0; b0 < B; b0 += CH) {
            double chunk[CH];
            const int nb = B - b0 < CH ? B - b0 : CH;
            bc_chunk<CH>(T, v[M.hot[0]], v[M.hot[1]], v[M.hot[2]], pass == 0 ? A.AV[i] : 0.0, b0, nb, chunk);
            for (int j = 0; j < nb; ++j) val[pass][b0 + j] = chunk[j];
        }
    for (int b = 0; b < B; ++b) {
        mag[b] = base - val[0][b];
        const double tru = base - val[1][b];
        a[b] = mag[b] - tru;
    }
}

}  // namespace

extern "C" {

const char* iso_population_version(void) { return "isochrones_amd population 1"; }

const char* iso_population_last_error(void) { return g_err; }

int iso_population_eval(const iso_population_model_table* model, const iso_population_bc_table* bc, const double* coords,
                        const double* distance, const double* AV, int64_t N, int32_t C, const iso_population_out* out,
                        void* stream) {
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_population_eval", true, model, bc, coords, distance, AV, N, C, out, A);
    if (rc) return rc;
    if (N == 0) return 0;
    const int64_t need = (N + BLOCK - 1) / BLOCK;
    const int blocks = need < MAX_BLOCKS ? (int)need : MAX_BLOCKS;
    hipLaunchKernelGGL(k_population_eval, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_POPULATION_ERR_HIP, "iso_population_eval", hipGetErrorString(e));
    return 0;
}

int iso_population_eval_host(const iso_population_model_table* model, const iso_population_bc_table* bc,
                             const double* coords, const double* distance, const double* AV, int64_t N, int32_t C,
                             const iso_population_out* out, void* stream) {
    (void)stream;
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_population_eval_host", false, model, bc, coords, distance, AV, N, C, out, A);
    if (rc) return rc;
    const int Q = A.M.Q, B = A.T.B;
    const iso_population_out& O = A.O;
    for (int64_t i = 0; i < N; ++i) {
        double v[ISO_POPULATION_MAX_COLS], mag[MAXC][ISO_POPULATION_MAX_BANDS], a[MAXC][ISO_POPULATION_MAX_BANDS];
        for (int c = 0; c < C; ++c) {
            component_host(A, i, c, v, mag[c], a[c]);
            for (int q = 0; q < Q; ++q)
                if (O.cols_out) O.cols_out[((int64_t)c * Q + q) * N + i] = v[q];
            for (int b = 0; b < B; ++b) {
                if (O.mag_out) O.mag_out[((int64_t)c * B + b) * N + i] = mag[c][b];
                if (O.A_out) O.A_out[((int64_t)c * B + b) * N + i] = a[c][b];
            }
        }
        for (int b = 0; b < B; ++b) {
            double sm = mag[0][b], sa = a[0][b];
            if (C > 1) {
                const double m1 = mag[1][b] != mag[1][b] ? pos_inf() : mag[1][b], a1 = a[1][b] != a[1][b] ? 0.0 : a[1][b];
                double sum = 0.0, sumt = 0.0;
                sum = sum + pow(10.0, -0.4 * mag[0][b]);
                sum = sum + pow(10.0, -0.4 * m1);
                sumt = sumt + pow(10.0, -0.4 * (mag[0][b] - a[0][b]));
                sumt = sumt + pow(10.0, -0.4 * (m1 - a1));
                sm = -2.5 * log10(sum);
                sa = sm - (-2.5 * log10(sumt));
            }
            if (O.sys_mag) O.sys_mag[(int64_t)b * N + i] = sm;
            if (O.sys_A) O.sys_A[(int64_t)b * N + i] = sa;
        }
    }
    return 0;
}

}  // extern "C"
