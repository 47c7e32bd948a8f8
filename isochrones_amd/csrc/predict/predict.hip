// Posterior-predictive check of a stored ensemble chain, for gfx950.  See include/isochrones_amd_predict.h for the
// definition, the order of the arithmetic and the summation order; DESIGN.md section 15 for the mapping and what bounds the
// kernel.
//
// One kernel, float64:
//   k_predict_chain  one workgroup of 128 lanes per ensemble (workgroups stride over the ensemble range).  Lane l takes the
//                    samples s = t * W + walker with s mod 128 == l, so a wavefront reads runs of consecutive walkers - the
//                    contiguous axis of the parameter-major storage - and stores the magnitude rows the same way.  A sample
//                    interpolates the four model columns per component, brackets the BC grid once per component and reads
//                    its sixteen corners, eight adjacent bands at a time (more than 8 bands: one pass per chunk of 8).  The
//                    sample's z terms wait in LDS until every band has said whether the sample is good, then go to the
//                    lane's partial sums, also in LDS; the partials are combined by the fixed tree of the header.  The MAP
//                    is an argmax over lnprob with the same lane mapping and an (value, index) tree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "isochrones_amd_predict.h"
#include "../common/chain_view.h"
#include "../common/grid_interp.h"

namespace {

constexpr int BLOCK = ISO_PREDICT_LANES;
constexpr int MAX_BLOCKS = ISO_PREDICT_MAX_BLOCKS;      // eight workgroups per CU, the rest by striding
constexpr int MAXC = ISO_PREDICT_MAX_COMPS;
constexpr int CH = 8;                           // bands per pass
constexpr int NSPEC = ISO_PREDICT_NSPEC;
static_assert(ISO_PREDICT_ROW_MAJOR == CHAIN_ROW_MAJOR && ISO_PREDICT_PARAM_MAJOR == CHAIN_PARAM_MAJOR, "chain layouts");

struct Args {
    const double* chain;
    const double* lnprob;
    const double* obs_val;
    const double* obs_unc;
    iso_predict_out O;
    iso_predict_model_table M;
    iso_predict_bc_table T;
    ChainStrides st;
    int64_t rows;                               // n_ens * W
    int32_t W, C, nsteps, ndim, B, i_dist, i_AV, ens_begin, n_ens_out;
    int32_t n;                                  // nsteps * W samples an ensemble
    int32_t comp[MAXC];                         // pack_comp()
};

__host__ __device__ inline bool finite_(double x) { return x - x == 0.0; }

// steps 1 to 5 for one sample and the bands [b0, b0 + nb): the system magnitudes and component 0's (Teff, logg, feh).
// wk[j * ws], j < 2 * CH: working space of a multiple system (the kernel's is LDS: pow and log10 then run in loops over
// the bands instead of eight unrolled copies held in registers)
__host__ __device__ inline void sample_chunk(const Args& A, const double* __restrict__ row, int b0, int nb, double dist,
                                             double av, double (&mag)[CH], double (&spec)[3], double* __restrict__ wk,
                                             int ws) {
    const double dm = 5 * log10(dist / 10.0);
    if (A.C > 1)
        for (int j = 0; j < nb; ++j) wk[(CH + j) * ws] = 0.0;
    for (int c = 0; c < A.C; ++c) {
        const int comp = c == 0 ? A.comp[0] : (c == 1 ? A.comp[1] : A.comp[2]);
        const double x0 = row[comp_p0(comp) * A.st.st_d], x1 = row[comp_p1(comp) * A.st.st_d],
                     xk = row[comp_pk(comp) * A.st.st_d];
        double v[4], bcv[CH];
        cell3(A.M, 4, x0, x1, xk, v);                           // step 1 of the header: (Teff, logg, feh, Mbol)
        bc_chunk<CH>(A.T, v[0], v[1], v[2], av, b0, nb, bcv);   // step 2
        if (c == 0) {
            spec[0] = v[0];
            spec[1] = v[1];
            spec[2] = v[2];
        }
        const double base = v[3] + dm;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if (j >= nb) continue;
            const double m = base - bcv[j];
            if (A.C == 1) mag[j] = m;
            else wk[j * ws] = m;
        }
        if (A.C > 1) {
#pragma nounroll
            for (int j = 0; j < nb; ++j) wk[(CH + j) * ws] = wk[(CH + j) * ws] + pow(10.0, -0.4 * wk[j * ws]);
        }
    }
    if (A.C > 1) {
#pragma nounroll
        for (int j = 0; j < nb; ++j) wk[j * ws] = -2.5 * log10(wk[(CH + j) * ws]);
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (j < nb) mag[j] = wk[j * ws];
    }
}

__host__ __device__ inline double zterm(double val, double unc, double model) {
    const double d = val - model;
    return (d * d) / (unc * unc);
}

// One sample: magnitudes stored, z terms of the present terms into zt[j * zs] (j < B + 4).  Returns whether it is good.
__host__ __device__ inline bool sample(const Args& A, int e, int s, const double* __restrict__ ov,
                                       const double* __restrict__ ou, double* __restrict__ zt, int zs,
                                       double* __restrict__ wk, int ws, int* __restrict__ nanc) {
    const int t = s / A.W, w = s - t * A.W;
    const int64_t r = (int64_t)e * A.W + w, R = (int64_t)A.n_ens_out * A.W;
    const double* __restrict__ row = A.chain + (int64_t)t * A.st.st_t + ((int64_t)A.ens_begin * A.W + r) * A.st.st_w;
    const double dist = row[A.i_dist * A.st.st_d], av = row[A.i_AV * A.st.st_d];
    bool bad = false;
    double spec[3] = {0.0, 0.0, 0.0};
    for (int b0 = 0; b0 < A.B; b0 += CH) {
        const int nb = A.B - b0 < CH ? A.B - b0 : CH;
        double mag[CH];
        sample_chunk(A, row, b0, nb, dist, av, mag, spec, wk, ws);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if (j >= nb) continue;
            if (A.O.mags) A.O.mags[((int64_t)t * A.B + b0 + j) * R + r] = mag[j];
            if (mag[j] != mag[j]) {
#ifdef __HIP_DEVICE_COMPILE__
                atomicAdd(nanc + b0 + j, 1);                    // an integer count in LDS: the order does not matter
#else
                ++nanc[b0 + j];
#endif
            }
            const double val = ov[b0 + j];
            if (val == val) {
                bad |= !finite_(mag[j]);
                zt[(b0 + j) * zs] = zterm(val, ou[b0 + j], mag[j]);
            }
        }
    }
    const double model[NSPEC] = {spec[0], spec[1], spec[2], 1000.0 / dist};
#pragma unroll
    for (int q = 0; q < NSPEC; ++q) {
        const double val = ov[A.B + q];
        if (val == val) {
            bad |= !finite_(model[q]);
            zt[(A.B + q) * zs] = zterm(val, ou[A.B + q], model[q]);
        }
    }
    return !bad;
}

// (value, index) of the better of two MAP candidates: an index of -1 is no candidate; the larger value, then the lower index
__host__ __device__ inline void better(double& v, int64_t& i, double v2, int64_t i2) {
    if (i2 >= 0 && (i < 0 || v2 > v || (v2 == v && i2 < i))) {
        v = v2;
        i = i2;
    }
}

__global__ void __launch_bounds__(BLOCK) k_predict_chain(const Args A_) {
    extern __shared__ double lds[];
    __shared__ Args s_args;
    for (int i = (int)threadIdx.x; i < (int)(sizeof(Args) / 4); i += BLOCK)
        reinterpret_cast<int32_t*>(&s_args)[i] = reinterpret_cast<const int32_t*>(&A_)[i];
    __syncthreads();
    const Args& A = s_args;
    __shared__ int s_bad;
    __shared__ int s_nan[ISO_PREDICT_MAX_BANDS];
    __shared__ double s_val[BLOCK];
    __shared__ long long s_idx[BLOCK];
    const int NT = A.B + NSPEC, lane = (int)threadIdx.x;
    double* __restrict__ acc = lds;                             // [NT][BLOCK]  partial sums of the header
    double* __restrict__ tmp = lds + NT * BLOCK;                // [NT][BLOCK]  the sample in flight
    double* __restrict__ wk = tmp + NT * BLOCK;                 // [2 * CH][BLOCK]  sample_chunk's working space
    for (int e = blockIdx.x; e < A.n_ens_out; e += gridDim.x) {
        const double* __restrict__ ov = A.obs_val + (int64_t)(A.ens_begin + e) * NT;
        const double* __restrict__ ou = A.obs_unc + (int64_t)(A.ens_begin + e) * NT;
        for (int j = 0; j < NT; ++j) acc[j * BLOCK + lane] = 0.0;
        if (lane == 0) s_bad = 0;
        if (lane < ISO_PREDICT_MAX_BANDS) s_nan[lane] = 0;
        __syncthreads();
        int bad = 0;
        for (int s = lane; s < A.n; s += BLOCK) {
            if (sample(A, e, s, ov, ou, tmp + lane, BLOCK, wk + lane, BLOCK, s_nan)) {
                for (int j = 0; j < NT; ++j)
                    if (ov[j] == ov[j]) acc[j * BLOCK + lane] = acc[j * BLOCK + lane] + tmp[j * BLOCK + lane];
            } else {
                ++bad;
            }
        }
        if (bad) atomicAdd(&s_bad, bad);
        __syncthreads();
        for (int h = BLOCK / 2; h > 0; h >>= 1) {
            if (lane < h)
                for (int j = 0; j < NT; ++j) acc[j * BLOCK + lane] = acc[j * BLOCK + lane] + acc[j * BLOCK + lane + h];
            __syncthreads();
        }
        const int nbad = s_bad;
        const double ngood = (double)(A.n - nbad);
        for (int j = lane; j < NT; j += BLOCK) {
            const double mean = ov[j] == ov[j] ? acc[j * BLOCK] / ngood : qnan();
            if (A.O.term_chi2) A.O.term_chi2[(int64_t)e * NT + j] = mean;
            tmp[j * BLOCK] = mean;
        }
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;
            int np = 0;
            for (int j = 0; j < NT; ++j)
                if (ov[j] == ov[j]) {
                    sum = sum + tmp[j * BLOCK];
                    ++np;
                }
            if (A.O.ppc) A.O.ppc[e] = np > 0 ? sum / (double)np : qnan();
            if (A.O.n_bad) A.O.n_bad[e] = nbad;
        }
        if (A.O.mag_nan && lane < A.B) A.O.mag_nan[(int64_t)e * A.B + lane] = s_nan[lane];
        if (A.lnprob && (A.O.map_index || A.O.map_pars)) {
            double bv = 0.0;
            int64_t bi = -1;
            for (int s = lane; s < A.n; s += BLOCK) {
                const int t = s / A.W, w = s - t * A.W;
                const double lp = A.lnprob[(int64_t)t * A.rows + (int64_t)(A.ens_begin + e) * A.W + w];
                if (lp == lp) better(bv, bi, lp, s);
            }
            s_val[lane] = bv;
            s_idx[lane] = bi;
            __syncthreads();
            for (int h = BLOCK / 2; h > 0; h >>= 1) {
                if (lane < h) {
                    double v = s_val[lane];
                    int64_t i = s_idx[lane];
                    better(v, i, s_val[lane + h], s_idx[lane + h]);
                    s_val[lane] = v;
                    s_idx[lane] = i;
                }
                __syncthreads();
            }
            const int64_t best = s_idx[0];
            if (lane == 0 && A.O.map_index) A.O.map_index[e] = best;
            if (A.O.map_pars) {
                const int t = best < 0 ? 0 : (int)(best / A.W), w = best < 0 ? 0 : (int)(best - (int64_t)t * A.W);
                const double* __restrict__ row =
                    A.chain + (int64_t)t * A.st.st_t + ((int64_t)(A.ens_begin + e) * A.W + w) * A.st.st_w;
                for (int d = lane; d < A.ndim; d += BLOCK)
                    A.O.map_pars[(int64_t)e * A.ndim + d] = best < 0 ? qnan() : row[d * A.st.st_d];
            }
        }
        __syncthreads();                                        // the next ensemble reuses the LDS
    }
}

size_t lds_bytes(int B) { return (size_t)(2 * (B + NSPEC) + 2 * CH) * BLOCK * sizeof(double); }

// arguments checked, strides filled in
int prepare(const char* who, const iso_predict_model_table* m, const iso_predict_bc_table* bc, const double* chain,
            const double* lnprob, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim, int32_t ens_begin,
            int32_t n_ens_out, const int32_t* comps, int32_t C, int32_t i_dist, int32_t i_AV, const double* obs_val,
            const double* obs_unc, const iso_predict_out* out, Args& A) {
    const ChainShape s{layout, nsteps, n_ens, W, ndim, ens_begin, n_ens_out, comps, C};
    const char* why = nullptr;
    if (!m || !m->cols || !m->ax0 || !m->ax1 || !m->axk) why = "null model table pointer";
    else if (!bc || !bc->bc || !bc->axT || !bc->axg || !bc->axf || !bc->axA) why = "null BC table pointer";
    else if (!chain || !comps || !obs_val || !obs_unc || !out) why = "null pointer";
    else if ((why = chain_shape_error(CHAIN_CHECK_LAYOUT | CHAIN_CHECK_SIZES, s))) {}
    else if (bc->B < 1 || bc->B > ISO_PREDICT_MAX_BANDS) why = "B must be 1 to 32 bands";
    else if (C < 1 || C > ISO_PREDICT_MAX_COMPS) why = "C must be 1 to 3 components";
    else if (m->n0 < 2 || m->n1 < 2 || m->nk < 2) why = "every model axis needs at least 2 nodes";
    else if (bc->nT < 2 || bc->ng < 2 || bc->nf < 2 || bc->nA < 2) why = "every BC axis needs at least 2 nodes";
    else if ((int64_t)m->n0 * m->n1 * m->nk * 4 > INT32_MAX) why = "model table too large (more than 2^31 - 1 entries)";
    else if ((double)bc->nT * bc->ng * bc->nf * bc->nA * bc->B > (double)INT32_MAX)
        why = "BC table too large (more than 2^31 - 1 entries)";
    else if ((why = chain_shape_error(CHAIN_CHECK_RANGE | CHAIN_CHECK_ROWS, s))) {}
    else if (nsteps * W > INT32_MAX) why = "more than 2^31 - 1 samples an ensemble";
    else if (ndim > 256) why = "more than 256 parameters";
    else if (i_dist < 0 || i_dist >= ndim) why = "i_dist is outside [0, ndim)";
    else if (i_AV < 0 || i_AV >= ndim) why = "i_AV is outside [0, ndim)";
    else why = chain_shape_error(CHAIN_CHECK_COMPS, s);
    if (why) return fail(ISO_PREDICT_ERR_INVALID, who, why);
    const int64_t rows = (int64_t)n_ens * W;
    A.st = chain_strides(layout, rows, ndim);
    A.chain = chain;
    A.lnprob = lnprob;
    A.obs_val = obs_val;
    A.obs_unc = obs_unc;
    A.O = *out;
    A.M = *m;
    A.T = *bc;
    A.rows = rows;
    A.W = W;
    A.C = C;
    A.nsteps = (int32_t)nsteps;
    A.ndim = ndim;
    A.B = bc->B;
    A.i_dist = i_dist;
    A.i_AV = i_AV;
    A.ens_begin = ens_begin;
    A.n_ens_out = n_ens_out;
    A.n = (int32_t)(nsteps * W);
    for (int c = 0; c < MAXC; ++c)
        A.comp[c] = c < C ? pack_comp(comps[3 * c], comps[3 * c + 1], comps[3 * c + 2]) : 0;
    return 0;
}

}  // namespace

extern "C" {

const char* iso_predict_version(void) { return "isochrones_amd predict 1"; }

const char* iso_predict_last_error(void) { return g_err; }

int iso_predict_chain(const iso_predict_model_table* model, const iso_predict_bc_table* bc, const double* chain,
                      const double* lnprob, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                      int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C, int32_t i_dist, int32_t i_AV,
                      const double* obs_val, const double* obs_unc, const iso_predict_out* out, void* stream) {
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_predict_chain", model, bc, chain, lnprob, layout, nsteps, n_ens, W, ndim, ens_begin,
                           n_ens_out, comps, C, i_dist, i_AV, obs_val, obs_unc, out, A);
    if (rc) return rc;
    const size_t lds = lds_bytes(A.B);
    // function attributes are per device: raise the limit before every large launch, on whichever device is current
    if (lds > 60 * 1024 &&
        hipFuncSetAttribute((const void*)k_predict_chain, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
        return fail(ISO_PREDICT_ERR_HIP, "iso_predict_chain: hipFuncSetAttribute failed");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = n_ens_out < MAX_BLOCKS ? n_ens_out : MAX_BLOCKS;
    hipLaunchKernelGGL(k_predict_chain, dim3((unsigned)blocks), dim3(BLOCK), lds, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_PREDICT_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int iso_predict_chain_host(const iso_predict_model_table* model, const iso_predict_bc_table* bc, const double* chain,
                           const double* lnprob, int layout, int64_t nsteps, int32_t n_ens, int32_t W, int32_t ndim,
                           int32_t ens_begin, int32_t n_ens_out, const int32_t* comps, int32_t C, int32_t i_dist,
                           int32_t i_AV, const double* obs_val, const double* obs_unc, const iso_predict_out* out,
                           void* stream) {
    (void)stream;
    g_err[0] = 0;
    Args A;
    const int rc = prepare("iso_predict_chain_host", model, bc, chain, lnprob, layout, nsteps, n_ens, W, ndim, ens_begin,
                           n_ens_out, comps, C, i_dist, i_AV, obs_val, obs_unc, out, A);
    if (rc) return rc;
    constexpr int MAXT = ISO_PREDICT_MAX_BANDS + NSPEC;
    const int NT = A.B + NSPEC;
    static thread_local double acc[MAXT][BLOCK];
    for (int e = 0; e < n_ens_out; ++e) {
        const double* ov = obs_val + (int64_t)(ens_begin + e) * NT;
        const double* ou = obs_unc + (int64_t)(ens_begin + e) * NT;
        int nbad = 0;
        int nanc[ISO_PREDICT_MAX_BANDS] = {0};
        for (int l = 0; l < BLOCK; ++l) {
            for (int j = 0; j < NT; ++j) acc[j][l] = 0.0;
            for (int s = l; s < A.n; s += BLOCK) {
                double z[MAXT], wk[2 * CH];
                if (sample(A, e, s, ov, ou, z, 1, wk, 1, nanc)) {
                    for (int j = 0; j < NT; ++j)
                        if (ov[j] == ov[j]) acc[j][l] = acc[j][l] + z[j];
                } else {
                    ++nbad;
                }
            }
        }
        for (int h = BLOCK / 2; h > 0; h >>= 1)
            for (int l = 0; l < h; ++l)
                for (int j = 0; j < NT; ++j) acc[j][l] = acc[j][l] + acc[j][l + h];
        const double ngood = (double)(A.n - nbad);
        double sum = 0.0;
        int np = 0;
        for (int j = 0; j < NT; ++j) {
            const double mean = ov[j] == ov[j] ? acc[j][0] / ngood : qnan();
            if (out->term_chi2) out->term_chi2[(int64_t)e * NT + j] = mean;
            if (ov[j] == ov[j]) {
                sum = sum + mean;
                ++np;
            }
        }
        if (out->ppc) out->ppc[e] = np > 0 ? sum / (double)np : qnan();
        if (out->n_bad) out->n_bad[e] = nbad;
        if (out->mag_nan)
            for (int j = 0; j < A.B; ++j) out->mag_nan[(int64_t)e * A.B + j] = nanc[j];
        if (lnprob && (out->map_index || out->map_pars)) {
            double bv = 0.0;
            int64_t bi = -1;
            for (int s = 0; s < A.n; ++s) {
                const int t = s / W, w = s - t * W;
                const double lp = lnprob[(int64_t)t * A.rows + (int64_t)(ens_begin + e) * W + w];
                if (lp == lp) better(bv, bi, lp, s);
            }
            if (out->map_index) out->map_index[e] = bi;
            if (out->map_pars) {
                const int t = bi < 0 ? 0 : (int)(bi / W), w = bi < 0 ? 0 : (int)(bi - (int64_t)t * W);
                const double* row = chain + (int64_t)t * A.st.st_t + ((int64_t)(ens_begin + e) * W + w) * A.st.st_w;
                for (int d = 0; d < ndim; ++d) out->map_pars[(int64_t)e * ndim + d] = bi < 0 ? qnan() : row[d * A.st.st_d];
            }
        }
    }
    return 0;
}

}  // extern "C"
