// Exact (x0, x1, target) -> last-axis coordinate solve on a 3-D table for gfx950: the (mass, age, [Fe/H]) -> EEP
// inversion.  See include/isochrones_amd_solve.h for the definition and DESIGN.md section 12 for why a bisection.
//
// One kernel, one query per lane, float64:
//   k_solve_last_axis  brackets x0 and x1 once (corner weights and the four row offsets are per-query constants), then
//                      bisects k over the intersection of the four corner columns' finite ranges - each round reads the
//                      four corner values at one k - and ends with one linear inverse and one coalesced store.  A
//                      query whose corner columns have a NaN inside their range walks the range in order instead
//                      (the definition asks for the smallest k, and a hole makes g(k) >= target non-monotone).
//
// g(k) follows the interpolator's arithmetic term by term (oracle/iso_oracle.c: orc_interp_value): weight =
// ((1 * w0) * w1) * w2, values accumulated from 0.0 in corner order, the last axis fastest, no fused multiply-adds
// (the library is built with -ffp-contract=off).  At a knot the weight along the last axis is exactly 0 or 1, so inside
// a hole-free range the four zero-weight corners add +-0 and are not read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "isochrones_amd_solve.h"
#include "../common/grid_cell.h"
#include "../common/last_error.h"

namespace {

constexpr int BLOCK = 256;

struct Corners {
    double w00, w01, w10, w11;      // weights over (ax0, ax1)
    int r00, r01, r10, r11;         // offsets of the four corner columns in col
};

// g(k) inside a hole-free range: the four corners at k (the other four have weight 0 and finite values)
__device__ __forceinline__ double g_knot(const double* __restrict__ col, const Corners& c, int k) {
    return ((col[c.r00 + k] * c.w00 + col[c.r01 + k] * c.w01) + col[c.r10 + k] * c.w10) + col[c.r11 + k] * c.w11;
}

// g(k) with all eight corners multiplied, as the interpolator does it: a NaN next to the knot gives NaN
__device__ __forceinline__ double g_full(const double* __restrict__ col, const Corners& c, int k, int nk) {
    const bool top = k == nk - 1;               // the last knot: cell below it, t = 1
    const int kk = top ? k - 1 : k;
    const double lo = top ? 0.0 : 1.0, hi = top ? 1.0 : 0.0;
    double v = 0.0;
    v += col[c.r00 + kk] * (c.w00 * lo);
    v += col[c.r00 + kk + 1] * (c.w00 * hi);
    v += col[c.r01 + kk] * (c.w01 * lo);
    v += col[c.r01 + kk + 1] * (c.w01 * hi);
    v += col[c.r10 + kk] * (c.w10 * lo);
    v += col[c.r10 + kk + 1] * (c.w10 * hi);
    v += col[c.r11 + kk] * (c.w11 * lo);
    v += col[c.r11 + kk + 1] * (c.w11 * hi);
    return v;
}

__global__ void __launch_bounds__(BLOCK) k_solve_last_axis(const iso_solve_table T, const double* __restrict__ x0,
                                                           const double* __restrict__ x1,
                                                           const double* __restrict__ target, int64_t n,
                                                           double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const double a = x0[q], b = x1[q], y = target[q];
    const int n0 = T.n0, n1 = T.n1, nk = T.nk;
    double e = qnan();
    if (on_axis(T.ax0, n0, a) && on_axis(T.ax1, n1, b) && y == y) {     // a NaN target has no k*
        int i, j;
        double t0, t1;
        bracket(T.ax0, n0, a, i, t0);
        bracket(T.ax1, n1, b, j, t1);
        Corners c;
        c.w00 = (1 - t0) * (1 - t1);
        c.w01 = (1 - t0) * t1;
        c.w10 = t0 * (1 - t1);
        c.w11 = t0 * t1;
        const int cell = i * n1 + j;
        c.r00 = cell * nk;
        c.r01 = c.r00 + nk;
        c.r10 = c.r00 + n1 * nk;
        c.r11 = c.r10 + nk;
        const int2* __restrict__ rng = reinterpret_cast<const int2*>(T.range);
        const int2 q00 = rng[cell], q01 = rng[cell + 1], q10 = rng[cell + n1], q11 = rng[cell + n1 + 1];
        const int holes = (q00.x | q01.x | q10.x | q11.x) & ISO_SOLVE_HOLE_BIT;
        const int mask = ~ISO_SOLVE_HOLE_BIT;
        const int F = max(max(max(q00.x & mask, q01.x & mask), max(q10.x & mask, q11.x & mask)), 0);
        const int L = min(min(min(q00.y, q01.y), min(q10.y, q11.y)), nk - 1);
        const double* __restrict__ col = T.col;
        const double* __restrict__ axk = T.axk;
        if (!holes) {
            // g is finite on [F, H]: below the last table knot g(L) reads the NaN pad at L + 1; on the last table knot it
            // reads L - 1, which has to be inside the range
            const int H = (L == nk - 1 && F < L) ? L : L - 1;
            if (F <= H) {
                double glo = g_knot(col, c, F);
                if (glo >= y) {
                    if (glo == y) e = axk[F];
                } else {
                    double ghi = g_knot(col, c, H);
                    if (ghi >= y) {
                        int lo = F, hi = H;                 // g(lo) < y <= g(hi)
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            const double gm = g_knot(col, c, mid);
                            const bool up = gm >= y;
                            hi = up ? mid : hi;
                            ghi = up ? gm : ghi;
                            lo = up ? lo : mid;
                            glo = up ? glo : gm;
                        }
                        const double elo = axk[lo];
                        e = elo + (y - glo) / (ghi - glo) * (axk[hi] - elo);
                    }
                }
            }
        } else {
            double prev = qnan();
            for (int k = F; k <= L; ++k) {
                const double g = g_full(col, c, k, nk);
                if (g >= y) {
                    if (k == F) {
                        if (g == y) e = axk[k];
                    } else if (prev == prev) {
                        const double elo = axk[k - 1];
                        e = elo + (y - prev) / (g - prev) * (axk[k] - elo);
                    }
                    break;
                }
                prev = g;
            }
        }
    }
    out[q] = e;
}

int check_table(const iso_solve_table* t, const char*& why) {
    if (!t || !t->col || !t->ax0 || !t->ax1 || !t->axk || !t->range) {
        why = "null table pointer";
        return 1;
    }
    if (t->n0 < 2 || t->n1 < 2 || t->nk < 2) {
        why = "every axis needs at least 2 nodes";
        return 1;
    }
    if ((int64_t)t->n0 * t->n1 * t->nk > INT32_MAX) {
        why = "table too large (more than 2^31 - 1 entries)";
        return 1;
    }
    return 0;
}

int launch(const iso_solve_table* t, const double* x0, const double* x1, const double* target, int64_t n, double* out,
           hipStream_t st) {
    const int64_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > INT32_MAX) return fail(ISO_SOLVE_ERR_INVALID, "iso_solve: too many queries in one call (split the batch)");
    hipLaunchKernelGGL(k_solve_last_axis, dim3((unsigned)blocks), dim3(BLOCK), 0, st, *t, x0, x1, target, n, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISO_SOLVE_ERR_HIP, hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

const char* iso_solve_version(void) { return "isochrones_amd solve 1"; }

const char* iso_solve_last_error(void) { return g_err; }

int iso_solve_last_axis(const iso_solve_table* table, const double* x0, const double* x1, const double* target,
                        int64_t n, double* out, void* stream) {
    g_err[0] = 0;
    const char* why = nullptr;
    if (check_table(table, why)) return fail(ISO_SOLVE_ERR_INVALID, why);
    if (n < 0) return fail(ISO_SOLVE_ERR_INVALID, "iso_solve_last_axis: n < 0");
    if (n == 0) return 0;
    if (!x0 || !x1 || !target || !out) return fail(ISO_SOLVE_ERR_INVALID, "iso_solve_last_axis: null pointer");
    return launch(table, x0, x1, target, n, out, (hipStream_t)stream);
}

int iso_solve_last_axis_host(const iso_solve_table* table, const double* x0, const double* x1, const double* target,
                             int64_t n, double* out, double* stage, void* stream) {
    g_err[0] = 0;
    const char* why = nullptr;
    if (check_table(table, why)) return fail(ISO_SOLVE_ERR_INVALID, why);
    if (n < 0) return fail(ISO_SOLVE_ERR_INVALID, "iso_solve_last_axis_host: n < 0");
    if (n == 0) return 0;
    if (!x0 || !x1 || !target || !out || !stage)
        return fail(ISO_SOLVE_ERR_INVALID, "iso_solve_last_axis_host: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)n * sizeof(double);
    const double* src[3] = {x0, x1, target};
    for (int d = 0; d < 3; ++d) {
        const hipError_t e = hipMemcpyAsync(stage + d * n, src[d], bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(ISO_SOLVE_ERR_HIP, hipGetErrorString(e));
    }
    const int rc = launch(table, stage, stage + n, stage + 2 * n, n, stage + 3 * n, st);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(out, stage + 3 * n, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // the result is host data: wait for this stream
    if (e != hipSuccess) return fail(ISO_SOLVE_ERR_HIP, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
