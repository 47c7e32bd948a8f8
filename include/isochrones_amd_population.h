/* C ABI of libiso_population.so: a batch of coeval systems of one or two stars evaluated on a model grid and a
 * bolometric-correction grid, for gfx950.  Per component the model columns at its grid coordinates, its apparent
 * magnitudes and its per-band extinctions; per system the combined magnitudes and extinctions, the reference's
 * generate_binary(..., all_As=True) (isochrones/models.py:580-661) without the EEP estimate, which the caller has made.
 * The call draws no random numbers, solves for no EEP and loops over no rejections: it is the evaluation alone.
 *
 * Model table.  cols[n0][n1][nk][Q]: Q columns of a 3-D model grid, the Q values of one node adjacent, NaN-padded as the
 * grid is, with its axes ax0, ax1, axk (strictly increasing, at least 2 nodes each): the layout and the rules of
 * iso_derived_table (isochrones_amd_derived.h).  4 <= Q <= ISO_POPULATION_MAX_COLS.  hot[4]: the indices in [0, Q) of
 * the columns Teff, logg, feh and Mbol, in that order.  n0 * n1 * nk * Q <= 2^31 - 1.
 *
 * Bolometric-correction table.  bc[nT][ng][nf][nA][B]: B selected band columns of the 4-D grid on (Teff, logg, [Fe/H],
 * AV), the B values of one node adjacent, with its axes axT, axg, axf, axA (strictly increasing, at least 2 nodes each):
 * the layout of iso_predict_bc_table (isochrones_amd_predict.h).  1 <= B <= ISO_POPULATION_MAX_BANDS.
 * nT * ng * nf * nA * B <= 2^31 - 1.
 *
 * Inputs, float64, read in place, N systems of C components (C is 1 or 2), 0 <= N <= 2^31 - 1:
 *   coords[(c * 3 + a) * N + i]   the coordinate of component c < C of system i on axis a of (ax0, ax1, axk)
 *   distance[i]                   pc
 *   AV[i]
 *
 * One component.  Every operation is one IEEE float64 operation rounded on its own, in the order written; no fused
 * multiply-add anywhere (the library is built with -ffp-contract=off and writes no fma).
 *   1. value[q], q < Q = the model columns at (x0, x1, xk), trilinear, by the rules of isochrones_amd_derived.h: per axis
 *      i = the largest index with ax[i] <= x but at most n - 2, t = (x - ax[i]) / (ax[i + 1] - ax[i]), u = 1 - t; the
 *      eight corners in the order (b0, b1, bk) = 000, 001, ... 111 (bk fastest), weight (f0 * f1) * fk with f = t where
 *      the bit is 1 and u where it is 0; value[q] = 0.0, then value[q] + cols[corner][q] * weight per corner.  A NaN
 *      coordinate or one off its axis gives NaN for all Q columns; a NaN neighbour propagates (every corner is multiplied
 *      by its weight even when that weight is zero).
 *      (Teff, logg, feh, Mbol) = value[hot[0 .. 3]].
 *   2. bc_c[b], b < B = the band columns at (Teff, logg, feh, AV) by the same rule in four dimensions (steps 2 and 3 of
 *      isochrones_amd_predict.h): the sixteen corners in the order (bT, bg, bf, bA) = 0000, 0001, ... 1111 (bA fastest),
 *      weight ((fT * fg) * ff) * fA, value = 0.0 then value + node * weight; a NaN coordinate or one outside its axis
 *      gives NaN for every band.  bc0_c[b] is the same at AV = 0.0: index, t and u on the T, g and f axes are those of
 *      bc_c (the same numbers from the same operations), only the bracket on axA differs.
 *   3. mag_c[b]  = (Mbol + 5 * log10(distance / 10)) - bc_c[b]
 *      true_c[b] = (Mbol + 5 * log10(distance / 10)) - bc0_c[b]
 *      A_c[b]    = mag_c[b] - true_c[b]
 *
 * The system.  For C = 1: sys_mag[b] = mag_0[b] and sys_A[b] = A_0[b].  For C = 2, with the reference's fillna of
 * models.py:651-659:
 *      m1 = isnan(mag_1[b]) ? +inf : mag_1[b]
 *      a1 = isnan(A_1[b]) ? 0.0 : A_1[b]
 *      sys_mag[b] = -2.5 * log10((0.0 + pow(10, -0.4 * mag_0[b])) + pow(10, -0.4 * m1))
 *      sys_A[b]   = sys_mag[b] - (-2.5 * log10((0.0 + pow(10, -0.4 * (mag_0[b] - A_0[b]))) + pow(10, -0.4 * (m1 - a1))))
 * so an absent or off-grid secondary leaves the primary's light and a NaN primary gives NaN.
 * log10 and pow are the math library's of the side that runs (device or host), so a magnitude or an extinction of the
 * kernel and one of the host entry may differ in the last bits; the model columns are the same bits on both sides, and
 * the bits iso_derived_chain gives for the same table and point (steps 1 and 2 are one statement, the internal
 * csrc/common/grid_interp.h, compiled for both kernels and both host entries).
 *
 * Outputs, float64, structure-of-arrays with i fastest, every one skipped when its pointer is null:
 *   cols_out[(c * Q + q) * N + i]   value[q] of component c
 *   mag_out[(c * B + b) * N + i]    mag_c[b]
 *   A_out[(c * B + b) * N + i]      A_c[b]
 *   sys_mag[b * N + i]
 *   sys_A[b * N + i]
 * A system's outputs depend on its own inputs and the tables only: they are bit-identical alone and in any batch.
 *
 * The library allocates nothing and works on device pointers the caller owns (the structs themselves are host memory,
 * read before the call returns).  iso_population_eval launches one kernel on the given stream and does not synchronise;
 * for an even Q it wants cols 16-byte aligned (a node's columns are read two at a time).  iso_population_eval_host does
 * the same on host pointers in plain C++ with ascending loops and touches no device.  N = 0 is a no-op.  Return codes:
 * 0 ok, ISO_POPULATION_ERR_INVALID for a bad argument (iso_population_last_error() says which),
 * ISO_POPULATION_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_POPULATION_H
#define ISOCHRONES_AMD_POPULATION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_POPULATION_ERR_INVALID (-1)
#define ISO_POPULATION_ERR_HIP (-2)

#define ISO_POPULATION_MAX_COLS 32
#define ISO_POPULATION_MAX_BANDS 32
#define ISO_POPULATION_MAX_COMPS 2
/* the grid's cap: workgroups of 256 lanes; a call of more than 256 * ISO_POPULATION_MAX_BLOCKS systems strides */
#define ISO_POPULATION_MAX_BLOCKS 2048

/* every pointer is a device pointer the caller owns (a host pointer for iso_population_eval_host) */
typedef struct iso_population_model_table {
    const double* cols;
    const double* ax0;
    const double* ax1;
    const double* axk;
    int32_t n0, n1, nk, Q;
    int32_t hot[4];
} iso_population_model_table;

typedef struct iso_population_bc_table {
    const double* bc;
    const double* axT;
    const double* axg;
    const double* axf;
    const double* axA;
    int32_t nT, ng, nf, nA, B, reserved;
} iso_population_bc_table;

/* the outputs of one call; a null pointer skips that output */
typedef struct iso_population_out {
    double* cols_out;
    double* mag_out;
    double* A_out;
    double* sys_mag;
    double* sys_A;
} iso_population_out;

const char* iso_population_version(void);
const char* iso_population_last_error(void);

int iso_population_eval(const iso_population_model_table* model, const iso_population_bc_table* bc, const double* coords,
                        const double* distance, const double* AV, int64_t N, int32_t C, const iso_population_out* out,
                        void* stream);

/* the same on host pointers, in plain C++ (no device is touched; stream is ignored) */
int iso_population_eval_host(const iso_population_model_table* model, const iso_population_bc_table* bc,
                             const double* coords, const double* distance, const double* AV, int64_t N, int32_t C,
                             const iso_population_out* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
