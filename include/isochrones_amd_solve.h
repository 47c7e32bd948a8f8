/* C ABI of libiso_solve.so: exact inversion of one column along the last axis of a 3-D table, for gfx950.
 *
 * This is the (mass, age, [Fe/H]) -> EEP solve (the job of the reference's get_eep_accurate, isochrones/models.py:544-578,
 * without the optimiser).  For a track table the axes are ([Fe/H], mass, EEP) and the column is `age`; for an isochrone
 * table they are (age, [Fe/H], EEP) and the column is `initial_mass`.
 *
 * For one query (x0, x1, target) let g(k) be the trilinear interpolation of the column at (x0, x1, axk[k]), with the
 * interpolator's own rules: a query on a node takes the cell above it (the last node: the cell below, weight 1), every
 * corner of the cell is multiplied by its weight even when that weight is zero (a NaN neighbour gives NaN), a NaN or
 * out-of-axis coordinate gives NaN (the bracket and the on-axis rule are the lines the other grid libraries compile, the
 * internal csrc/common/grid_cell.h).  The search range is the intersection of the [first, last] finite ranges of the four
 * corner columns.  With k* the smallest index of the range with g(k*) >= target:
 *
 *   k* is the first index of the range and g(k*) == target          axk[k*]
 *   k* is the first index of the range and g(k*) >  target          NaN
 *   no k*                                                           NaN
 *   g(k*) or g(k* - 1) is NaN (a hole inside the range)             NaN
 *   a NaN or out-of-axis query                                      NaN
 *   otherwise     axk[k*-1] + (target - g(k*-1)) / (g(k*) - g(k*-1)) * (axk[k*] - axk[k*-1])
 *
 * The column must be nondecreasing along the last axis inside every (i, j)'s finite range; the caller has checked that
 * (the library takes it as given: a bisection over k finds k*).
 *
 * The library allocates nothing, starts no resident waves and launches on device pointers the caller owns, on the
 * stream it is given.  iso_solve_last_axis does not synchronise.  iso_solve_last_axis_host returns host data, so it
 * waits for the given stream (and only for it) before it returns.  Return codes: 0 ok, ISO_SOLVE_ERR_INVALID for a bad
 * argument, ISO_SOLVE_ERR_HIP for a failed runtime call (iso_solve_last_error() says which).
 */
#ifndef ISOCHRONES_AMD_SOLVE_H
#define ISOCHRONES_AMD_SOLVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_SOLVE_ERR_INVALID (-1)
#define ISO_SOLVE_ERR_HIP (-2)
/* bit of range[..][0] that says: this column has a NaN between its first and last finite entry */
#define ISO_SOLVE_HOLE_BIT 0x40000000

/* One table prepared for solving; every pointer is a device pointer the caller owns.
 *   col    [n0][n1][nk]     the column, NaN-padded
 *   ax0, ax1, axk           the axes, strictly increasing, n0, n1, nk >= 2 entries
 *   range  [n0][n1][2]      first (| ISO_SOLVE_HOLE_BIT) and last finite index of every column; first > last for a
 *                           column with no finite entry */
typedef struct iso_solve_table {
    const double* col;
    const double* ax0;
    const double* ax1;
    const double* axk;
    const int32_t* range;
    int32_t n0, n1, nk;
} iso_solve_table;

const char* iso_solve_version(void);
const char* iso_solve_last_error(void);

/* out[q] for q < n; x0, x1, target, out: device arrays of n doubles */
int iso_solve_last_axis(const iso_solve_table* table, const double* x0, const double* x1, const double* target,
                        int64_t n, double* out, void* stream);

/* the same for host arrays of n doubles; stage: a device buffer of 4 n doubles the caller owns */
int iso_solve_last_axis_host(const iso_solve_table* table, const double* x0, const double* x1, const double* target,
                             int64_t n, double* out, double* stage, void* stream);

#ifdef __cplusplus
}
#endif

#endif
