/* C ABI of libiso_nested.so: nested sampling of a catalog (per-star evidences) for gfx950.
 *
 * One launch fits every star of a catalog: one workgroup per star, the live points in LDS ("Nested sampling of
 * a catalog").  The library allocates nothing and does not synchronise: it launches on device pointers the caller owns, on
 * the current device and on the stream it is given.  The catalog's tables and per-star blocks come from libiso_hip.so:
 * iso_catalog_fast_args() copies the catalog's kernel-argument block out, and that block is handed to iso_nested_fit()
 * unchanged (both libraries compile the same definition; the size is checked on both sides).
 *
 * Return codes: 0 ok, ISO_NESTED_ERR_INVALID for a bad argument or a shape without a kernel, ISO_NESTED_ERR_HIP for a failed
 * launch (iso_nested_last_error() says which).
 *
 * Outputs, D = n_stars_per_system + 4 parameters per point:
 *   rows    [n_models][2 D + 8]   mean, std of every parameter | lnZ lnZ_err H ncall niter prior_fraction status ok
 *                                 status: 0 ok, 1 no support found in max_fill_chunks chunks, 2 max_chunks exhausted;
 *                                 a row with ok = 0 carries NaN in its moments, lnZ, lnZ_err and H
 *   dead    [n_models][max_dead][D + 2]  or NULL: unit-cube coordinates, logl, logw + logl of every retired point
 *   n_dead  [n_models] int32             or NULL
 *   trace   [n_models][max_steps][3 + D + D D] or NULL, per macro-step: thr[K - 1], index of the first draw examined and of
 *                                 the last draw consumed (draw index = 256 chunk + lane), the ellipsoid's mean and factor
 *                                 (row-major, lower triangular)
 *   n_steps [n_models] int32             or NULL
 */
#ifndef ISOCHRONES_AMD_NESTED_H
#define ISOCHRONES_AMD_NESTED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_NESTED_MAX_D 7
#define ISO_NESTED_MAX_BANDS 12
#define ISO_NESTED_ERR_INVALID (-1)
#define ISO_NESTED_ERR_HIP (-2)

const char* iso_nested_version(void);
const char* iso_nested_last_error(void);
/* the kernel the last successful iso_nested_fit() of this thread launched, spelled as c++filt spells its symbol */
const char* iso_nested_last_kernel(void);
/* sizeof the kernel-argument block iso_nested_fit() expects (what iso_catalog_fast_args() must be asked for) */
size_t iso_nested_fast_args_size(void);
/* live points retired per macro-step: min(n_live / 10, n_live - 2 (D + 1)), at least 1 */
int iso_nested_remove(int n_live, int n_stars_per_system);
/* the largest n_live whose buffers fit the 160 KB of LDS a workgroup may ask for; below max(20, 4 (D + 1)): no fit possible */
int iso_nested_max_live(int n_stars_per_system, int n_bands, int axes_len);
/* the same for a catalog's kernel-argument block (iso_catalog_fast_args): its staged axes are what the cap depends on */
int iso_nested_max_live_catalog(const void* fast_args, size_t fast_args_size, int n_stars_per_system, int n_bands);

int iso_nested_fit(const void* fast_args, size_t fast_args_size, int kind, int n_stars_per_system, int n_bands,
                   int64_t n_models, const int64_t* global_index, int n_live, double evidence_tolerance, double enlarge,
                   uint64_t seed, int max_iter, int max_fill_chunks, int max_chunks, double* rows, double* dead,
                   int32_t* n_dead, int max_dead, double* trace, int32_t* n_steps, int max_steps, void* stream);

#ifdef __cplusplus
}
#endif

#endif
