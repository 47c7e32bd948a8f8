/* C ABI of libiso_draw.so: random draws of synthetic populations and injection sets, for gfx950.  Every column of every
 * system is an exact inverse distribution function of one or two counter-based uniforms: no rejection loop, no state.
 *
 * Systems and columns.  N systems, C columns, 1 <= C <= ISO_DRAW_MAX_COLS.  The output x is [C][N]: column c of system i at
 * x[c * N + i], so consecutive systems are consecutive doubles.
 *
 * Global number.  System i of a call has the global number j = index[i], index an optional [N] array of int64 (used to
 * redraw chosen systems); without it j = first + i.
 *
 * Random numbers.  Philox4x32-10 under the key (low word of seed, high word of seed) and the counter
 *     (low word of j, high word of j, stream | round << 8, ISO_DRAW_PHILOX_TAG),
 * stream the record's own number 0 .. 255 (a column keeps its numbers wherever it stands among the columns of a call),
 * round 0 .. 2^24 - 1.  The tag differs from the samplers' 0x51 and the nested sampler's 0x4E.  One call per (system,
 * stream, round) gives the words w0 .. w3 and from them two uniforms of 53 bits,
 *     u0 = ((w0 * 2^21 + (w1 & 0x1FFFFF)) + 0.5) / 2^53,      u1 the same from w2, w3,
 * in float64: the integer is exact, the half is one rounded addition, the division a power of two.  The one integer whose
 * sum rounds to 2^53 is held at u = 1 - 2^-53, so 0 < u < 1 always.  The counter arithmetic is integer: host entry and
 * kernel see the same u0, u1 bit for bit.  A system's draws depend on (seed, j, stream, round) and, for a linked column,
 * on its parent's value only: they are the same bits alone, in any batch, at any first, through index, in any order of the
 * other columns and on a repeated call.
 *
 * Draw records.  A column is an iso_draw_record: kind, parent (a column of the same call, or -1), stream, lo, hi and ten
 * doubles p0 .. p9 packed on the host.  Every threshold a branch compares u with is computed on the host and carried in the
 * record (piece masses, component weights, Phi at the bounds), so host entry and kernel take the same branch.  With
 * Phi(z) = erfc(-z / sqrt 2) / 2, ndtri its inverse (Wichura's AS 241 PPND16, csrc/common/ndtri.h) and the result v:
 *   FLAT        v = lo + u0 * (hi - lo)
 *   FLATLOG     v = log10(u0 * p1 + p0)                         p0 = 10^lo (0 for lo = -inf), p1 = 10^hi - 10^lo
 *   POWERLAW    the inverse of x^alpha on [lo, hi] ("plaw" below) with p0 = a1 = alpha + 1, p1 = E, p2 = mode, base lo:
 *               mode 0: v = base * exp(log1p(u0 * E) / a1)      E = expm1(a1 * ln(hi / lo)); no cancellation near a1 = 0
 *               mode 1: v = base * exp(u0 * E)                  a1 == 0; E = ln(hi / lo)
 *               mode 2: v = hi * exp(log(u0) / a1)              lo == 0 (a1 > 0)
 *   GAUSS, TRUNCGAUSS   z = ndtri(p2 + u0 * p3), negated if p4 != 0; v = p0 + p1 * z
 *               p0 = mean, p1 = sigma.  With the standardised bounds a, b, flipped to (-b, -a) when a > 0 (p4 = 1) so that
 *               the mass is taken in the lower tail: p2 = Phi(a), p3 = Phi(b) - Phi(a).  Unbounded: p2 = 0, p3 = 1, p4 = 0.
 *               A window without mass (p3 not above 0) is refused.
 *   LOGNORMAL   v = exp(p0 + p1 * ndtri(u0))                    p0 = mu, p1 = sigma
 *   CHABRIER    u0 < p0: the lognormal piece on its window, z = ndtri(p3 + (u0 / p0) * p4), negated if p5 != 0,
 *               v = exp(p1 + p2 * z); otherwise the power-law piece on its window, plaw with u = (u0 - p0) / (1 - p0),
 *               a1 = p6, E = p7, base p8, mode p9 (0 or 1).  p0 = the lower piece's share of the mass on the bounds, the
 *               masses in closed form.  One uniform is enough.
 *   FEH         the component k is the first with u0 < c_k, c_0 = p1, c_1 = p2, the last one otherwise; then GAUSS's
 *               inverse from u1 with Phi(a) = p[3 + 2k], the mass p[4 + 2k], flipped if bit k of p9 is set, and (mean, sigma)
 *               of the local disk (p0 != 0): (0.016, 0.15), (-0.15, 0.22) and the halo (-1.5, 0.4); otherwise (-0.3, 0.3)
 *               and the halo, with c_1 = 1.  c_k: the cumulated mixture weight times mass inside the bounds, normalised.
 *   LINGAUSS    mu = p0 + p4 * (x_parent - p5); a = (lo - mu) * p3, b = (hi - mu) * p3, flipped when a > 0;
 *               z = ndtri(Phi(a) + u0 * (Phi(b) - Phi(a))), unflipped; v = mu + p1 * z.  p1 = sigma, p3 = 1 / sigma: the
 *               record of include/isochrones_amd_relation.h, Phi computed where the sample is.  Where the window's mass
 *               Phi(b) - Phi(a) underflows to 0 (a mean some 38 sigma outside the bounds; it cannot be refused when the record is
 *               packed) v is the bound next to the mean: lo when flipped, hi otherwise; NaN where the mass is NaN.
 *   TABLE       a piecewise-constant density on K = p1 bins, 1 <= K <= ISO_DRAW_MAX_BINS.  At tables[p0]: the K + 1 edges
 *               e, then per parent bin (one without a parent) the K + 1 cumulative masses cum, cum_0 = 0, cum_K = 1.  The bin
 *               k is the first with u0 < cum_{k+1}; v = e_k + (u0 - cum_k) / (cum_{k+1} - cum_k) * (e_{k+1} - e_k).  With a
 *               parent (p2 = its number of bins, 1 .. ISO_DRAW_MAX_BINS, its edges at tables[p3]) the parent's value is
 *               bracketed on the parent's edges (e_k <= x < e_{k+1}, clamped to the first and last bin) and that bin's
 *               masses are used.
 *   CONSTANT    v = p0
 * v is then held to [lo, hi] (a NaN stays NaN).  Links may chain; order lists the columns so that a parent comes before its
 * child (NULL: 0 .. C - 1), and an order in which a child precedes its parent, as every order of a cycle does, is refused.
 *
 * The device kernel.  k_draw_systems: one lane per system, 256 lanes per workgroup, grid-stride over N.  The C values of a
 * system stay in the lane's registers; the records travel in the kernel arguments, and a column's kind is uniform across
 * the launch.  The source writes no fused multiply-add and is compiled with -ffp-contract=off; there is no atomic.  Kernel
 * and host entry compile the same lines and differ by their exp, log, log1p, log10, erfc and sqrt: they agree to rounding,
 * and in every discrete choice exactly.
 *
 * The library allocates nothing and works on pointers the caller owns.  iso_draw_systems launches on the given stream and
 * does not synchronise.  Return codes: 0 ok, ISO_DRAW_ERR_INVALID for a bad argument or a refused shape
 * (iso_draw_last_error() says which: it is refused, not answered), ISO_DRAW_ERR_HIP for a failed runtime call.
 */
#ifndef ISOCHRONES_AMD_DRAW_H
#define ISOCHRONES_AMD_DRAW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_DRAW_ERR_INVALID (-1)
#define ISO_DRAW_ERR_HIP (-2)

#define ISO_DRAW_MAX_COLS 8
#define ISO_DRAW_MAX_BINS 64
#define ISO_DRAW_NPAR 10
#define ISO_DRAW_PHILOX_TAG 0xD7
/* the grid's cap: workgroups of 256 lanes; a call of more than 256 * ISO_DRAW_MAX_BLOCKS systems strides */
#define ISO_DRAW_MAX_BLOCKS 4096

/* kinds: 1 .. 8 are the ISO_HIER_* values, 9 is ISO_RELATION_LINGAUSS */
#define ISO_DRAW_FLAT 1
#define ISO_DRAW_FLATLOG 2
#define ISO_DRAW_POWERLAW 3
#define ISO_DRAW_GAUSS 4
#define ISO_DRAW_LOGNORMAL 5
#define ISO_DRAW_CHABRIER 6
#define ISO_DRAW_FEH 7
#define ISO_DRAW_TRUNCGAUSS 8
#define ISO_DRAW_LINGAUSS 9
#define ISO_DRAW_TABLE 10
#define ISO_DRAW_CONSTANT 11

typedef struct iso_draw_record {
    int32_t kind;
    int32_t parent; /* LINGAUSS, TABLE: the column of the call it follows, or -1 */
    int32_t stream; /* the column's number in the Philox counter, 0 .. 255 */
    int32_t reserved;
    double lo, hi;
    double p[ISO_DRAW_NPAR];
} iso_draw_record;

const char* iso_draw_version(void);
const char* iso_draw_last_error(void);

/* records ([C]) and order ([C], or NULL) are host arrays; tables ([n_tables] doubles, NULL when no record is a TABLE),
 * index ([N] int64, or NULL) and x ([C][N]) are device pointers. */
int iso_draw_systems(const iso_draw_record* records, int32_t C, const int32_t* order, const double* tables,
                     int64_t n_tables, uint64_t seed, int32_t round, int64_t first, const int64_t* index, int64_t N,
                     double* x, void* stream);

/* the same on host pointers, in plain C++ with ascending loops (no device is touched; stream is ignored) */
int iso_draw_systems_host(const iso_draw_record* records, int32_t C, const int32_t* order, const double* tables,
                          int64_t n_tables, uint64_t seed, int32_t round, int64_t first, const int64_t* index, int64_t N,
                          double* x, void* stream);

/* host only: u[2 * i], u[2 * i + 1] = the uniforms u0, u1 of system j[i], i < n.  `column` is the stream number that enters the
 * counter, a record's `stream` (0 .. 255), not a column's place in a call. */
int iso_draw_uniforms_host(uint64_t seed, int32_t round, const int64_t* j, int64_t n, int32_t column, double* u);

#ifdef __cplusplus
}
#endif

#endif
