"""The definition of include/isochrones_amd_derived.h in numpy, operation by operation (every product and every sum is
one float64 numpy operation, in the header's order), and the fixtures the host-ABI and the GPU tests share."""
import functools

import numpy as np

TOL = 1e-12          # |a - b| <= TOL * (1 + |b|): see tests/test_derived_twin_cpu.py for the reasoning
ROW_MAJOR, PARAM_MAJOR = 0, 1

#: (S, W, T) of the shared fixtures; the GPU test adds rows of 130 and 64 * 3 + 1 (a wave boundary inside a row)
SHAPES = ((1, 2, 1), (3, 10, 7), (5, 26, 4))
GPU_SHAPES = SHAPES + ((1, 130, 3), (1, 64 * 3 + 1, 2))
QS = (1, 3, 8)
CS = (1, 2, 3)


def bracket(ax, x):
    """i = the largest index with ax[i] <= x, at most n - 2 (0 for a NaN); t = (x - ax[i]) / (ax[i + 1] - ax[i])."""
    ax = np.asarray(ax, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        i = np.searchsorted(ax, np.where(np.isnan(x), ax[0], x), side="right") - 1
    i = np.clip(i, 0, ax.size - 2)
    with np.errstate(invalid="ignore"):
        t = (x - ax[i]) / (ax[i + 1] - ax[i])
    return i, t


def interp(cols, axes, x0, x1, xk):
    """cols [n0, n1, nk, Q], three float64 arrays of N coordinates -> [N, Q]."""
    cols = np.asarray(cols, dtype=np.float64)
    xs = [np.asarray(x, dtype=np.float64) for x in (x0, x1, xk)]
    with np.errstate(invalid="ignore"):
        ok = np.ones(xs[0].shape, dtype=bool)
        for ax, x in zip(axes, xs):
            ok &= ~np.isnan(x) & ~(x < ax[0]) & ~(x > ax[-1])
    (i0, t0), (i1, t1), (ik, tk) = (bracket(ax, x) for ax, x in zip(axes, xs))
    f = ((1 - t0, t0), (1 - t1, t1), (1 - tk, tk))
    v = np.zeros(xs[0].shape + (cols.shape[3],))
    with np.errstate(invalid="ignore"):
        for b0 in (0, 1):
            for b1 in (0, 1):
                for bk in (0, 1):
                    w = (f[0][b0] * f[1][b1]) * f[2][bk]
                    v = v + cols[i0 + b0, i1 + b1, ik + bk] * w[:, None]
    v[~ok] = np.nan
    return v


def derive(chain, layout, n_ens, W, cols, axes, comps, ens_begin=0, n_ens_out=None):
    """chain [T, D, n_ens * W] (PARAM_MAJOR) or [T, n_ens * W, D] (ROW_MAJOR) -> (out [T, C * Q, R], nan_count [n_out, C * Q])."""
    n_out = n_ens - ens_begin if n_ens_out is None else n_ens_out
    x = chain if layout == PARAM_MAJOR else chain.transpose(0, 2, 1)          # [T, D, rows]
    x = x[:, :, ens_begin * W:(ens_begin + n_out) * W]
    T, R, Q = x.shape[0], n_out * W, cols.shape[3]
    out = np.empty((T, len(comps) * Q, R))
    for c, (p0, p1, pk) in enumerate(comps):
        v = interp(cols, axes, x[:, p0].ravel(), x[:, p1].ravel(), x[:, pk].ravel())       # [T * R, Q]
        out[:, c * Q:(c + 1) * Q] = v.reshape(T, R, Q).transpose(0, 2, 1)
    nan_count = np.isnan(out).reshape(T, -1, n_out, W).sum(axis=(0, 3)).T.astype(np.int32)
    return out, nan_count


#: the bound on |twin - interp_ld| in units of 2^-52 * cmax (see interp_ld)
LD_BOUND = 40


def interp_ld(cols, axes, x0, x1, xk):
    """The formula of :func:`interp` in ``np.longdouble`` -> (value as longdouble [N, Q], cmax [N, Q]).

    The bracket indices are the float64 search's; ``t``, ``1 - t``, the weights, the products and the sums are long
    double.  ``cmax`` is the largest |corner| among the cell's eight corners, per column.  NaN (both) where the twin
    gives NaN.

    ``LD_BOUND``, in units of 2^-52 * cmax, bounds the distance of a float64 evaluation in the header's order from this
    one.  Each of ``t`` and ``1 - t`` carries at most 4 roundings of absolute size <= 2^-52.  A weight is a product of
    three such factors in [0, 1] plus two roundings.  Over the eight corners the absolute weight errors sum to at most
    3 * 4 * 2 + 2 = 26 units.  The eight products add 1 unit and the eight sums at most 8.  That totals 35 units,
    rounded up to 40.  The twin itself was measured at 2.43."""
    L = np.longdouble
    cols = np.asarray(cols, dtype=np.float64)
    xs = [np.asarray(x, dtype=np.float64) for x in (x0, x1, xk)]
    with np.errstate(invalid="ignore"):
        ok = np.ones(xs[0].shape, dtype=bool)
        for ax, x in zip(axes, xs):
            ok &= ~np.isnan(x) & ~(x < ax[0]) & ~(x > ax[-1])
    idx, f = [], []
    for ax, x in zip(axes, xs):
        i, _ = bracket(ax, x)
        lo, hi = ax[i].astype(L), ax[i + 1].astype(L)
        t = (x.astype(L) - lo) / (hi - lo)
        idx.append(i)
        f.append((1 - t, t))
    v = np.zeros(xs[0].shape + (cols.shape[3],), dtype=L)
    cmax = np.zeros(xs[0].shape + (cols.shape[3],))
    with np.errstate(invalid="ignore"):
        for b0 in (0, 1):
            for b1 in (0, 1):
                for bk in (0, 1):
                    corner = cols[idx[0] + b0, idx[1] + b1, idx[2] + bk]
                    w = (f[0][b0] * f[1][b1]) * f[2][bk]
                    v = v + corner.astype(L) * w[:, None]
                    cmax = np.maximum(cmax, np.abs(corner))
    v[~ok] = np.nan
    cmax[np.isnan(v)] = np.nan
    return v, cmax


def derive_ld(chain, layout, n_ens, W, cols, axes, comps):
    """:func:`derive` through :func:`interp_ld` -> (out as longdouble [T, C * Q, R], cmax [T, C * Q, R])."""
    x = chain if layout == PARAM_MAJOR else chain.transpose(0, 2, 1)
    T, R, Q = x.shape[0], n_ens * W, cols.shape[3]
    out, cmax = np.empty((T, len(comps) * Q, R), dtype=np.longdouble), np.empty((T, len(comps) * Q, R))
    for c, (p0, p1, pk) in enumerate(comps):
        v, m = interp_ld(cols, axes, x[:, p0].ravel(), x[:, p1].ravel(), x[:, pk].ravel())
        out[:, c * Q:(c + 1) * Q] = v.reshape(T, R, Q).transpose(0, 2, 1)
        cmax[:, c * Q:(c + 1) * Q] = m.reshape(T, R, Q).transpose(0, 2, 1)
    return out, cmax


def ld_ratio(a, ref, cmax):
    """The largest |a - ref| / (2^-52 * cmax) over the finite entries of ``ref``; NaN positions must already agree."""
    fin = ~np.isnan(ref)
    if not fin.any():
        return 0.0
    err = np.abs(np.asarray(a)[fin].astype(np.longdouble) - ref[fin])
    return float(np.max(err / (np.longdouble(2.0) ** -52 * cmax[fin].astype(np.longdouble))))


def same_bits(a, b):
    """Same shape, NaN at the same positions, every other value the same 64 bits (so -0.0 is not 0.0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = ~np.isnan(b)
    return bool(np.array_equal(a.view(np.int64)[fin], b.view(np.int64)[fin]))


def close(a, b):
    """NaN positions identical, |a - b| <= TOL * (1 + |b|) elsewhere."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = ~np.isnan(b)
    return bool(np.all(np.abs(a[fin] - b[fin]) <= TOL * (1 + np.abs(b[fin]))))


# ---- fixtures ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid(kind):
    """A small ``ia.grids``-shaped synthetic table: (grid [n0, n1, nk, ncol], axes, columns).  Ragged, NaN-padded."""
    from isochrones_amd import grids
    if kind == "track":
        g, ax, cols = grids.synthetic_track_grid(np.array([-1.0, -0.5, 0.0, 0.25, 0.5]),
                                                 grids.mist_masses()[40:100:6], np.arange(200.0, 460.0, 4.0))
    else:
        g, ax, cols = grids.synthetic_iso_grid(np.array([8.5, 9.0, 9.3, 9.6, 9.9, 10.1]), np.array([-1.0, -0.5, 0.0, 0.5]),
                                               np.arange(200.0, 460.0, 4.0))
    g.setflags(write=False)
    return g, tuple(np.ascontiguousarray(a, dtype=np.float64) for a in ax), tuple(cols)


def packed(kind, Q):
    """The first Q of (radius, Teff, logg, mass, Mbol, logL, density, feh) packed [n0, n1, nk, Q], and the axes."""
    g, axes, cols = grid(kind)
    want = ("radius", "Teff", "logg", "mass", "Mbol", "logL", "density", "feh")[:Q]
    return np.ascontiguousarray(g[..., [cols.index(c) for c in want]]), axes


def comps_for(C):
    """C components over a chain of 6 parameters; the first two share (p0, p1), the third reads other ones."""
    return [(2, 3, 0), (2, 3, 1), (5, 3, 4)][:C]


def _draw(rng, ax, n):
    """n coordinates over one axis: uniform inside, one in 40 each on a node, above the table, below it, and NaN."""
    v = rng.uniform(ax[0], ax[-1], n)
    kind_of = rng.integers(0, 40, n)
    v = np.where(kind_of == 0, ax[rng.integers(0, ax.size, n)], v)      # on a node (the last one included)
    v = np.where(kind_of == 1, ax[-1] + 0.5, v)
    v = np.where(kind_of == 2, ax[0] - 0.5, v)
    return np.where(kind_of == 3, np.nan, v)


@functools.lru_cache(maxsize=None)
def chain(kind, S, W, T, seed=0):
    """Parameter-major storage [T, 6, S * W] whose parameters are drawn over the axes a component maps them to, with a few
    samples off the table, on nodes and NaN.  Read-only."""
    _, axes = packed(kind, 1)
    rng = np.random.default_rng(seed + 1000 * S + 10 * W + T)
    n = T * S * W
    ax_of = {2: 0, 5: 0, 3: 1, 0: 2, 1: 2, 4: 2}                 # parameter -> axis, as comps_for uses them
    x = np.empty((T, 6, S * W))
    for p, a in ax_of.items():
        x[:, p] = _draw(rng, axes[a], n).reshape(T, S * W)
    x.setflags(write=False)
    return x


#: (S, W, T), the smallest shapes that reach each branch of the kernel's work split (256 rows a chunk, 2 048 workgroups):
#: two chunks with 53 rows in the last and ensemble 2 across row 256; one lane in the second chunk; none there; 2 100
#: items; 2 060 items of two chunks each
EDGE_SHAPES = ((3, 103, 9), (1, 257, 3), (1, 256, 3), (1, 2, 2100), (2, 130, 1030))

#: which of (p0, p1) a component shares with the one before it, over chain7: reused twice; new then reused at c = 2; new
#: twice; only p1 changes; only p0 changes; the same triple three times
COMP_PATTERNS = ([(2, 3, 0), (2, 3, 1), (2, 3, 4)],
                 [(2, 3, 0), (5, 3, 4), (5, 3, 1)],
                 [(2, 3, 0), (5, 3, 4), (2, 3, 1)],
                 [(2, 3, 0), (2, 6, 0)],
                 [(2, 3, 0), (5, 3, 0)],
                 [(2, 3, 0), (2, 3, 0), (2, 3, 0)])


@functools.lru_cache(maxsize=None)
def chain7(kind, S, W, T, seed=0):
    """:func:`chain` with a seventh parameter drawn over axis 1 in the same mix, so that a component can change p1 alone.
    Parameter-major [T, 7, S * W], read-only."""
    _, axes = packed(kind, 1)
    x = np.empty((T, 7, S * W))
    x[:, :6] = chain(kind, S, W, T, seed)
    rng = np.random.default_rng(7 + seed + 1000 * S + 10 * W + T)
    x[:, 6] = _draw(rng, axes[1], T * S * W).reshape(T, S * W)
    x.setflags(write=False)
    return x


def rule_table():
    """A hand-built 3 x 3 x 4 table with 2 columns, a non-uniform last axis and one NaN node."""
    axes = (np.array([0.0, 1.0, 2.0]), np.array([10.0, 20.0, 40.0]), np.array([1.0, 2.0, 4.0, 8.0]))
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in (3, 3, 4)], indexing="ij")
    cols = np.stack([100.0 * i + 10.0 * j + k, 1.0 + i * j + 0.5 * k * k], axis=-1)
    cols[2, 2, 3] = np.nan
    return cols, axes


def chain_wide(kind, S, W, T, ndim, comp, seed=0):
    """Parameter-major [T, ndim, S * W], zero but for the three parameters of the one component ``comp``, which are drawn
    over their axes in the mix of :func:`chain`."""
    _, axes = packed(kind, 1)
    rng = np.random.default_rng(11 + seed + ndim)
    x = np.zeros((T, ndim, S * W))
    for p, ax in zip(comp, axes):
        x[:, p] = _draw(rng, ax, T * S * W).reshape(T, S * W)
    return x


def nan_column_case(Q=4, col=2, S=3, W=40, T=4, seed=0):
    """packed("track", Q) with column ``col`` set to NaN at the eight nodes of one interior cell whose surroundings are
    finite, and a chain [T, 3, S * W] (comps [(0, 1, 2)]) drawn over that cell and up to two cells either side of it
    on every axis: inside the cell and in the cells that share a node with it column ``col`` is NaN, two cells away it is
    not; the other columns are finite everywhere.  -> (clean cols, dirty cols, axes, chain)."""
    clean, axes = packed("track", Q)
    fin = np.isfinite(clean).all(axis=3)
    cell = next((i, j, k) for i in range(1, fin.shape[0] - 2) for j in range(1, fin.shape[1] - 2)
                for k in range(1, fin.shape[2] - 2) if fin[max(i - 2, 0):i + 4, max(j - 2, 0):j + 4, max(k - 2, 0):k + 4].all())
    dirty = clean.copy()
    dirty[cell[0]:cell[0] + 2, cell[1]:cell[1] + 2, cell[2]:cell[2] + 2, col] = np.nan
    rng = np.random.default_rng(seed)
    x = np.empty((T, 3, S * W))
    for a, (ax, i) in enumerate(zip(axes, cell)):
        x[:, a] = rng.uniform(ax[max(i - 2, 0)], ax[min(i + 3, ax.size - 1)], (T, S * W))
    x[0, :, 0] = [ax[i] + 0.5 * (ax[i + 1] - ax[i]) for ax, i in zip(axes, cell)]          # one sample surely inside
    return clean, dirty, axes, x


_NAN2 = (np.nan, np.nan)
#: ((x0, x1, xk), the two exact values) on rule_table
RULES = (
    # inside, the last axis non-uniform: xk = 3 lies halfway between the nodes 2 and 4
    ((0.5, 15.0, 3.0), (56.5, 2.5)),
    ((0.25, 35.0, 7.0), (25.0 + 17.5 + 2.75, 1.0 + 0.25 * 1.75 + 0.5 * (0.25 * 4 + 0.75 * 9))),
    # on a node: the cell above it, weight 0 on every other corner
    ((1.0, 20.0, 2.0), (111.0, 2.5)),
    ((0.0, 10.0, 1.0), (0.0, 1.0)),
    # on the last node of each axis: the cell below, weight 1
    ((2.0, 15.0, 3.0), (206.5, 1.0 + 1.0 + 1.25)),
    ((0.5, 40.0, 3.0), (71.5, 1.0 + 1.0 + 1.25)),
    ((0.5, 15.0, 8.0), (58.0, 1.25 + 4.5)),
    # off either end of each axis, and a NaN coordinate
    ((-0.1, 15.0, 3.0), _NAN2), ((2.1, 15.0, 3.0), _NAN2), ((0.5, 9.0, 3.0), _NAN2), ((0.5, 41.0, 3.0), _NAN2),
    ((0.5, 15.0, 0.5), _NAN2), ((0.5, 15.0, 8.5), _NAN2),
    ((np.nan, 15.0, 3.0), _NAN2), ((0.5, np.nan, 3.0), _NAN2), ((0.5, 15.0, np.nan), _NAN2),
    # the NaN node (2, 2, 3): a corner of the cell above (1, 1, 2) with weight zero, and the last node itself
    ((1.0, 20.0, 4.0), _NAN2),
    ((2.0, 40.0, 8.0), _NAN2),
    ((1.5, 30.0, 6.0), _NAN2),                                   # inside the cell that has it
    ((1.0, 20.0, 3.0), (111.5, 3.25)),                           # the cell below it along the last axis
    ((0.5, 15.0, 6.0), (50.0 + 5.0 + 2.5, 1.25 + 0.5 * 6.5)),    # a cell away from it
)


def search_table(axis, n):
    """A table with n nodes on ``axis`` and 2 on the others, Q = 1, whose value is the node index along ``axis``; that
    axis is non-uniform (cumulative sums of 1, 2, 3, ...), the others are [0, 1].  -> (cols, axes)."""
    axes = [np.array([0.0, 1.0]) for _ in range(3)]
    axes[axis] = np.cumsum(np.arange(1.0, n + 1.0))
    shape = [2, 2, 2]
    shape[axis] = n
    view = [1, 1, 1]
    view[axis] = n
    cols = np.broadcast_to(np.arange(float(n)).reshape(view), shape)[..., None]
    return np.ascontiguousarray(cols), tuple(axes)


def search_samples(axis, n):
    """Coordinates for search_table(axis, n) -> (x [3, N] on (ax0, ax1, axk), expected [N] with NaN for "outside" and -1
    for "the twin's value").  On ``axis``: every node, every midpoint, just inside and just outside both ends.  The
    other two coordinates are 0.25 and 0.5: their weights are dyadic, so a node's value is its index exactly."""
    ax = search_table(axis, n)[1][axis]
    mid = 0.5 * (ax[:-1] + ax[1:])
    inside = np.array([np.nextafter(ax[0], np.inf), np.nextafter(ax[-1], -np.inf)])
    outside = np.array([np.nextafter(ax[0], -np.inf), np.nextafter(ax[-1], np.inf)])
    xa = np.concatenate([ax, mid, inside, outside])
    want = np.concatenate([np.arange(float(n)), np.full(mid.size + 2, -1.0), [np.nan, np.nan]])
    x = np.empty((3, xa.size))
    x[[a for a in range(3) if a != axis]] = np.array([[0.25], [0.5]])
    x[axis] = xa
    return x, want
