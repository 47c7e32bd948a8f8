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
        ax = axes[a]
        v = rng.uniform(ax[0], ax[-1], n)
        kind_of = rng.integers(0, 40, n)
        v = np.where(kind_of == 0, ax[rng.integers(0, ax.size, n)], v)      # on a node (the last one included)
        v = np.where(kind_of == 1, ax[-1] + 0.5, v)
        v = np.where(kind_of == 2, ax[0] - 0.5, v)
        v = np.where(kind_of == 3, np.nan, v)
        x[:, p] = v.reshape(T, S * W)
    x.setflags(write=False)
    return x


def rule_table():
    """A hand-built 3 x 3 x 4 table with 2 columns, a non-uniform last axis and one NaN node."""
    axes = (np.array([0.0, 1.0, 2.0]), np.array([10.0, 20.0, 40.0]), np.array([1.0, 2.0, 4.0, 8.0]))
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in (3, 3, 4)], indexing="ij")
    cols = np.stack([100.0 * i + 10.0 * j + k, 1.0 + i * j + 0.5 * k * k], axis=-1)
    cols[2, 2, 3] = np.nan
    return cols, axes
