"""TEST INFRASTRUCTURE - a numpy statement of what ``solve_eep`` must return (include/isochrones_amd_solve.h), built on
``oracle.oracle.OracleTable.interp`` (the CPU interpolation pinned to the reference) and sharing no code with the
package's implementation.

For every query g(k) is evaluated at EVERY knot of the last axis by the oracle interpolator; k* is the smallest index
inside the intersection of the four corner columns' [first, last] finite ranges with g(k*) >= target; the result is the
linear inverse between the knots k* - 1 and k*, with the rules of the header for the first knot, holes and NaN.
"""
import numpy as np

from oracle import oracle as orc


def finite_ranges(col):
    """(first, last) finite index along the last axis of col[n0, n1, nk]; (nk, -1) where nothing is finite."""
    n0, n1, nk = col.shape
    first = np.full((n0, n1), nk, dtype=np.int64)
    last = np.full((n0, n1), -1, dtype=np.int64)
    for i in range(n0):
        for j in range(n1):
            k = np.flatnonzero(np.isfinite(col[i, j]))
            if k.size:
                first[i, j], last[i, j] = k[0], k[-1]
    return first, last


def _cell(ax, x):
    """Lower node of the cell the interpolator uses for x (a node takes the cell above it, the last node the cell below)."""
    return np.clip(np.searchsorted(ax, x, side="right") - 1, 0, ax.size - 2)


def knot_values(grid, axes, icol, x0, x1, nthreads=1):
    """g[n, nk]: the oracle interpolator's value of column ``icol`` at (x0, x1, axk[k]) for every knot k."""
    table = orc.OracleTable(grid, axes)
    axk = table.axes[2]
    x0, x1 = np.asarray(x0, dtype=float).ravel(), np.asarray(x1, dtype=float).ravel()
    m, nk = x0.size, axk.size
    return table.interp([np.repeat(x0, nk), np.repeat(x1, nk), np.tile(axk, m)], [icol], nthreads=nthreads).reshape(m, nk)


def cell_ranges(col, axes, x0, x1):
    """(ok, i, j, F, L) per query: inside both axes, the cell the interpolator uses (cell 0 where not ok) and the
    intersection [F, L] of its four corner columns' finite ranges (F > L: empty)."""
    ax0, ax1 = np.asarray(axes[0], dtype=float), np.asarray(axes[1], dtype=float)
    first, last = finite_ranges(np.asarray(col, dtype=float))
    a, b = np.asarray(x0, dtype=float).ravel(), np.asarray(x1, dtype=float).ravel()
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a) & np.isfinite(b) & (a >= ax0[0]) & (a <= ax0[-1]) & (b >= ax1[0]) & (b <= ax1[-1])
    i = _cell(ax0, np.where(ok, a, ax0[0]))
    j = _cell(ax1, np.where(ok, b, ax1[0]))
    F = np.maximum.reduce([first[i, j], first[i, j + 1], first[i + 1, j], first[i + 1, j + 1]])
    L = np.minimum.reduce([last[i, j], last[i, j + 1], last[i + 1, j], last[i + 1, j + 1]])
    return ok, i, j, F, L


def solve(grid, axes, icol, x0, x1, target, chunk=256, nthreads=1):
    """grid[n0, n1, nk, ncol], axes (ax0, ax1, axk), column number -> (e, g_lo, g_hi, k_star) per query: the solution,
    the two knot values it was inverted between (NaN where no segment was inverted) and k* (-1: none)."""
    grid = np.asarray(grid, dtype=float)
    axk = np.ascontiguousarray(axes[2], dtype=float)
    nk = axk.size
    x0, x1, target = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=float), np.broadcast(x0, x1, target).shape)
                                           .ravel()) for v in (x0, x1, target)]
    n = x0.size
    e = np.full(n, np.nan)
    g_lo, g_hi = np.full(n, np.nan), np.full(n, np.nan)
    k_star = np.full(n, -1, dtype=np.int64)
    ks = np.arange(nk)
    for s in range(0, n, chunk):
        a, b, y = x0[s:s + chunk], x1[s:s + chunk], target[s:s + chunk]
        g = knot_values(grid, axes, icol, a, b, nthreads=nthreads)
        ok, _, _, F, L = cell_ranges(grid[..., icol], axes, a, b)
        with np.errstate(invalid="ignore"):
            reach = (g >= y[:, None]) & (ks[None, :] >= F[:, None]) & (ks[None, :] <= L[:, None]) & ok[:, None]
        for r in np.flatnonzero(reach.any(axis=1)):
            k = int(reach[r].argmax())
            k_star[s + r] = k
            if k == F[r]:
                if g[r, k] == y[r]:
                    e[s + r] = axk[k]
                continue
            lo, hi = g[r, k - 1], g[r, k]
            if np.isnan(lo):
                continue
            g_lo[s + r], g_hi[s + r] = lo, hi
            with np.errstate(invalid="ignore"):
                e[s + r] = axk[k - 1] + (y[r] - lo) / (hi - lo) * (axk[k] - axk[k - 1])
    return e, g_lo, g_hi, k_star


def local_slope(axes, g_lo, g_hi, k_star):
    """Slope of g along the last axis on the segment a solution was inverted on (NaN where there was none)."""
    axk = np.asarray(axes[2], dtype=float)
    k = np.maximum(k_star, 1)
    return (g_hi - g_lo) / (axk[k] - axk[k - 1])
