"""A plain-numpy twin of the N-D multilinear interpolation (DFInterpolator, ND = 2, 3, 4), the two O(1) first guesses of the
uniform-axis brackets, and the edge tables the CPU tests, the GPU tests and oracle/make_golden.py share.  No GPU, no library.

The rule (reference isochrones/interp.py:10-35, 116-123, 264-291), per axis a_0 < ... < a_{n-1}:

    i = min(#{a_j <= x} - 1, n - 2),     t = (x - a_i) / (a_{i+1} - a_i)

the 2^ND corners are summed in the reference's order (bit ND-1-d of the corner number offsets axis d, the weight is the
product over d = 0 .. ND-1 of t_d or 1 - t_d, starting from 1.0); a NaN coordinate or one outside [a_0, a_{n-1}] gives NaN; a
NaN corner gives NaN even under weight 0; at x = a_{n-1} the last cell is used with t = 1 (this project's documented
deviation: the reference reads past the table there).

The error bound of a float64 evaluation against the long-double one, per point and column:

    limit = 2 * (5*ND + 2**ND + 1) * 2**-53 * sum_j |v_j|          (j over the 2^ND corner values of that column)

- every t carries at most 3 roundings (two differences, one quotient; the operands are exact) and 1 - t at most 4;
- a weight is a product of ND factors that are at most 1, so its absolute error is at most 5*ND eps (4 from a factor, 1
  from its multiplication);
- the 2^ND products and sums add at most (2^ND + 1) eps relative to sum |w v|, which is at most sum |v|;
- the factor 2 covers second-order terms and fused multiply-adds, which only remove roundings.
(A |t| slightly above 1 - x one ulp below a node on a cell whose spacing rounds - leaves the factors at most 1 + 2 eps, which
the second-order allowance covers.)
"""
import functools
import os
import re
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53


def _lds_budget():
    """MAX_LDS_AXIS_DOUBLES of the library's sources: non-uniform axes are staged in LDS while they fit this many doubles."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isochrones_amd", "csrc", "iso_internal.h")
    with open(path) as f:
        return int(re.search(r"\bMAX_LDS_AXIS_DOUBLES\s*=\s*(\d+)", f.read()).group(1))


MAX_LDS_AXIS_DOUBLES = _lds_budget()


def limit_factor(nd):
    return 2.0 * (5 * nd + 2 ** nd + 1) * EPS


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------
def bracket_index(axis, x):
    """min(#{a_j <= x} - 1, n - 2) per element of x (meaningless, but in range, for NaN and out-of-axis x)."""
    axis = np.asarray(axis, dtype=np.float64)
    cnt = np.searchsorted(axis, np.asarray(x, dtype=np.float64), side="right")
    return np.clip(cnt - 1, 0, axis.size - 2)


def _evaluate(grid, axes, xs, icols, dtype, shift_axis=None, shift=0):
    grid = np.asarray(grid)
    nd = len(axes)
    assert nd in (2, 3, 4) and grid.ndim == nd + 1
    axes = [np.asarray(a, dtype=np.float64) for a in axes]
    xs = [np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64) for x in xs]
    icols = np.asarray(icols, dtype=np.int64)
    n = xs[0].size
    bad = np.zeros(n, dtype=bool)
    for a, x in zip(axes, xs):
        bad |= np.isnan(x)
        with np.errstate(invalid="ignore"):
            bad |= (x < a[0]) | (x > a[-1])
    applicable = ~bad
    idx, ts = [], []
    for d, (a, x) in enumerate(zip(axes, xs)):
        i = bracket_index(a, np.where(bad, a[0], x))
        if d == shift_axis:
            i = i + shift
            applicable &= (i >= 0) & (i <= a.size - 2)
            i = np.clip(i, 0, a.size - 2)
        al = a.astype(dtype)
        xl = np.where(bad, a[0], x).astype(dtype)
        lo, hi = al[i], al[i + 1]
        ts.append((xl - lo) / (hi - lo))
        idx.append(i)
    vals = np.zeros((n, icols.size), dtype=dtype)
    sumabs = np.zeros((n, icols.size), dtype=dtype)
    with np.errstate(invalid="ignore"):
        for j in range(1 << nd):
            w = np.ones(n, dtype=dtype)
            where = []
            for d in range(nd):
                bit = (j >> (nd - 1 - d)) & 1
                w = w * (ts[d] if bit else (1 - ts[d]))
                where.append(idx[d] + bit)
            corner = grid[tuple(where)][:, icols].astype(dtype)
            vals = vals + corner * w[:, None]
            sumabs = sumabs + np.abs(corner)
    vals[bad] = np.nan
    sumabs[bad] = np.nan
    return vals, sumabs, applicable


def interp(grid, axes, xs, icols, dtype=np.longdouble):
    """(values [n, k], sum_j |v_j| [n, k]) of the rule, evaluated in `dtype`."""
    vals, sumabs, _ = _evaluate(grid, axes, xs, icols, dtype)
    return vals, sumabs


def neighbour(grid, axes, xs, icols, axis, shift, dtype=np.float64):
    """What a bracket whose cell index on `axis` is off by `shift` (-1 or +1) would give, with t recomputed from that cell.
    Returns (values, decisive [n]): a probe is decisive when the shifted cell exists and the NaN-ness of its result differs
    from the rule's in some column - the only way such an error shows, the interpolant being continuous."""
    assert shift in (-1, 1)
    want, _, _ = _evaluate(grid, axes, xs, icols, dtype)
    got, _, applicable = _evaluate(grid, axes, xs, icols, dtype, shift_axis=axis, shift=shift)
    decisive = applicable & np.any(np.isnan(got) != np.isnan(want), axis=1)
    return got, decisive


def check(got, grid, axes, xs, icols, what=""):
    """NaN pattern exact, values within the bound of the long-double twin.  Returns the worst error / limit."""
    want, sumabs = interp(grid, axes, xs, icols)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN pattern differs at rows %s" % (what, np.unique(np.nonzero(nan_g != nan_w)[0])[:10])
    fin = ~nan_w
    if not fin.any():
        return 0.0
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    lim = limit_factor(len(axes)) * sumabs[fin]
    zero = lim == 0                                      # a cell whose corners are all zero: the result must be exact
    assert np.all(err[zero] == 0), "%s: a value differs where every corner is zero" % what
    worst = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    assert worst <= 1.0, "%s: error / limit = %g" % (what, worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# uniform axes: the host's test and the kernels' first guesses
# ---------------------------------------------------------------------------------------------------------------------------
def _round_once(fr):
    """The float64 nearest (ties to even) to a Fraction: what a fused multiply-add returns."""
    return fr.numerator / fr.denominator        # int / int is correctly rounded in CPython


def is_uniform(axis):
    """axis_uniform() of the library: every node equals both i*step + a0 (two roundings) and fma(i, step, a0) (one)."""
    a = np.asarray(axis, dtype=np.float64)
    if a.size < 2 or a.size >= (1 << 24):
        return False
    a0, step = float(a[0]), float(a[1] - a[0])
    if not step > 0:
        return False
    i = np.arange(a.size, dtype=np.float64)
    if not np.array_equal(i * step + a0, a):
        return False
    fa0, fstep = Fraction(a0), Fraction(step)
    return all(_round_once(Fraction(j) * fstep + fa0) == float(a[j]) for j in range(a.size))


def first_guess_generic(x, a0, step, n):
    """bracket() of kernels/dev_common.h before its fix-up: int((x - a0) / step), clamped to [0, n - 2]."""
    x = np.asarray(x, dtype=np.float64)
    return np.clip(((x - a0) / step).astype(np.int64), 0, n - 2)


def first_guess_fused(x, a0, step, n):
    """eep_bracket() of fast/brackets.h before its fix-up: int((x - a0) * (1 / step)), clamped to [0, n - 2]."""
    x = np.asarray(x, dtype=np.float64)
    inv = 1.0 / np.float64(step)
    return np.clip(((x - a0) * inv).astype(np.int64), 0, n - 2)


def fixup_needed(axis, x, guess):
    """+1 where the guess is one too low (the kernel's ++k), -1 where it is one too high (--k), 0 where it is right."""
    axis = np.asarray(axis, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    g = guess(x, float(axis[0]), float(axis[1] - axis[0]), axis.size)
    d = bracket_index(axis, x) - g
    assert np.all(np.abs(d) <= 1), "a first guess is off by more than one cell"
    return d


def node_probes(axis):
    """Every node and its two floating-point neighbours (so: one ulp outside either end), +-0.0 and NaN."""
    a = np.asarray(axis, dtype=np.float64)
    return np.concatenate([a, np.nextafter(a, -np.inf), np.nextafter(a, np.inf), [0.0, -0.0, np.nan]])


# ---------------------------------------------------------------------------------------------------------------------------
# the edge tables
# ---------------------------------------------------------------------------------------------------------------------------
THIRD = 1.0 / 3.0
UNIFORM = {"U2": ((0.7, 120), (0.1, 150)),
           "U3": ((0.3, 64), (0.7, 40), (0.1, 50)),
           "U4": ((THIRD, 20), (0.7, 22), (0.1, 24), (0.3, 20))}
UNSTAGED = {"G2_global": (6145, 3), "G2_exact": (6141, 3), "G3_global": (6000, 2, 150), "G3_exact": (6140, 2, 2)}
MINIMUM = {"M2": (2, 2), "M3": (2, 2, 2), "M4": (2, 2, 2, 2)}
NCOL = 6


class EdgeTable:
    def __init__(self, name, grid, axes, probes, nan_nodes=None):
        self.name, self.grid, self.axes, self.probes = name, grid, axes, probes
        self.nd = len(axes)
        self.ncol = grid.shape[-1]
        self.nan_nodes = nan_nodes or {}

    @property
    def columns(self):
        return ["c%d" % j for j in range(self.ncol)]

    def xs(self, rows=None):
        p = self.probes if rows is None else self.probes[rows]
        return [np.ascontiguousarray(p[:, d]) for d in range(self.nd)]


def _smooth_grid(rng, axes, ncol):
    """Values of order one with both signs, different in every column, nowhere exactly zero on purpose."""
    shape = tuple(a.size for a in axes)
    g = rng.standard_normal(shape + (ncol,))
    return g + np.sign(g) * 0.25


def _off_probes(axis):
    """{node j: set of (guess number, direction)} - where a first guess (0 generic, 1 fused) is one too low (+1) or too high
    (-1) at a_j or at one of its two floating-point neighbours."""
    a = np.asarray(axis)
    out = {}
    for g, guess in enumerate((first_guess_generic, first_guess_fused)):
        for x in (a, np.nextafter(a, -np.inf), np.nextafter(a, np.inf)):
            d = fixup_needed(a, np.clip(x, a[0], a[-1]), guess)
            for j in np.flatnonzero(d):
                out.setdefault(int(j), []).append((g, int(d[j])))
    return out


def _choose_nan_nodes(axes, target=5):
    """{axis: nodes to blank} so that fix-up probes are decisive.  A probe at (or one ulp around) node j lies in cell j - 1 or
    j and its wrong neighbour is the other of the two; node j + 1 belongs to cell j only, so a NaN there separates them.  Nodes
    are taken greedily, the one that serves the most of the four (guess, direction) combinations still short of `target`
    probes first; chosen nodes of one axis stay three apart, so that most of the table remains finite."""
    have = {(g, s): 0 for g in (0, 1) for s in (1, -1)}
    cand = []
    for d, a in enumerate(axes):
        for j, combos in _off_probes(a).items():
            if 1 <= j and j + 1 <= a.size - 2:
                cand.append((d, j + 1, combos))
    chosen = {d: [] for d in range(len(axes))}
    while min(have.values()) < target:
        best, gain = None, 0
        for d, m, combos in cand:
            if any(abs(m - c) < 3 for c in chosen[d]):
                continue
            g = len({c for c in combos if have[c] < target})
            if g > gain:
                best, gain = (d, m, combos), g
        if best is None:
            break
        chosen[best[0]].append(best[1])
        for c in best[2]:
            have[c] += 1
    return {d: sorted(v) for d, v in chosen.items()}


def _probe_rows(rng, axes, specials, n_draws):
    """Rows: for every axis d and every special value of it, that value with the other coordinates drawn inside their axes;
    then uniform draws, 2 % beyond the table on every side."""
    rows = []
    for d, sp in enumerate(specials):
        block = np.column_stack([rng.uniform(a[0], a[-1], sp.size) for a in axes])
        block[:, d] = sp
        rows.append(block)
    lo = np.array([a[0] for a in axes])
    hi = np.array([a[-1] for a in axes])
    rows.append(rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), size=(n_draws, len(axes))))
    p = np.vstack(rows)
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])])       # mixed, so that a short batch sees every kind


def _uniform_table(name):
    spec = UNIFORM[name]
    rng = np.random.default_rng([20261020, len(spec)])
    axes = [np.arange(n, dtype=np.float64) * step for step, n in spec]
    for a in axes:
        assert is_uniform(a)
    grid = _smooth_grid(rng, axes, NCOL)
    nan_nodes = _choose_nan_nodes(axes)
    for d, a in enumerate(axes):                         # NaN at single nodes of axis d, in column d (ND <= 4 < NCOL)
        if not nan_nodes[d]:
            continue
        sl = [slice(None)] * len(axes)
        sl[d] = nan_nodes[d]
        grid[tuple(sl) + (d,)] = np.nan
    # a ragged tail along the last axis in the last two columns: rows of the first axis end at different nodes
    last = axes[-1].size
    for i0 in range(0, axes[0].size, 3):
        grid[i0, ..., last - 2 - (i0 % 5):, NCOL - 2:] = np.nan
    probes = _probe_rows(rng, axes, [node_probes(a) for a in axes], 400)
    return EdgeTable(name, grid, axes, probes, nan_nodes)


def _clustered_axis(rng, n):
    """A non-uniform axis with nodes one ulp apart in places."""
    a = np.sort(rng.uniform(1.0, 9.0, n))
    a = np.unique(a)
    assert a.size == n
    for j in rng.choice(np.arange(2, n - 8), 40, replace=False):
        a[j + 1] = np.nextafter(a[j], np.inf)
        a[j + 2] = np.nextafter(a[j + 1], np.inf)
    a = np.sort(a)
    assert np.all(np.diff(a) > 0) and not is_uniform(a)
    return a


def _unstaged_table(name):
    shape = UNSTAGED[name]
    rng = np.random.default_rng([20261021, sum(shape)])
    axes = [_clustered_axis(rng, shape[0])]
    for n in shape[1:]:
        if n == 2:                                         # (b - a) + a != b: two nodes the library does not call uniform
            a = np.array([-1.0 - len(axes), 1e-17])
        else:
            a = np.sort(rng.uniform(-1.0, 1.0, n)) if n < 100 else _clustered_axis(rng, n)
        assert not is_uniform(a)
        axes.append(a)
    ncol = 1 if np.prod(shape) > 1_000_000 else NCOL
    grid = _smooth_grid(rng, axes, ncol)
    long_axes = [d for d, n in enumerate(shape) if n >= 100]
    for d in long_axes:
        sl = [slice(None)] * len(axes)
        sl[d] = rng.choice(np.arange(1, shape[d] - 1), min(60, shape[d] // 15), replace=False)
        grid[tuple(sl) + (0,)] = np.nan
    specials = []
    for d, a in enumerate(axes):
        if a.size >= 100:          # a sample of the nodes (the clustered ones included), both ends, and what node_probes adds
            pick = np.unique(np.concatenate([np.arange(12), a.size - 1 - np.arange(12), rng.choice(a.size, min(300, a.size), replace=False),
                                             np.flatnonzero(np.diff(a) < 1e-14)[:60]]))
            sp = a[pick]
            specials.append(np.concatenate([sp, np.nextafter(sp, -np.inf), np.nextafter(sp, np.inf), [0.0, -0.0, np.nan]]))
        else:
            specials.append(node_probes(a))
    probes = _probe_rows(rng, axes, specials, 400)
    return EdgeTable(name, grid, axes, probes)


def _minimum_table(name):
    shape = MINIMUM[name]
    rng = np.random.default_rng([20261022, len(shape)])
    axes = [np.array([-0.25, 0.5]), np.array([0.0, 1e-3]), np.array([1.0, np.nextafter(1.0, np.inf)]), np.array([-3.0, -1.0])][:len(shape)]
    grid = _smooth_grid(rng, axes, NCOL)
    grid[(1,) * len(shape) + (2,)] = np.nan                # one corner missing in one column
    probes = _probe_rows(rng, axes, [node_probes(a) for a in axes], 300)     # (more than 257 rows: the batch sizes of the tests)
    return EdgeTable(name, grid, axes, probes)


@functools.lru_cache(maxsize=None)
def edge_table(name):
    if name in UNIFORM:
        return _uniform_table(name)
    if name in UNSTAGED:
        return _unstaged_table(name)
    return _minimum_table(name)


def edge_tables(names=None):
    """{name: EdgeTable} - U2, U3, U4 (uniform axes whose step is no power of two), the four G tables (an axis beyond, or
    exactly at, the LDS budget) and M2, M3, M4 (two nodes on every axis); fixed seeds, built once per process."""
    names = names or (list(UNIFORM) + list(UNSTAGED) + list(MINIMUM))
    return {n: edge_table(n) for n in names}


def widen(table, ncol=70):
    """The table with its columns repeated (scaled, so that no two are equal) up to `ncol` columns."""
    reps = -(-ncol // table.ncol)
    g = np.concatenate([table.grid * (1.0 + 0.5 * r) for r in range(reps)], axis=-1)[..., :ncol]
    return EdgeTable(table.name + "w", np.ascontiguousarray(g), table.axes, table.probes, table.nan_nodes)


def staged_doubles(axes):
    """assign_lds() of the library: (offset or -1 per axis, doubles used)."""
    used, offs = 0, []
    for a in axes:
        if is_uniform(a) or used + len(a) > MAX_LDS_AXIS_DOUBLES:
            offs.append(-1)
        else:
            offs.append(used)
            used += len(a)
    return offs, used


def fixup_counts_on(grid, axes, xs, axis, guess, icols=None):
    """(decisive rows that need ++k, decisive rows that need --k) on one uniform axis of any table: the rows whose first guess
    on that axis is off by one and whose result under the uncorrected cell has another NaN pattern than the rule's."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    icols = np.arange(np.asarray(grid).shape[-1]) if icols is None else np.asarray(icols)
    valid = np.ones(xs[0].size, dtype=bool)              # in range, no NaN coordinate
    with np.errstate(invalid="ignore"):
        for a, x in zip(axes, xs):
            valid &= (x >= a[0]) & (x <= a[-1])
    need = np.zeros(xs[axis].size, dtype=np.int64)
    need[valid] = fixup_needed(axes[axis], xs[axis][valid], guess)
    out = []
    for want in (1, -1):
        rows = np.flatnonzero(need == want)
        if rows.size == 0:
            out.append(0)
            continue
        _, dec = neighbour(grid, axes, [x[rows] for x in xs], icols, axis, -want)   # guess too low: the uncorrected cell is i - 1
        out.append(int(dec.sum()))
    return tuple(out)


def fixup_counts(table, guess):
    """The same over every axis of a uniform edge table and its probes."""
    up = down = 0
    for d in range(table.nd):
        u, v = fixup_counts_on(table.grid, table.axes, table.xs(), d, guess)
        up, down = up + u, down + v
    return up, down
