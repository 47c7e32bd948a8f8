"""TEST INFRASTRUCTURE - seeded tables and query sets for the edge tests of the exact EEP solve (libiso_solve.so): ragged
finite ranges, holes, plateaus, every axis length around the powers of two, and queries drawn per cell so that every
branch of the kernel is reached on purpose.  numpy and the twin (tests/_solve_twin.py, built on the CPU oracle) only:
nothing here imports the package under test.  tests/test_solve_cases_cpu.py proves on the CPU that the generators reach
every class of query; tests/test_gpu_solve_edges.py runs the same (table, query set) pairs on the device."""
import functools

import numpy as np

from tests import _solve_twin as T

NAN, INF = float("nan"), float("inf")

#: (n0, n1, nk) of test_bit_identity_on_ragged_tables
SHAPES = [(2, 2, 2), (2, 3, 3), (3, 2, 4), (3, 5, 7), (4, 3, 9), (5, 4, 17), (7, 6, 33), (3, 3, 64)]
HOLE_SHAPES = [(4, 3, 9), (5, 4, 17), (3, 3, 64)]
#: axis lengths of test_bracket_every_axis_length: 2, 3 and each side of every power of two up to 32
BRACKET_LENGTHS = [2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33]
#: uneven fractions of a segment (not representable sums of few powers of two: the division has to round)
FRACTIONS = (0.3137, 0.71)


def axis(rng, n, zero_at=None):
    """A strictly increasing, non-uniform axis of n nodes with negative and positive nodes; ``zero_at``: the index of a
    node that is exactly 0.0."""
    x = np.cumsum(rng.uniform(0.3, 1.7, n))
    x -= x[n // 2 if zero_at is None else zero_at] + (0.123 if zero_at is None else 0.0)
    if zero_at is not None:
        x[zero_at] = 0.0
    assert np.all(np.diff(x) > 0)
    return x


def _kind_range(rng, kind, nk):
    """[first, last] of a column of one kind; kinds that do not fit into nk knots degrade to a one-knot column."""
    if kind == "full":
        return 0, nk - 1
    if kind == "empty":
        return nk, -1
    if kind == "top" and nk >= 3:                             # short at the top
        return 0, int(rng.integers(1, nk - 1))
    if kind == "bottom" and nk >= 3:
        return int(rng.integers(1, nk - 1)), nk - 1
    if kind == "both" and nk >= 4:
        f = int(rng.integers(1, nk - 2))
        return f, int(rng.integers(f + 1, nk - 1))
    k = int(rng.integers(0, nk))
    return k, k


KINDS = ("full", "top", "bottom", "both", "one", "empty")


def _cells(n0, n1):
    return [(i, j) for i in range(n0 - 1) for j in range(n1 - 1)]


def _corners(i, j):
    return [(i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)]


def _g_finite(fin, cell):
    """Where g is finite in a cell, from where its four columns are: g(k) multiplies the corners at k and k + 1 (the
    last knot: k - 1 and k) whatever their weights."""
    both = np.logical_and.reduce([fin[p] for p in _corners(*cell)])
    g = np.zeros(both.size, dtype=bool)
    g[:-1] = both[:-1] & both[1:]
    g[-1] = both[-1] & both[-2]
    return g


def _hole_classes(fin, first, last, cell):
    """Which of the four hole classes of tests/test_solve_cases_cpu.py the queries of one cell can fall into."""
    F, L = max(first[p] for p in _corners(*cell)), min(last[p] for p in _corners(*cell))
    holes = [k for p in _corners(*cell) for k in range(first[p], last[p] + 1) if not fin[p][k]]
    out = set()
    if not holes or F > L:
        return out
    inside = any(F <= k <= L for k in holes)
    g = _g_finite(fin, cell)
    seen = False
    for k in range(F, L + 1):
        if g[k]:
            if k > F:
                out.add(("hole_in" if inside else "hole_out") if g[k - 1] else ("prev_nan" if seen else "first_nan"))
            seen = True
    return out


def _layout(rng, n0, n1, nk, holes):
    """(first[n0, n1], last[n0, n1], {(i, j): [(k, value), ...]} of the holes).  One cell keeps four full columns without
    holes.  Tables of nine or more columns hold every kind of column, a pair of nonempty neighbours (corners of one cell)
    with disjoint ranges, an empty intersection and a cell whose F and L come from different columns; smaller ones hold
    what fits: the full cell and, with two cells, one whose intersection is empty.  With holes, the cells reach all four
    hole classes between them; a 3 x 3 table has no room for that next to a one-knot and an empty column (each
    kills every cell it touches, and three cells have to live), so there the one-knot column is left out."""
    big = n0 * n1 >= 9
    must = list(KINDS[1:]) if big else []
    if holes and n0 * n1 == 9:
        must.remove("one")
    for _ in range(20000):
        pi, pj = int(rng.integers(0, n0 - 1)), int(rng.integers(0, n1 - 1))
        kinds = np.full((n0, n1), "full", dtype=object)
        free = [(i, j) for i in range(n0) for j in range(n1) if (i, j) not in _corners(pi, pj)]
        rng.shuffle(free)
        p_kind = [0.4, 0.2, 0.2, 0.2, 0.0, 0.0] if holes else [0.3, 0.2, 0.2, 0.15, 0.075, 0.075]
        for n, (i, j) in enumerate(free):
            kinds[i, j] = must[n] if n < len(must) else rng.choice(KINDS, p=p_kind)
        first, last = np.empty((n0, n1), dtype=int), np.empty((n0, n1), dtype=int)
        for i in range(n0):
            for j in range(n1):
                first[i, j], last[i, j] = _kind_range(rng, kinds[i, j], nk)
        F = {c: max(first[p] for p in _corners(*c)) for c in _cells(n0, n1)}
        L = {c: min(last[p] for p in _corners(*c)) for c in _cells(n0, n1)}
        empty_cell = any(F[c] > L[c] for c in F)
        disjoint = any(first[p] <= last[p] and first[q] <= last[q] and (first[p] > last[q] or first[q] > last[p])
                       for c in F for p in _corners(*c) for q in _corners(*c))
        # a ragged cell that still has a segment to invert, its ends set by two different columns
        mixed = any(L[c] - F[c] >= 2 and len({p for p in _corners(*c) if first[p] == F[c]} |
                                              {p for p in _corners(*c) if last[p] == L[c]}) >= 2
                    and (F[c] > 0 or L[c] < nk - 1) for c in F)
        if big and not (empty_cell and disjoint and mixed):
            continue
        if not big and len(F) >= 2 and not empty_cell:
            continue
        where = {}
        if holes:
            cand = [p for p in free if last[p] - first[p] >= 3]
            if len(cand) < min(holes, 3):
                continue
            fin = np.zeros((n0, n1, nk), dtype=bool)
            for i in range(n0):
                for j in range(n1):
                    fin[i, j, first[i, j]:last[i, j] + 1] = True
            for n, p in enumerate(cand[:holes]):
                f, l = first[p], last[p]
                mid = int(rng.integers(f + 2, l - 1)) if l - f >= 4 else f + 1
                ks = [[l - 1], [f + 1], [mid], [mid, int(rng.integers(mid, l))]][n % 4]
                where[p] = [(k, INF if n % 2 else NAN) for k in sorted(set(ks))]
                fin[p][[k for k, _ in where[p]]] = False
            reached = set().union(*[_hole_classes(fin, first, last, c) for c in F])
            if reached != {"hole_in", "hole_out", "prev_nan", "first_nan"}:
                continue
        return first, last, where
    raise AssertionError("no layout found for %r" % ((n0, n1, nk),))


def ragged(rng, n0, n1, nk, holes=0):
    """(col[n0, n1, nk], (ax0, ax1, axk)): nondecreasing NaN-padded columns with their own [first, last], plateaus of
    length 2 to 5, a per-column offset and scale, and with ``holes`` > 0 that many columns with a NaN or +inf strictly
    inside their range (last - 1, first + 1 and positions further inside in turn)."""
    axes = (axis(rng, n0, zero_at=int(rng.integers(0, n0))), axis(rng, n1), axis(rng, nk, zero_at=int(rng.integers(0, nk))))
    first, last, where = _layout(rng, n0, n1, nk, holes)
    steps = rng.uniform(0.2, 1.0, nk)
    k = 1
    while k < nk - 1:                                         # shared plateaus: g has them at every (x0, x1)
        run = int(rng.integers(1, 5))                         # 1 to 4 zero steps: 2 to 5 equal values
        if rng.random() < 0.35:
            steps[k:min(k + run, nk - 1)] = 0.0               # never the last step: the top knot stays reachable
            k += run
        k += int(rng.integers(1, 4))
    if nk >= 3 and not (steps[1:] == 0.0).any():
        steps[int(rng.integers(1, nk - 1))] = 0.0
    col = np.full((n0, n1, nk), NAN)
    for i in range(n0):
        for j in range(n1):
            s = steps * rng.uniform(0.6, 1.4)
            s[:nk - 1][rng.random(nk - 1) < 0.1] = 0.0        # and the column's own
            v = (1.0 + 0.37 * i * i + 0.53 * j * j + 0.29 * i * j + rng.uniform(0.0, 0.05)) + np.cumsum(s)
            col[i, j, first[i, j]:last[i, j] + 1] = v[first[i, j]:last[i, j] + 1]
    for (i, j), ks in where.items():
        for k, v in ks:
            col[i, j, k] = v
    return col, axes


def hole_positions(col):
    """{(i, j): [k, ...]}: the non-finite entries strictly inside every column's [first, last], in plain Python."""
    out = {}
    n0, n1, nk = col.shape
    for i in range(n0):
        for j in range(n1):
            fin = [k for k in range(nk) if np.isfinite(col[i, j, k])]
            if fin:
                bad = [k for k in range(fin[0], fin[-1] + 1) if not np.isfinite(col[i, j, k])]
                if bad:
                    out[(i, j)] = bad
    return out


def _coords(rng, ax, i):
    """Coordinates that the interpolator puts into cell i of an axis: its lower node, one ulp above it, one ulp below
    its upper node, two interior points; the last cell also gets the last node of the axis (twice: its class is rare)."""
    lo, hi = ax[i], ax[i + 1]
    xs = [lo, np.nextafter(lo, INF), np.nextafter(hi, -INF), lo + 0.5 * (hi - lo), lo + rng.uniform(0.05, 0.95) * (hi - lo)]
    if i == ax.size - 2:
        xs += [hi, hi]
    return xs


def _targets(rng, g, F, L, span):
    """Targets for one (x0, x1) from its own knot values g[nk]: see the module docstring of the CPU test for the
    classes they are meant to reach."""
    nk = g.size
    if F > L or not np.isfinite(g[F:L + 1]).any():
        return list(rng.uniform(span[0], span[1], 5))
    fin = [k for k in range(F, L + 1) if np.isfinite(g[k])]
    out = [g[F], np.nextafter(g[fin[0]], -INF), g[fin[-1]], np.nextafter(g[fin[-1]], INF), g[fin[0]]]
    seg = [k for k in fin if k > F and np.isfinite(g[k - 1])]
    for k in (rng.choice(seg, size=min(3, len(seg)), replace=False) if seg else []):
        out += [g[k], 0.5 * (g[k - 1] + g[k])] + [g[k - 1] + f * (g[k] - g[k - 1]) for f in FRACTIONS]
    flat = [k for k in fin if k + 1 <= L and g[k + 1] == g[k]]
    for k in (rng.choice(flat, size=min(2, len(flat)), replace=False) if flat else []):
        out.append(g[k])                                      # a value the column holds at two knots or more
    if L == nk - 1 and nk - 1 in seg:                         # the top knot: the cell below it, weight 1
        out += [g[nk - 1], g[nk - 2] + FRACTIONS[0] * (g[nk - 1] - g[nk - 2])]
    for k in fin:                                             # the first finite g behind a hole: g(k* - 1) is NaN
        if k > F and not np.isfinite(g[k - 1]):
            under = [g[m] for m in fin if m < k]
            out += [g[k], np.nextafter(g[k], -INF)] + ([under[-1] + f * (g[k] - under[-1]) for f in FRACTIONS] if under else [])
    return [y for y in out if np.isfinite(y)]


def queries(rng, col, axes, pairs=None):
    """(x0, x1, target) for a table: per cell ``pairs`` coordinate pairs that cover every coordinate of _coords on
    both axes, and per pair the targets of _targets."""
    n0, n1, nk = col.shape
    cells = _cells(n0, n1)
    pairs = pairs or max(24, -(-96 // len(cells)))
    a, b = [], []
    for i, j in cells:
        c0, c1 = _coords(rng, axes[0], i), _coords(rng, axes[1], j)
        for n in range(pairs):
            a.append(c0[n % len(c0)])
            b.append(c1[(n // len(c0) + n) % len(c1)])
    a, b = np.array(a), np.array(b)
    g = T.knot_values(col[..., None], axes, 0, a, b)
    _, _, _, F, L = T.cell_ranges(col, axes, a, b)
    span = (np.nanmin(np.where(np.isfinite(col), col, NAN)) - 0.5, np.nanmax(np.where(np.isfinite(col), col, NAN)) + 0.5)
    x0, x1, y = [], [], []
    for n in range(a.size):
        ts = _targets(rng, g[n], int(F[n]), int(L[n]), span)
        x0 += [a[n]] * len(ts)
        x1 += [b[n]] * len(ts)
        y += ts
    return np.array(x0), np.array(x1), np.array(y)


def _first_segment(g):
    """The smallest k with g(k - 1) and g(k) finite and different (None: there is none)."""
    for k in range(1, g.size):
        if np.isfinite(g[k - 1]) and np.isfinite(g[k]) and g[k] > g[k - 1]:
            return k
    return None


def specials(col, axes):
    """The fixed special queries of a table: NaN and +-inf in each input, coordinates one ulp outside each end of each
    axis, -0.0 and 0.0 on an axis node at 0.0 -> (x0, x1, target, tag); ``tag`` names what the row is."""
    ax0, ax1 = axes[0], axes[1]
    zero = [int(np.flatnonzero(ax == 0.0)[0]) if (ax == 0.0).any() else None for ax in (ax0, ax1)]
    rows = []
    for i, j in _cells(*col.shape[:2]):
        a, b = ax0[i] + 0.37 * (ax0[i + 1] - ax0[i]), ax1[j] + 0.61 * (ax1[j + 1] - ax1[j])
        g = T.knot_values(col[..., None], axes, 0, [a], [b])[0]
        seg = _first_segment(g)
        if seg is None:
            continue
        y = 0.5 * (g[seg - 1] + g[seg])
        rows.append((a, b, y, "plain"))
        for v, name in ((NAN, "nan"), (INF, "+inf"), (-INF, "-inf")):
            rows += [(v, b, y, name + " x0"), (a, v, y, name + " x1"), (a, b, v, name + " target")]
        rows += [(np.nextafter(ax0[0], -INF), b, y, "below x0"), (np.nextafter(ax0[-1], INF), b, y, "above x0"),
                 (a, np.nextafter(ax1[0], -INF), y, "below x1"), (a, np.nextafter(ax1[-1], INF), y, "above x1")]
    for d, z in enumerate(zero):
        if z is None:
            continue
        for i, j in _cells(*col.shape[:2]):
            other = (ax1[j] + 0.61 * (ax1[j + 1] - ax1[j])) if d == 0 else (ax0[i] + 0.37 * (ax0[i + 1] - ax0[i]))
            for zv, name in ((0.0, "+0.0"), (-0.0, "-0.0")):
                a, b = (zv, other) if d == 0 else (other, zv)
                g = T.knot_values(col[..., None], axes, 0, [a], [b])[0]
                seg = _first_segment(g)
                if seg is not None:
                    for f in FRACTIONS:
                        rows.append((a, b, g[seg - 1] + f * (g[seg] - g[seg - 1]), name + " x%d" % d))
    x0, x1, y = (np.array([r[k] for r in rows], dtype=float) for k in range(3))
    return x0, x1, y, [r[3] for r in rows]


def special_table(kind):
    """Small tables for the special values: ``zero`` has a node at 0.0 on ax0 (the first node) and on ax1 (an inner
    node); ``inf_pad`` is padded with +inf instead of NaN behind every range; ``inf_inside`` holds +inf strictly inside
    two ranges (not on the first knot of any cell's intersection)."""
    rng = np.random.default_rng(77)
    n0, n1, nk = 3, 4, 8
    ax0, ax1, axk = axis(rng, n0, zero_at=0), axis(rng, n1, zero_at=2), axis(rng, nk, zero_at=3)
    col = np.empty((n0, n1, nk))
    for i in range(n0):
        for j in range(n1):
            s = rng.uniform(0.2, 1.0, nk)
            s[0] = 0.0
            col[i, j] = (1.0 + 0.37 * i * i + 0.53 * j * j + 0.29 * i * j) + np.cumsum(s)
    if kind == "inf_pad":
        col[0, 1, 6:] = INF
        col[1, 2, 5:] = INF
        col[2, 0, 7:] = INF
        col[2, 3, :2] = NAN
    elif kind == "inf_inside":
        col[1, 1, 5] = INF                                    # every neighbour starts at 0: never a first knot
        col[2, 3, 6] = INF
    else:
        assert kind == "zero"
    return col, (ax0, ax1, axk)


def bracket_table(which, n):
    """Full columns on non-uniform axes with ``n`` nodes on axis ``which`` (0 or 1), 3 on the other and nk = 5; the
    column value is not bilinear in (i, j), so a blend of the wrong cell's corners gives another g."""
    rng = np.random.default_rng(1000 * which + n)
    n0, n1 = (n, 3) if which == 0 else (3, n)
    axes = (axis(rng, n0), axis(rng, n1), axis(rng, 5))
    i, j = np.arange(n0)[:, None, None], np.arange(n1)[None, :, None]
    prof = np.array([0.0, 0.7, 1.1, 2.3, 2.9])[None, None, :]
    col = 3.0 * i * i + 1.7 * j * j + 0.9 * i * j + 0.25 * i + 0.125 * j + prof * (1.0 + 0.1 * i + 0.05 * j)
    return np.ascontiguousarray(col, dtype=float), axes


def bracket_queries(col, axes, which):
    """Axis ``which`` at every node, one ulp each side of every node and the middle of every cell; the other axis at an
    interior point, on a node and on its last node; targets at uneven fractions of each of the four segments."""
    ax = axes[which]
    xs = np.concatenate([ax, np.nextafter(ax, -INF), np.nextafter(ax, INF), 0.5 * (ax[:-1] + ax[1:])])
    o = axes[1 - which]
    others = np.array([o[0] + 0.41 * (o[1] - o[0]), o[1], o[-1]])
    a, b = np.repeat(xs, others.size), np.tile(others, xs.size)
    if which == 1:
        a, b = b, a
    g = T.knot_values(col[..., None], axes, 0, a, b)
    x0, x1, y = [], [], []
    for k in range(1, col.shape[2]):
        for n, f in enumerate(FRACTIONS):
            if (k + n) % 2:
                continue
            x0.append(a)
            x1.append(b)
            t = g[:, k - 1] + f * (g[:, k] - g[:, k - 1])
            y.append(np.where(np.isfinite(t), t, 1.0))        # off the axis: any target, the answer is NaN
    return np.concatenate(x0), np.concatenate(x1), np.concatenate(y)


def _seed(shape, holes):
    return 100000 * bool(holes) + 1000 * shape[0] + 100 * shape[1] + shape[2]


@functools.lru_cache(maxsize=None)
def ragged_case(shape, holes=0):
    """(col, axes, x0, x1, target, (e, g_lo, g_hi, k_star) of the twin) for one parametrisation of the ragged-table
    tests, made once per process and shared (read only)."""
    rng = np.random.default_rng(_seed(shape, holes))
    col, axes = ragged(rng, *shape, holes=holes)
    x0, x1, y = queries(rng, col, axes)
    sx0, sx1, sy, _ = specials(col, axes)
    x0, x1, y = np.concatenate([x0, sx0]), np.concatenate([x1, sx1]), np.concatenate([y, sy])
    want = T.solve(col[..., None], axes, 0, x0, x1, y)
    for v in (col, x0, x1, y) + tuple(axes) + tuple(want):
        v.setflags(write=False)
    return col, axes, x0, x1, y, want


def n_holes(shape):
    """Hole columns of a table with holes: a third of its columns."""
    return max(3, shape[0] * shape[1] // 3)


@functools.lru_cache(maxsize=None)
def bracket_case(which, n):
    col, axes = bracket_table(which, n)
    x0, x1, y = bracket_queries(col, axes, which)
    want = T.solve(col[..., None], axes, 0, x0, x1, y)
    return col, axes, x0, x1, y, want


@functools.lru_cache(maxsize=None)
def special_case(kind):
    col, axes = special_table(kind)
    x0, x1, y, tags = specials(col, axes)
    want = T.solve(col[..., None], axes, 0, x0, x1, y)
    return col, axes, x0, x1, y, tags, want
