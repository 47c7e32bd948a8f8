"""The generators of tests/_solve_tables.py do their job: for every (table, query set) that tests/test_gpu_solve_edges.py
runs on the device, the twin alone (tests/_solve_twin.py) puts at least MIN_PER_CLASS queries into every class of query
the table can produce, so that the comparison on the device cannot pass vacuously.  The counts are conditions on the
inputs, not measurements; they are printed.  No GPU is used.

Classes (F, L: the intersection of the four corner columns' ranges as ``column_ranges`` gives them; g: the oracle
interpolator's value at every knot; k*, e: the twin's):
  segment       finite e from a segment inverse (k* > F) in a cell without a hole flag
  first_knot    e = axk[F]: g(F) == target
  below         inside the table, F <= L, k* == F and g(F) > target: NaN
  above         inside the table, some finite g in [F, L], no k*: NaN
  top           finite e with k* == nk - 1 (the last knot: the cell below it with weight 1)
  plateau       finite e, g(k*) == target and g(k* + 1) == g(k*) with k* + 1 <= L: the smallest k of a plateau wins
  empty         inside the table, F > L
  x0_last       x0 on the last node of ax0 (the cell below it, t = 1)
  x1_last       x1 on the last node of ax1
and on tables with holes:
  hole_in       finite e from a cell with a hole flag whose hole lies inside [F, L]
  hole_out      finite e from a cell with a hole flag whose holes all lie outside [F, L]
  prev_nan      NaN because g(k* - 1) is NaN, with a finite g further down in the range
  first_nan     NaN because g(F) is NaN and nothing finite lies between F and k*
"""
import numpy as np
import pytest

from isochrones_amd import _solve_cabi, solve
from tests import _solve_tables as G
from tests import _solve_twin as T

MIN_PER_CLASS = 30
BASE = ("segment", "first_knot", "below", "above", "top", "x0_last", "x1_last")
HOLES = ("hole_in", "hole_out", "prev_nan", "first_nan")


def expected_classes(shape, holes):
    """What a table of this shape can produce: a plateau needs three knots, an empty intersection a second cell (the
    first one is the full cell that ``top`` needs)."""
    n0, n1, nk = shape
    out = list(BASE)
    if nk >= 3:
        out.append("plateau")
    if (n0 - 1) * (n1 - 1) >= 2:
        out.append("empty")
    return out + (list(HOLES) if holes else [])


def _plain_ranges(col):
    """first, last and hole flag per column in plain Python."""
    n0, n1, nk = col.shape
    first, last, flag = np.full((n0, n1), nk), np.full((n0, n1), -1), np.zeros((n0, n1), dtype=bool)
    for i in range(n0):
        for j in range(n1):
            fin = [k for k in range(nk) if col[i, j, k] == col[i, j, k] and abs(col[i, j, k]) != float("inf")]
            if fin:
                first[i, j], last[i, j] = fin[0], fin[-1]
                flag[i, j] = len(fin) != fin[-1] - fin[0] + 1
    return first, last, flag


def check_ranges(col):
    r = solve.column_ranges(col)                              # accepts the table: nondecreasing between finite neighbours
    first, last, flag = _plain_ranges(col)
    tf, tl = T.finite_ranges(col)
    np.testing.assert_array_equal(first, tf)
    np.testing.assert_array_equal(last, tl)
    np.testing.assert_array_equal(r[..., 0] & ~_solve_cabi.HOLE_BIT, first)
    np.testing.assert_array_equal(r[..., 1], last)
    np.testing.assert_array_equal((r[..., 0] & _solve_cabi.HOLE_BIT) != 0, flag)
    return r


def classify(col, axes, x0, x1, y, want):
    """{class: boolean mask over the queries}."""
    e, _, _, ks = want
    n0, n1, nk = col.shape
    r = check_ranges(col)
    first, last, flagc = r[..., 0] & ~_solve_cabi.HOLE_BIT, r[..., 1], (r[..., 0] & _solve_cabi.HOLE_BIT) != 0
    ok, i, j, _, _ = T.cell_ranges(col, axes, x0, x1)
    corners = [(i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)]
    F = np.maximum.reduce([first[c] for c in corners])
    L = np.minimum.reduce([last[c] for c in corners])
    flag = np.logical_or.reduce([flagc[c] for c in corners])
    g = T.knot_values(col[..., None], axes, 0, x0, x1)
    n = x0.size
    rows = np.arange(n)
    fin_e, fin_y = np.isfinite(e), np.isfinite(y)
    ks_c = np.clip(ks, 0, nk - 1)
    in_range = (np.arange(nk)[None, :] >= F[:, None]) & (np.arange(nk)[None, :] <= L[:, None])
    some_g = (np.isfinite(g) & in_range).any(axis=1)
    holes = G.hole_positions(col)
    inside = np.zeros(n, dtype=bool)
    for q in np.flatnonzero(flag & ok):
        ps = [p for c in corners for p in holes.get((int(c[0][q]), int(c[1][q])), [])]
        inside[q] = any(F[q] <= p <= L[q] for p in ps)
    below_k = np.arange(nk)[None, :] < ks[:, None]
    fin_below = (np.isfinite(g) & in_range & below_k).any(axis=1)            # a finite g in [F, k*)
    g_prev = g[rows, np.clip(ks - 1, 0, nk - 1)]
    g_next = g[rows, np.clip(ks + 1, 0, nk - 1)]
    with np.errstate(invalid="ignore"):
        cls = {
            "segment": ok & fin_e & (ks > F) & ~flag,
            "first_knot": ok & fin_e & (ks == F),
            "below": ok & fin_y & (F <= L) & (ks == F) & ~fin_e & (g[rows, ks_c] > y),
            "above": ok & fin_y & some_g & (ks == -1),
            "top": ok & fin_e & (ks == nk - 1),
            "plateau": ok & fin_e & (ks >= 0) & (g[rows, ks_c] == y) & (ks + 1 <= L) & (g_next == g[rows, ks_c]),
            "empty": ok & fin_y & (F > L),
            "x0_last": ok & fin_y & (x0 == axes[0][-1]),
            "x1_last": ok & fin_y & (x1 == axes[1][-1]),
            "hole_in": ok & fin_e & flag & inside,
            "hole_out": ok & fin_e & flag & ~inside,
            "prev_nan": ok & fin_y & (ks > F) & np.isnan(g_prev) & fin_below,
            "first_nan": ok & fin_y & (ks > F) & np.isnan(g[rows, np.clip(F, 0, nk - 1)]) & ~fin_below,
        }
    assert not (cls["prev_nan"] | cls["first_nan"])[fin_e].any()
    return cls


def _report(label, cls, wanted, n):
    counts = {k: int(cls[k].sum()) for k in cls}
    print("%s: %d queries; %s" % (label, n, ", ".join("%s %d" % (k, counts[k]) for k in BASE + ("plateau", "empty") + HOLES)))
    short = {k: counts[k] for k in wanted if counts[k] < MIN_PER_CLASS}
    assert not short, "%s: too few queries in %r (need %d each)" % (label, short, MIN_PER_CLASS)


@pytest.mark.parametrize("shape,holes", [(s, 0) for s in G.SHAPES] + [(s, 1) for s in G.HOLE_SHAPES])
def test_every_class_is_reached_on_the_ragged_tables(shape, holes, capsys):
    col, axes, x0, x1, y, want = G.ragged_case(shape, G.n_holes(shape) if holes else 0)
    cls = classify(col, axes, x0, x1, y, want)
    with capsys.disabled():
        print()
        _report("ragged %r%s" % (shape, " with holes" if holes else ""), cls, expected_classes(shape, holes), x0.size)
    assert x0.size <= 20000                                   # a few thousand queries per table, not a benchmark
    if holes:
        vals = col[np.isinf(col)]
        assert vals.size and (vals > 0).all() and np.isnan(col).any()


@pytest.mark.parametrize("shape,holes", [(s, 0) for s in G.SHAPES] + [(s, 1) for s in G.HOLE_SHAPES])
def test_ragged_tables_hold_what_they_promise(shape, holes):
    col, axes = G.ragged(np.random.default_rng(G._seed(shape, holes)), *shape, holes=G.n_holes(shape) if holes else 0)
    np.testing.assert_array_equal(col, G.ragged_case(shape, G.n_holes(shape) if holes else 0)[0])   # seeded
    n0, n1, nk = shape
    for ax in axes:
        d = np.diff(ax)
        assert (d > 0).all() and ax[0] <= 0 and (d.size < 2 or np.ptp(d) > 0.01)    # increasing, not all positive, not uniform
    assert (axes[0] == 0.0).any() and (axes[2] == 0.0).any()
    first, last, flag = _plain_ranges(col)
    check_ranges(col)
    assert flag.any() == bool(holes)
    if n0 * n1 >= 9:
        full = (first == 0) & (last == nk - 1)
        assert full.any()
        assert ((first > 0) & (last == nk - 1) & (first < last)).any()              # short at the bottom
        assert ((first == 0) & (last < nk - 1) & (first < last)).any()              # short at the top
        if nk >= 4:
            assert ((first > 0) & (last < nk - 1) & (first < last)).any()           # at both ends
        assert (first > last).any()                                                 # no finite entry
        assert (first == last).any() or (holes and n0 * n1 == 9)                    # one knot (see _solve_tables._layout)
        disjoint = False
        for i, j in G._cells(n0, n1):
            cs = [c for c in G._corners(i, j) if first[c] <= last[c]]
            disjoint |= any(first[p] > last[q] for p in cs for q in cs)
        assert disjoint
    steps = np.diff(col, axis=2)
    assert (steps[np.isfinite(steps)] >= 0).all()
    if nk >= 3:
        assert (steps == 0).any()
    # evaluating the neighbouring cell instead changes every solution
    _, _, x0, x1, y, want = G.ragged_case(shape, G.n_holes(shape) if holes else 0)
    solved = np.isfinite(want[0])
    for axis_ in (0, 1):
        if shape[axis_] > 2:                                  # with two nodes a shift is a swap: midpoints cannot tell
            e2 = T.solve(np.roll(col, 1, axis=axis_)[..., None], axes, 0, x0, x1, y)[0]
            assert (np.isnan(e2[solved]) | (e2[solved] != want[0][solved])).all()
    if holes:
        pos = G.hole_positions(col)
        assert len(pos) >= 3
        assert any(first[c] + 1 in ks for c, ks in pos.items()) and any(last[c] - 1 in ks for c, ks in pos.items())
        outside = False                                       # a hole outside the intersection of a cell it belongs to
        for i, j in G._cells(n0, n1):
            F, L = max(first[c] for c in G._corners(i, j)), min(last[c] for c in G._corners(i, j))
            outside |= F <= L and any(k < F or k > L for c in G._corners(i, j) for k in pos.get(c, []))
        assert outside


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n", G.BRACKET_LENGTHS)
def test_bracket_queries_tell_a_wrong_cell(which, n):
    """Every query of the bracket tables has an answer that changes when the table is shifted by one node along either
    axis, which is what a search that lands one cell off computes."""
    col, axes, x0, x1, y, want = G.bracket_case(which, n)
    check_ranges(col)
    assert col.shape == ((n, 3, 5) if which == 0 else (3, n, 5)) and np.isfinite(col).all()
    for ax in axes:
        assert (np.diff(ax) > 0).all() and np.ptp(np.diff(ax)) > 0.01 or ax.size == 2
    e = want[0]
    ok, i, j, _, _ = T.cell_ranges(col, axes, x0, x1)
    np.testing.assert_array_equal(np.isfinite(e), ok)         # full columns, targets inside a segment: all solved
    ax = axes[which]
    x = x0 if which == 0 else x1
    for node in range(n):                                     # every node, and one ulp each side of it
        for v in (ax[node], np.nextafter(ax[node], -np.inf), np.nextafter(ax[node], np.inf)):
            assert (x == v).sum() >= 4
    for c in range(n - 1):
        assert ((i if which == 0 else j)[ok] == c).sum() >= 4
        assert (x == 0.5 * (ax[c] + ax[c + 1])).sum() >= 4
    assert (~ok).sum() >= 8                                   # one ulp outside each end
    for axis_ in (0, 1):
        # with two nodes a shift is a swap, which the exact middle of the only cell cannot tell (nor can a search be wrong)
        tell = ok & (x != 0.5 * (ax[0] + ax[1])) if (n == 2 and axis_ == which) else ok
        for shift in (1, -1):
            e2 = T.solve(np.roll(col, shift, axis=axis_)[..., None], axes, 0, x0, x1, y)[0]
            changed = np.isnan(e2[tell]) | (e2[tell] != e[tell])
            assert changed.all(), (axis_, shift, int((~changed).sum()))
    ks = want[3][ok]
    assert set(ks) == {1, 2, 3, 4}


@pytest.mark.parametrize("kind", ["zero", "inf_pad", "inf_inside"])
def test_special_tables_and_queries(kind, capsys):
    col, axes, x0, x1, y, tags, want = G.special_case(kind)
    r = check_ranges(col)
    flagged = ((r[..., 0] & _solve_cabi.HOLE_BIT) != 0).sum()
    assert flagged == (2 if kind == "inf_inside" else 0)
    assert np.isposinf(col).any() == (kind != "zero")
    assert axes[0][0] == 0.0 and axes[1][2] == 0.0
    e = want[0]
    tags = np.array(tags)
    with capsys.disabled():
        print("\n%s: %d special queries, %d finite" % (kind, e.size, np.isfinite(e).sum()))
    for name in ("nan", "+inf", "-inf"):
        for what in ("x0", "x1", "target"):
            m = tags == "%s %s" % (name, what)
            assert m.sum() >= 4 and np.isnan(e[m]).all()      # worked by hand: none of these has a solution
    for name in ("below x0", "above x0", "below x1", "above x1"):
        assert (tags == name).sum() >= 4 and np.isnan(e[tags == name]).all()
    assert np.isfinite(e[tags == "plain"]).sum() >= 4
    for d in (0, 1):
        plus, minus = tags == "+0.0 x%d" % d, tags == "-0.0 x%d" % d
        assert plus.sum() >= 4 and np.isfinite(e[plus]).sum() >= 4
        assert np.signbit((x0 if d == 0 else x1)[minus]).all() and not np.signbit((x0 if d == 0 else x1)[plus]).any()
        np.testing.assert_array_equal(e[plus], e[minus])      # -0.0 is the node at 0.0


def test_column_ranges_takes_an_inf_inside_a_range_as_a_hole():
    col = G.special_table("inf_inside")[0]
    r = solve.column_ranges(col)
    assert r[1, 1, 0] == _solve_cabi.HOLE_BIT and r[1, 1, 1] == col.shape[2] - 1
    bad = col.copy()
    bad[0, 0, 4] = bad[0, 0, 3] - 0.5                         # a fall between finite neighbours is still refused
    with pytest.raises(ValueError, match=r"\(0, 0, 4\)"):
        solve.column_ranges(bad)
