"""The numpy twin of include/isochrones_amd_derived.h against the C oracle's interpolator on the same samples, and the
interpolator's rules on a hand-built table; no GPU needed.

Tolerance.  A value is an 8-term sum of float64 products with weights in [0, 1] that sum to 1: two summation orders
differ by a few units of 1e-16 times the largest corner.  |a - b| <= 1e-12 (1 + |b|) leaves three orders of margin and
is tighter than the 1e-9 the project's other tests hold.  NaN positions must be identical."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import _derived_twin as tw


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_twin_matches_the_oracle_interpolator(kind):
    g, axes, cols = tw.grid(kind)
    table = orc.OracleTable(g, axes)
    S, W, T = 5, 26, 4
    x = tw.chain(kind, S, W, T)
    names = ("radius", "Teff", "logg", "mass", "Mbol", "logL", "density", "feh")
    icols = [cols.index(c) for c in names]
    packed, _ = tw.packed(kind, 8)
    seen_nan = seen_fin = 0
    for p0, p1, pk in tw.comps_for(3):
        xs = [x[:, p].ravel() for p in (p0, p1, pk)]
        want = table.interp(xs, icols)
        got = tw.interp(packed, axes, *xs)
        assert tw.close(got, want)
        seen_nan += int(np.isnan(want).sum())
        seen_fin += int(np.isfinite(want).sum())
    assert seen_nan > 50 and seen_fin > 1000           # the samples reach the padding and the table's inside


def test_derive_is_the_interpolator_per_component_and_counts_nans():
    packed, axes = tw.packed("iso", 3)
    S, W, T = 3, 10, 7
    x = tw.chain("iso", S, W, T)
    comps = tw.comps_for(2)
    out, nan_count = tw.derive(x, tw.PARAM_MAJOR, S, W, packed, axes, comps)
    assert out.shape == (T, 6, S * W) and nan_count.shape == (S, 6) and nan_count.dtype == np.int32
    for c, (p0, p1, pk) in enumerate(comps):
        for t in (0, T - 1):
            v = tw.interp(packed, axes, x[t, p0], x[t, p1], x[t, pk])
            np.testing.assert_array_equal(out[t, 3 * c:3 * c + 3], v.T)
    np.testing.assert_array_equal(nan_count[1], np.isnan(out[:, :, W:2 * W]).sum(axis=(0, 2)))
    rows = np.ascontiguousarray(x.transpose(0, 2, 1))
    out_r, nan_r = tw.derive(rows, tw.ROW_MAJOR, S, W, packed, axes, comps)
    np.testing.assert_array_equal(out_r, out)
    np.testing.assert_array_equal(nan_r, nan_count)
    sub, nan_sub = tw.derive(x, tw.PARAM_MAJOR, S, W, packed, axes, comps, ens_begin=1, n_ens_out=2)
    np.testing.assert_array_equal(sub, out[:, :, W:])
    np.testing.assert_array_equal(nan_sub, nan_count[1:])


def _at(x0, x1, xk):
    cols, axes = tw.rule_table()
    return tw.interp(cols, axes, np.array([x0]), np.array([x1]), np.array([xk]))[0]


def test_rules_on_a_hand_built_table():
    nan = np.nan
    # inside, the last axis non-uniform: xk = 3 lies halfway between the nodes 2 and 4
    np.testing.assert_array_equal(_at(0.5, 15.0, 3.0), [56.5, 2.5])
    np.testing.assert_array_equal(_at(0.25, 35.0, 7.0), [25.0 + 17.5 + 2.75, 1.0 + 0.25 * 1.75 + 0.5 * (0.25 * 4 + 0.75 * 9)])
    # on a node: the cell above it, weight 0 on every other corner
    np.testing.assert_array_equal(_at(1.0, 20.0, 2.0), [111.0, 2.5])
    np.testing.assert_array_equal(_at(0.0, 10.0, 1.0), [0.0, 1.0])
    # on the last node of each axis: the cell below, weight 1
    np.testing.assert_array_equal(_at(2.0, 15.0, 3.0), [206.5, 1.0 + 1.0 + 1.25])
    np.testing.assert_array_equal(_at(0.5, 40.0, 3.0), [71.5, 1.0 + 1.0 + 1.25])
    np.testing.assert_array_equal(_at(0.5, 15.0, 8.0), [58.0, 1.25 + 4.5])
    # off either end of each axis, and a NaN coordinate
    for q in ((-0.1, 15.0, 3.0), (2.1, 15.0, 3.0), (0.5, 9.0, 3.0), (0.5, 41.0, 3.0), (0.5, 15.0, 0.5), (0.5, 15.0, 8.5),
              (nan, 15.0, 3.0), (0.5, nan, 3.0), (0.5, 15.0, nan)):
        np.testing.assert_array_equal(_at(*q), [nan, nan])
    # the NaN node (2, 2, 3): a corner of the cell above (1, 1, 2) with weight zero, and the last node itself
    np.testing.assert_array_equal(_at(1.0, 20.0, 4.0), [nan, nan])
    np.testing.assert_array_equal(_at(2.0, 40.0, 8.0), [nan, nan])
    np.testing.assert_array_equal(_at(1.5, 30.0, 6.0), [nan, nan])           # inside the cell that has it
    np.testing.assert_array_equal(_at(1.0, 20.0, 3.0), [111.5, 3.25])         # the cell below it along the last axis
    np.testing.assert_array_equal(_at(0.5, 15.0, 6.0), [50.0 + 5.0 + 2.5, 1.25 + 0.5 * 6.5])     # a cell away from it


def test_bracket_rules():
    ax = np.array([1.0, 2.0, 4.0, 8.0])
    i, t = tw.bracket(ax, np.array([1.0, 1.5, 2.0, 3.0, 8.0, np.nan]))
    np.testing.assert_array_equal(i, [0, 0, 1, 1, 2, 0])
    np.testing.assert_array_equal(t[:5], [0.0, 0.5, 0.0, 0.5, 1.0])
