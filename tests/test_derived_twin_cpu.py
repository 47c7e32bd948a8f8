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


def test_rules_on_a_hand_built_table():
    cols, axes = tw.rule_table()
    for (x0, x1, xk), want in tw.RULES:
        got = tw.interp(cols, axes, np.array([x0]), np.array([x1]), np.array([xk]))[0]
        np.testing.assert_array_equal(got, want, err_msg=repr((x0, x1, xk)))
    assert sum(np.isnan(w[0]) for _, w in tw.RULES) == 12 and len(tw.RULES) == 21


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_twin_stays_within_the_rounding_bound_of_long_double(kind, capsys):
    """The 1e-12 of this file passes a contracted product or another summation order; tw.LD_BOUND (derived in
    tw.interp_ld) does not leave that room.  Q = 8 on the two-chunk shape, every reuse pattern's components."""
    S, W, T = tw.EDGE_SHAPES[0]
    cols, axes = tw.packed(kind, 8)
    x = tw.chain7(kind, S, W, T)
    worst = 0.0
    for comps in tw.COMP_PATTERNS[:3]:
        got, _ = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
        ref, cmax = tw.derive_ld(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        assert np.isfinite(got).mean() > 0.5 and np.isnan(got).mean() > 0.05
        worst = max(worst, tw.ld_ratio(got, ref, cmax))
    with capsys.disabled():
        print("\ntwin against long double, %s, Q = 8: worst %.2f units of 2^-52 cmax (bound %d)" % (kind, worst, tw.LD_BOUND))
    assert worst <= tw.LD_BOUND


def test_search_fixtures_hold_what_they_say():
    for axis, n in [(2, n) for n in (2, 3, 5, 16, 17, 65)] + [(0, 2), (0, 7), (1, 2), (1, 3)]:
        cols, axes = tw.search_table(axis, n)
        x, want = tw.search_samples(axis, n)
        got = tw.interp(cols, axes, *x)[:, 0]
        node = want >= 0
        assert node.sum() == n and want[n - 1] == n - 1
        np.testing.assert_array_equal(got[node], want[node])
        assert np.isnan(got[np.isnan(want)]).all() and np.isnan(want).sum() == 2
        np.testing.assert_array_equal(got[want == -1][:n - 1], np.arange(n - 1) + 0.5)       # t = 0.5 at a midpoint
        assert np.isfinite(got[want == -1]).all()


def test_bracket_rules():
    ax = np.array([1.0, 2.0, 4.0, 8.0])
    i, t = tw.bracket(ax, np.array([1.0, 1.5, 2.0, 3.0, 8.0, np.nan]))
    np.testing.assert_array_equal(i, [0, 0, 1, 1, 2, 0])
    np.testing.assert_array_equal(t[:5], [0.0, 0.5, 0.0, 0.5, 1.0])
