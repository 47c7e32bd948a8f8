"""The numpy twin of the exact EEP solve (tests/_solve_twin.py) against the reference's own get_eep_accurate
(tests/golden/solve/, made by tools/make_solve_golden.py), the rules of include/isochrones_amd_solve.h on hand-built
tables, and the host-side preparation of the package (isochrones_amd/solve.py: ranges, hole flags, monotonicity check)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import _solve_cases as K
from tests import _solve_twin as T


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_twin_against_the_reference(kind):
    grid, axes, icol, x0, x1, y, e_ref, resid = K.golden(kind)
    assert e_ref.size >= 300
    conv = np.isfinite(e_ref)
    assert (~conv).sum() <= 0.10 * e_ref.size
    e, g_lo, g_hi, k_star = T.solve(grid, axes, icol, x0, x1, y)
    assert np.all(np.isfinite(e[conv]))
    worst = float(np.max(np.abs(e[conv] - e_ref[conv])))
    trip = float(np.max(np.abs(orc.OracleTable(grid, axes).interp([x0, x1, e], [icol])[:, 0] - y)[np.isfinite(e)]))
    print("%s: max |e_twin - e_ref| = %.4g (recorded %.4g), round trip %.3g" % (kind, worst, K.GOLDEN_MAX_DIFF[kind], trip))
    assert K.GOLDEN_MAX_DIFF[kind] < 1e-6
    assert worst <= K.GOLDEN_TOL[kind]
    assert trip <= 1e-12
    slope = T.local_slope(axes, g_lo, g_hi, k_star)
    assert np.nanmin(slope) >= 1e-4          # the fixture's own promise


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_rules_on_hand_built_tables(name):
    profile, edits, queries = K.CASES[name]
    grid, axes = K.table(profile, edits)
    q = np.array(queries, dtype=float)
    e, _, _, _ = T.solve(grid, axes, 0, q[:, 0], q[:, 1], q[:, 2])
    np.testing.assert_array_equal(e, q[:, 3])


def test_last_node_follows_the_interpolator():
    """On the last node of ax0 the interpolator evaluates the cell below it with t = 1: g there is the node column's value
    wherever the neighbour column is finite, and NaN where the neighbour is padding."""
    profile, edits, _ = K.CASES["last_node"]
    grid, axes = K.table(profile, edits)
    tab = orc.OracleTable(grid, axes)
    g = tab.interp([np.full(6, 2.0), np.full(6, 10.0), axes[2]], [0])[:, 0]
    np.testing.assert_array_equal(g[:3], grid[2, 0, :3, 0])
    assert np.all(np.isnan(g[3:]))


def test_host_ranges_agree_with_the_twin():
    from isochrones_amd import _solve_cabi, solve
    profile, edits, _ = K.CASES["hole_inside_range"]
    grid, _ = K.table(profile, edits + ((2, 2, 0, np.nan), (0, 2, 5, np.nan)))
    grid[2, 1, :, 0] = np.nan
    r = solve.column_ranges(grid[..., 0])
    first, last = T.finite_ranges(grid[..., 0])
    assert r.dtype == np.int32 and r.shape == (3, 3, 2)
    np.testing.assert_array_equal(r[..., 0] & ~_solve_cabi.HOLE_BIT, first)
    np.testing.assert_array_equal(r[..., 1], last)
    holes = (r[..., 0] & _solve_cabi.HOLE_BIT) != 0
    want = np.zeros((3, 3), dtype=bool)
    want[1, 1] = True
    np.testing.assert_array_equal(holes, want)
    assert (first[2, 1], last[2, 1]) == (6, -1) and (first[2, 2], last[0, 2]) == (1, 4)


def test_non_monotone_column_is_refused():
    from isochrones_amd import solve
    grid, _ = K.table(K.RAMP, ((2, 1, 4, 4.0),))            # 5.75 -> 4.0 at (2, 1, 4); the step after it rises again
    with pytest.raises(ValueError) as err:
        solve.column_ranges(grid[..., 0], "age")
    msg = str(err.value)
    assert "(2, 1, 4)" in msg and "age" in msg and "get_eep_accurate" in msg and "accurate=True" in msg
    solve.column_ranges(K.table(K.PLATEAU)[0][..., 0])        # plateaus are fine


def test_solve_eep_refuses_a_non_monotone_table_before_any_device_work():
    import isochrones_amd as ia
    ic = ia.synthetic_track(bands=("J",), fehs=np.array([-0.5, 0.0, 0.5]), masses=np.array([0.8, 1.0, 1.2]),
                            eeps=np.arange(300.0, 330.0))
    dfi = ic.model_grid.interp
    dfi.grid[1, 2, 7, dfi.column_index["age"]] -= 1.0
    for _ in range(2):                                      # the refusal is kept with the table, not recomputed away
        with pytest.raises(ValueError, match=r"\(1, 2, 7\)"):
            ic.solve_eep(1.0, 9.0, 0.0)
    with pytest.raises(ValueError, match=r"\(1, 2, 7\)"):
        ic.get_eep(1.0, 9.0, 0.0, accurate="exact")
    with pytest.raises(ValueError, match="accurate must be"):
        ic.get_eep(1.0, 9.0, 0.0, accurate="fast")
