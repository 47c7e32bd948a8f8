"""k_solve_last_axis (libiso_solve.so) where tests/test_gpu_solve.py does not reach: ragged finite ranges whose F and L come
from different columns, empty and one-knot intersections, holes (NaN and +inf) next to F and L and outside the
intersection, plateaus, the bracket search at every small axis length and one ulp around every node, the launch tail,
the host entry point at the row count where Python switches paths, and special values.

Every comparison is tests/_solve_gpu.same against the numpy twin (tests/_solve_twin.py): NaN at the same positions,
every other value the same 64 bits.  The header fixes every float64 operation and its order and the library is built
without contraction, so the device and the twin have no rounding to differ by.  tests/test_solve_cases_cpu.py proves
on the CPU that the query sets used here reach every branch."""
import numpy as np
import pytest
import torch

from isochrones_amd.interp import HOST_CALL_ROWS
from tests import _solve_cases as K
from tests import _solve_tables as G
from tests import _solve_twin as T
from tests._solve_gpu import device, host, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,holes", [(s, 0) for s in G.SHAPES] + [(s, 1) for s in G.HOLE_SHAPES])
def test_bit_identity_on_ragged_tables(shape, holes):
    col, axes, x0, x1, y, want = G.ragged_case(shape, G.n_holes(shape) if holes else 0)
    got = device(col, axes, x0, x1, y)
    print("%r holes %d: %d queries, %d solved" % (shape, holes, x0.size, np.isfinite(want[0]).sum()))
    assert same(got, want[0], (col, axes, x0, x1, y))
    assert same(host(col, axes, x0, x1, y), got, (col, axes, x0, x1, y))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n", G.BRACKET_LENGTHS)
def test_bracket_every_axis_length(which, n):
    col, axes, x0, x1, y, want = G.bracket_case(which, n)
    assert same(device(col, axes, x0, x1, y), want[0], (col, axes, x0, x1, y))


def test_launch_tails_and_guards():
    """n on each side of one and two 256-lane workgroups: every prefix of the query set gives the prefix of the
    result, and nothing is written behind out (asserted by the harness), on the current and on a side stream."""
    col, axes, x0, x1, y, want = G.ragged_case((4, 3, 9), 0)
    pick = np.random.default_rng(5).permutation(x0.size)[:513]   # mixed: a lane past n would not read its neighbour's kind
    x0, x1, y, e = x0[pick], x1[pick], y[pick], want[0][pick]
    full = device(col, axes, x0, x1, y)
    assert same(full, e, (col, axes, x0, x1, y))
    assert np.isfinite(e).sum() > 100 and np.isnan(e).sum() > 100
    side = torch.cuda.Stream()
    for n in (1, 2, 255, 256, 257, 511, 513):
        for stream in (None, side):
            assert same(device(col, axes, x0[:n], x1[:n], y[:n], stream=stream), full[:n], (col, axes, x0, x1, y))


def test_host_entry_point_at_the_switch():
    """Python sends host arrays of up to HOST_CALL_ROWS rows through iso_solve_last_axis_host and longer ones through
    the device path: both sides of the switch agree bit for bit, with each other, the device-tensor call and the twin."""
    from tests.test_gpu_solve import _hand_ic, _triple
    grid, axes = K.table(K.PLATEAU, ((1, 1, 3, np.nan), (2, 0, 5, np.nan), (0, 2, 0, np.nan)))
    ic = _hand_ic("track", K.PLATEAU, ((1, 1, 3, np.nan), (2, 0, 5, np.nan), (0, 2, 0, np.nan)))
    rng = np.random.default_rng(6)
    n = HOST_CALL_ROWS + 1
    x0, x1 = rng.uniform(-0.05, 2.05, n), rng.uniform(9.5, 40.5, n)
    x0[:60], x1[30:90] = rng.choice(axes[0], 60), rng.choice(axes[1], 60)
    y = rng.uniform(0.8, 5.7, n)
    y[:200] = np.round(y[:200] * 4) / 4                       # values the table holds: knot hits and plateaus
    want = T.solve(grid, axes, 0, x0, x1, y)[0]
    assert np.isfinite(want).sum() > n // 4 and np.isnan(want).sum() > n // 10
    case = (grid[..., 0], axes, x0, x1, y)
    for rows in (HOST_CALL_ROWS - 1, HOST_CALL_ROWS, HOST_CALL_ROWS + 1):
        got = ic.solve_eep(*_triple("track", x0[:rows], x1[:rows], y[:rows]))
        assert isinstance(got, np.ndarray) and got.shape == (rows,)
        assert same(got, want[:rows], case)
    t = [torch.as_tensor(v, device="cuda") for v in _triple("track", x0, x1, y)]
    assert same(ic.solve_eep(*t).cpu().numpy(), want, case)
    for rows in (1, HOST_CALL_ROWS):                          # the entry point itself
        assert same(host(grid[..., 0], axes, x0[:rows], x1[:rows], y[:rows]), want[:rows], case)


@pytest.mark.parametrize("kind", ["zero", "inf_pad", "inf_inside"])
def test_special_values(kind):
    col, axes, x0, x1, y, tags, want = G.special_case(kind)
    got = device(col, axes, x0, x1, y)
    assert same(got, want[0], (col, axes, x0, x1, y))
    assert same(host(col, axes, x0, x1, y), got, (col, axes, x0, x1, y))
    tags = np.array(tags)
    # by hand: an infinite or NaN coordinate is off its axis, no g reaches +inf, and g(F) > -inf is no hit
    for name in ("nan", "+inf", "-inf"):
        for what in ("x0", "x1", "target"):
            m = tags == "%s %s" % (name, what)
            assert m.sum() >= 4 and np.isnan(got[m]).all(), (name, what)
    for name in ("below x0", "above x0", "below x1", "above x1"):     # one ulp outside the axis
        assert np.isnan(got[tags == name]).all(), name
    assert np.isfinite(got[tags == "plain"]).sum() >= 4
    for d in (0, 1):                                          # -0.0 is the node at 0.0
        plus, minus = got[tags == "+0.0 x%d" % d], got[tags == "-0.0 x%d" % d]
        assert np.isfinite(plus).sum() >= 4
        assert same(minus, plus)
