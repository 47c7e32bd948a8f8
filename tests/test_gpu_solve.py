"""The exact (mass, age, [Fe/H]) -> EEP solve on the device (libiso_solve.so through ``solve_eep``) against its numpy
twin (tests/_solve_twin.py), the reference's own get_eep_accurate (tests/golden/solve/) and the package's own
interpolator, in every call form."""
import functools

import numpy as np
import pytest
import torch

import isochrones_amd as ia
from isochrones_amd.interp import DFInterpolator
from isochrones_amd.models import (EvolutionTrackGrid, EvolutionTrackInterpolator, IsochroneGrid, IsochroneInterpolator,
                                   _bc)
from tests import _solve_cases as K
from tests import _solve_twin as T
from tests._solve_gpu import same

pytestmark = pytest.mark.gpu

BANDS = ("J", "H", "K")


@functools.lru_cache(maxsize=None)
def _full(kind):
    """The MIST-shaped synthetic interpolator of one parametrisation, built once for the module."""
    return ia.synthetic_track(bands=BANDS) if kind == "track" else ia.synthetic_isochrone(bands=BANDS)


def _ic(kind, grid, axes, columns):
    """An interpolator of either parametrisation over a given table (a one-band synthetic BC table beside it)."""
    names = ["initial_feh", "initial_mass", "EEP"] if kind == "track" else ["log10_isochrone_age_yr", "feh", "EEP"]
    dfi = DFInterpolator.from_arrays(grid, axes, list(columns), names)
    if kind == "track":
        return EvolutionTrackInterpolator(EvolutionTrackGrid(dfi), _bc(("J",)), bands=("J",))
    return IsochroneInterpolator(IsochroneGrid(dfi), _bc(("J",)), bands=("J",))


def _hand_ic(kind, profile, edits):
    """A hand-built one-column table of tests/_solve_cases.py dressed as a model table: the column the solve inverts
    holds it, the columns the interpolator insists on are zeros."""
    g1, axes = K.table(profile, edits)
    cols = ["age" if kind == "track" else "initial_mass", "Teff", "logg", "feh", "Mbol"]
    g = np.zeros(g1.shape[:3] + (len(cols),))
    g[..., 0] = g1[..., 0]
    return _ic(kind, g, axes, cols)


def _triple(kind, x0, x1, y):
    """(mass, age, feh) from (x0, x1, target) in the order of the table's axes."""
    return (x1, y, x0) if kind == "track" else (y, x0, x1)


def _value(ic, kind, x0, x1, e):
    name = "age" if kind == "track" else "initial_mass"
    pars = [x1, e, x0] if kind == "track" else [e, x0, x1]
    return np.asarray(ic.interp_value(pars, [name]), dtype=float).reshape(-1)


def _queries(kind, axes, n, rng):
    """Random queries over (and a little beyond) the table, NaNs, exact nodes, and targets spread over the column's
    whole span so that a good share has a solution."""
    lo0, hi0, lo1, hi1 = axes[0][0], axes[0][-1], axes[1][0], axes[1][-1]
    x0 = rng.uniform(lo0 - 0.03 * (hi0 - lo0), hi0 + 0.03 * (hi0 - lo0), n)
    if kind == "track":
        x1 = np.exp(rng.uniform(np.log(lo1 * 0.97), np.log(hi1 * 1.03), n))     # masses: log-uniform
        y = rng.uniform(4.9, 10.6, n)
    else:
        x1 = rng.uniform(lo1 - 0.03 * (hi1 - lo1), hi1 + 0.03 * (hi1 - lo1), n)
        y = np.exp(rng.uniform(np.log(0.09), np.log(12.0), n))
    x0[:50], x1[50:100], y[100:150] = np.nan, np.nan, np.nan
    x0[150:400] = rng.choice(axes[0], 250)                                       # on nodes, the last one included
    x1[300:600] = rng.choice(axes[1], 300)
    x0[600:620], x1[610:630] = hi0, hi1
    return x0, x1, y


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_device_against_the_twin_on_mist_shaped_tables(kind):
    ic = _full(kind)
    dfi = ic.model_grid.interp
    axes = dfi.index_columns
    icol = dfi.column_index["age" if kind == "track" else "initial_mass"]
    n = 100_000
    x0, x1, y = _queries(kind, axes, n, np.random.default_rng(7 if kind == "track" else 8))
    e_dev = ic.solve_eep(*_triple(kind, x0, x1, y))
    assert isinstance(e_dev, np.ndarray) and e_dev.shape == (n,)
    e_twin, g_lo, g_hi, k_star = T.solve(dfi.grid, axes, icol, x0, x1, y, nthreads=orc_threads())
    fin = np.isfinite(e_twin)
    print("%s: %d of %d queries have a solution" % (kind, fin.sum(), n))
    assert fin.sum() > n // 10
    np.testing.assert_array_equal(np.isnan(e_dev), np.isnan(e_twin))
    trip = np.abs(_value(ic, kind, x0[fin], x1[fin], e_dev[fin]) - y[fin])
    slope = T.local_slope(axes, g_lo, g_hi, k_star)[fin]
    on_knot = np.isnan(slope)                                 # an exact hit on the first knot: no segment, same knot
    np.testing.assert_array_equal(e_dev[fin][on_knot], e_twin[fin][on_knot])
    diff = (np.abs(e_dev[fin] - e_twin[fin]) * slope)[~on_knot]
    print("%s: max round trip %.3g, max |e_dev - e_twin| * slope %.3g, max |e_dev - e_twin| %.3g" % (
        kind, trip.max(), diff.max(), np.abs(e_dev[fin] - e_twin[fin]).max()))
    assert trip.max() <= 1e-10
    assert diff.max() <= 1e-10
    # the kernel performs the twin's float64 operations in the twin's order, without contraction: every bit agrees
    assert same(e_dev, e_twin, (dfi.grid[..., icol], axes, x0, x1, y))


def orc_threads():
    from oracle import oracle as orc
    return max(1, min(16, orc.max_threads()))


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_device_against_the_reference(kind):
    grid, axes, icol, x0, x1, y, e_ref, _ = K.golden(kind)
    ic = _ic(kind, grid, axes, [str(c) for c in np.load(K.GOLDEN + "/%s.npz" % kind)["columns"]])
    e = ic.solve_eep(*_triple(kind, x0, x1, y))
    conv = np.isfinite(e_ref)
    assert np.all(np.isfinite(e[conv]))
    worst = float(np.max(np.abs(e[conv] - e_ref[conv])))
    print("%s: max |e_dev - e_ref| = %.4g" % (kind, worst))
    assert worst <= K.GOLDEN_TOL[kind]


@pytest.mark.parametrize("kind", ["track", "iso"])
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_rules_on_the_device(kind, name):
    """Plateaus, the first knot, NaN / off-axis queries, a hole inside the range, the last nodes: each through both
    parametrisations, as host arrays (the host entry point) and as device tensors (the batch launch)."""
    profile, edits, queries = K.CASES[name]
    ic = _hand_ic(kind, profile, edits)
    q = np.array(queries, dtype=float)
    m, a, f = _triple(kind, q[:, 0], q[:, 1], q[:, 2])
    np.testing.assert_array_equal(ic.solve_eep(m, a, f), q[:, 3])
    t = [torch.as_tensor(v, device="cuda") for v in (m, a, f)]
    np.testing.assert_array_equal(ic.solve_eep(*t).cpu().numpy(), q[:, 3])
    for row in q:                                             # and one by one, as plain numbers
        got = ic.solve_eep(*[float(v) for v in _triple(kind, row[0], row[1], row[2])])
        assert isinstance(got, float)
        np.testing.assert_array_equal(got, row[3])


def test_call_forms_agree_bit_for_bit():
    ic = _full("track")
    rng = np.random.default_rng(3)
    n = 6000                                                  # above the host entry point's row limit
    mass, age, feh = rng.uniform(0.7, 3.0, n), rng.uniform(8.0, 9.8, n), rng.uniform(-1.0, 0.4, n)
    host = ic.solve_eep(mass, age, feh)
    assert isinstance(host, np.ndarray) and np.isfinite(host).sum() > n // 2
    small = ic.solve_eep(mass[:100], age[:100], feh[:100])    # the host entry point
    np.testing.assert_array_equal(small, host[:100])
    for i in range(5):
        one = ic.solve_eep(float(mass[i]), float(age[i]), float(feh[i]))
        assert type(one) is float
        np.testing.assert_array_equal(one, host[i])
    # broadcasting: one age and one feh for many masses; a column against a row
    np.testing.assert_array_equal(ic.solve_eep(mass[:50], 9.0, 0.1), ic.solve_eep(mass[:50], np.full(50, 9.0), np.full(50, 0.1)))
    grid2 = ic.solve_eep(mass[:4, None], np.array([8.5, 9.0, 9.5])[None, :], 0.0)
    assert grid2.shape == (12,)
    np.testing.assert_array_equal(grid2.reshape(4, 3)[2, 1], ic.solve_eep(float(mass[2]), 9.0, 0.0))
    # CUDA tensors: the result stays on the device, on a stream that is not the default one
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tm, ta, tf = (torch.as_tensor(v, device="cuda") for v in (mass, age, feh))
        out = ic.solve_eep(tm, ta, tf)
        mixed = ic.solve_eep(tm, 9.0, 0.1)
        exact = ic.get_eep(tm, ta, tf, accurate="exact")
        also = ic.get_eep(tm, ta, tf, accurate=True)         # tensors cannot go through the per-star optimiser
    assert out.is_cuda and out.dtype == torch.float64 and out.device == tm.device and out.shape == (n,)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), host)
    np.testing.assert_array_equal(exact.cpu().numpy(), host)
    np.testing.assert_array_equal(also.cpu().numpy(), host)
    np.testing.assert_array_equal(mixed.cpu().numpy(), ic.solve_eep(mass, 9.0, 0.1))
    np.testing.assert_array_equal(ic.get_eep(mass, age, feh, accurate="exact"), host)
    assert ic.get_eep(float(mass[0]), float(age[0]), float(feh[0]), accurate="exact") == host[0]
    with pytest.raises(TypeError):
        ic.get_eep(mass, age, feh, accurate="exact", xatol=1e-3)


def test_isochrone_interpolator_solves_on_its_own_grid():
    ic = _full("iso")
    rng = np.random.default_rng(4)
    n = 2000
    age, feh, eep = rng.uniform(8.0, 10.0, n), rng.uniform(-1.0, 0.4, n), rng.uniform(250.0, 600.0, n)
    mass = np.asarray(ic.interp_value([eep, age, feh], ["initial_mass"]), dtype=float).reshape(-1)
    got = ic.get_eep(mass, age, feh, accurate="exact")
    np.testing.assert_array_equal(got, ic.solve_eep(mass, age, feh))
    back = np.asarray(ic.interp_value([got, age, feh], ["initial_mass"]), dtype=float).reshape(-1)
    assert np.isfinite(got).all() and np.max(np.abs(back - mass)) <= 1e-10
    t = ic.get_eep(torch.as_tensor(mass, device="cuda"), torch.as_tensor(age, device="cuda"),
                   torch.as_tensor(feh, device="cuda"), accurate=True)
    np.testing.assert_array_equal(t.cpu().numpy(), got)


def test_generate_and_generate_binary_hit_the_requested_age():
    ic = _full("track")
    rng = np.random.default_rng(5)
    mass = rng.uniform(0.6, 4.0, 300)
    df = ic.generate(mass, 9.2, -0.2, accurate="exact")
    fin = np.isfinite(df["age"].values)
    assert fin.sum() > 100
    assert np.max(np.abs(df["age"].values[fin] - df["requested_age"].values[fin])) <= 1e-10
    assert np.max(np.abs(df["eep"].values[fin] - ic.solve_eep(mass, 9.2, -0.2)[fin])) <= 1e-9
    fast = ic.generate(mass, 9.2, -0.2)                       # the default estimate misses the age by far more
    assert np.nanmax(np.abs(fast["age"].values - 9.2)) > 1e-6
    both = ic.generate_binary(mass, 0.7 * mass, 9.2, -0.2, accurate="exact")
    for comp in ("_0", "_1"):
        a, want = both["age" + comp].values, both["requested_age" + comp].values
        ok = np.isfinite(a)
        assert ok.sum() > 100 and np.max(np.abs(a[ok] - want[ok])) <= 1e-10
    iso = _full("iso")                                        # delegates to its companion track interpolator
    dfi = iso.generate(mass[:50], 9.2, -0.2, accurate="exact")
    oki = np.isfinite(dfi["age"].values)
    assert oki.sum() > 10 and np.max(np.abs(dfi["age"].values[oki] - 9.2)) <= 1e-10


def test_simulate_cluster_with_the_exact_solve():
    from isochrones_amd.cluster import simulate_cluster
    ic = _full("iso")
    cat = simulate_cluster(200, 9.1, -0.1, 500.0, 0.1, -2.5, 0.3, 0.4, bands=("J", "H", "K"), ic=ic, seed=11, accurate="exact")
    df = cat.df
    n = len(df)
    np.testing.assert_array_equal(df["eep_pri"].values, ic.solve_eep(df["mass_pri"].values, np.full(n, 9.1), np.full(n, -0.1)))
    np.testing.assert_array_equal(df["eep_sec"].values, ic.solve_eep(df["mass_sec"].values, np.full(n, 9.1), np.full(n, -0.1)))
    assert np.isfinite(df["eep_pri"].values).sum() > n // 2
    plain = simulate_cluster(200, 9.1, -0.1, 500.0, 0.1, -2.5, 0.3, 0.4, bands=("J", "H", "K"), ic=ic, seed=11).df
    np.testing.assert_array_equal(plain["mass_pri"].values, df["mass_pri"].values)
    np.testing.assert_array_equal(plain["eep_pri"].values, ic.get_eep(df["mass_pri"].values, np.full(n, 9.1), np.full(n, -0.1)))


def test_accurate_true_keeps_the_per_star_optimiser_for_host_arrays():
    ic = ia.synthetic_track(bands=("J",))
    mass, age, feh = np.array([0.9, 1.0, 1.3, 2.0]), np.array([9.5, 9.3, 9.0, 8.6]), np.array([-0.3, 0.0, 0.1, 0.2])
    got = ic.get_eep(mass, age, feh, accurate=True)
    eep0 = ic.get_eep(mass, age, feh)
    want = np.array([ic.get_eep_accurate(m, a, f, eep0=e if np.isfinite(e) else 300)
                     for m, a, f, e in zip(mass, age, feh, eep0)])
    np.testing.assert_array_equal(got, want)
    one = ic.get_eep(1.0, 9.3, 0.0, accurate=True)
    e0 = ic.get_eep(1.0, 9.3, 0.0)
    assert one == ic.get_eep_accurate(1.0, 9.3, 0.0, eep0=e0 if np.isfinite(e0) else 300)
    exact = ic.solve_eep(mass, age, feh)                      # and the optimiser lands near the exact solution
    assert np.max(np.abs(got - exact)) < 0.1


def test_device_copies_follow_the_table():
    ic = _hand_ic("track", K.RAMP, ())                        # (mass, age, feh) = (x1, target, x0)
    assert ic.solve_eep(10.0, 1.5, 0.0) == 100.5
    t0 = ic._solve_table(torch.cuda.current_device())
    assert ic._solve_table(torch.cuda.current_device()) is t0         # made once per (interpolator, device)
    dfi = ic.model_grid.interp
    dfi.add_column(np.zeros(dfi.grid.shape[:-1]), "extra")             # the table is rebuilt: so are the copies
    assert ic.solve_eep(10.0, 1.5, 0.0) == 100.5
    assert ic._solve_table(torch.cuda.current_device()) is not t0
