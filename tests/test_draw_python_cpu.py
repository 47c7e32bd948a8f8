"""The Python layer over libiso_draw.so without a device: StarPopulation.generate(rng="philox"), InjectionSet.draw(rng="philox")
and PopulationModel.sample go through iso_draw_systems_host (the evaluation through the host backend of
tests/_population_twin.py)."""
import numpy as np
import pandas as pd
import pytest
from scipy.stats import beta, norm, uniform

import isochrones_amd as ia
from isochrones_amd import draws, populations as pp, priors as P, selection
from isochrones_amd.csrc.libraries import BINNED, DRAW, HIER, POPULATION, RELATION, SELECT
from tests import _population_twin as tw

SFH = pp.StarFormationHistory(uniform(0.1, 0.25))


@pytest.fixture(scope="module", autouse=True)
def built():
    for spec in (DRAW, POPULATION, HIER, SELECT, RELATION, BINNED):
        spec.build()


def _population(imf=P.FlatPrior((0.5, 1.0)), **kw):
    kw = dict(dict(sfh=SFH, feh=P.FlatPrior((-0.9, 0.4)), distance=P.FlatPrior((50.0, 500.0)), AV=P.AVPrior((0.0, 1.0))), **kw)
    pop = pp.StarPopulation(tw.small_ic(), imf=imf, **kw)
    pop._backend = tw.host_backend()
    return pop


def test_exports():
    assert ia.DrawPlan is draws.DrawPlan and ia.draws is draws


def test_generate_philox_frames():
    pop = _population()
    df = pop.generate(200, rng="philox", seed=3)
    ic = tw.small_ic()
    assert list(df.columns) == pp.column_names(list(ic.model_grid.interp.columns), list(ic.bands)) and len(df) == 200
    pd.testing.assert_frame_equal(df, pop.generate(200, rng="philox", seed=3), check_exact=True)      # the same frame twice
    assert not pop.generate(200, rng="philox", seed=4).equals(df)
    pd.testing.assert_frame_equal(df.iloc[:50].reset_index(drop=True), pop.generate(50, rng="philox", seed=3), check_exact=True)
    assert not df.mass_0.isnull().any()
    assert not pop.draw_plan().host_columns
    assert df.requested_age_0.between(8.0, np.log10(0.35e9)).all() and df.distance_0.between(50.0, 500.0).all()
    # the numpy path is the default and is not the Philox one
    assert not pop.generate(200, seed=3).equals(df)
    with pytest.raises(ValueError, match="rng is"):
        pop.generate(5, rng="mt19937")
    with pytest.raises(TypeError):
        pop.generate(5, rng="philox", nonsense=1)


def test_generate_philox_exact_n():
    pop = _population(imf=P.FlatPrior((0.15, 1.0)))              # the mass axis starts at 0.3: at least one draw in six is off
    loose = pop.generate(300, rng="philox", seed=3, exact_N=False)
    assert 100 < len(loose) < 270 and not loose.mass_0.isnull().any()
    df = pop.generate(300, rng="philox", seed=3)
    assert len(df) == 300 and not df.mass_0.isnull().any()
    # exactly the systems off the grid were redrawn: the others are the first round's, and system j does not depend on N
    first = pop.draw_plan().draw(300, 3)
    same = df.initial_feh_0.values == first["feh"]                # (the frame's initial_feh is the draw itself)
    assert same.sum() == len(loose) and np.array_equal(df.initial_feh_0.values[same], loose.initial_feh_0.values)
    assert np.array_equal(df.mass_0.values[same], loose.mass_0.values)
    assert np.all(same[first["mass"] < 0.3] == False)            # noqa: E712  (below the mass axis: redrawn)
    pd.testing.assert_frame_equal(df.iloc[:120].reset_index(drop=True), pop.generate(120, rng="philox", seed=3), check_exact=True)
    pop = _population(imf=P.FlatPrior((0.1, 0.2)))               # entirely below the mass axis
    with pytest.raises(RuntimeError, match="still off the model grid after 100 rounds"):
        pop.generate(3, rng="philox", seed=1)
    assert len(pop.generate(3, rng="philox", seed=1, exact_N=False)) == 0


def test_single_fraction():
    n, fB = 4000, 0.4
    pop = _population(fB=fB)
    d = pop.draw_plan().draw(n, 2)
    singles = int((d["binary"] >= fB).sum())
    assert abs(singles - n * (1 - fB)) < 5 * np.sqrt(n * fB * (1 - fB)), singles
    # the frame keeps the systems on the grid, in order; a companion is there only where the uniform fell below fB (one
    # below the mass axis is off the grid and shows as absent)
    df = pop.generate(n, rng="philox", seed=2, exact_N=False)
    rows = np.flatnonzero(np.isin(d["feh"], df.initial_feh_0.values))
    assert len(rows) == len(df) > n // 3 and np.array_equal(d["feh"][rows], df.initial_feh_0.values)
    has = df.mass_1.notnull().values
    assert np.all(d["binary"][rows][has] < fB) and has.sum() > 0.2 * len(df) * fB
    q = df.mass_1.values[has] / df.mass_0.values[has]
    assert q.min() >= 0.2 and q.max() <= 1.0 + 1e-9


def test_host_columns():
    pop = _population(sfh=pp.StarFormationHistory(norm(0.2, 0.02)))
    plan = pop.draw_plan()
    assert plan.host_columns == ("age",) and "age" not in plan.device_columns and len(plan.device_columns) == 6
    df = pop.generate(100, rng="philox", seed=1)
    assert len(df) == 100 and df.requested_age_0.between(7.9, 8.6).all()
    grid = _population(sfh=pp.StarFormationHistoryGrid(np.array([0.15, 0.3]), np.array([1.0, 1.0]))).draw_plan()
    assert grid.host_columns == ("age",)
    # the other columns keep their streams: the same masses with and without a host column
    assert np.array_equal(plan.draw(50, 1)["mass"], _population().draw_plan().draw(50, 1)["mass"])


def test_host_columns_are_fresh_in_every_redraw_round():
    """A host column (here the IMF, a frozen scipy distribution) with a good part of its draws off the grid: every round of
    redrawing has its own host values, so the frame fills for every seed, a redrawn row is no copy of one of the first rows,
    and the numbers are as distinct as independent draws are."""
    # masses flat on (0.15, 1.0), the mass axis starts at 0.3 (a scipy uniform would be read as a star-formation history)
    pop = _population(imf=beta(1, 1, loc=0.15, scale=0.85))
    plan = pop.draw_plan()
    assert plan.host_columns == ("mass",)
    assert not np.array_equal(plan.draw(40, 3)["mass"], plan.draw(40, 3, round=1)["mass"])
    assert np.array_equal(plan.draw(40, 3, round=1)["mass"], plan.draw(40, 3, round=1)["mass"])
    for seed in range(8):
        first = plan.draw(300, seed)["mass"]
        df = pop.generate(300, rng="philox", seed=seed)              # (seed 3's first host draw is off the grid)
        assert len(df) == 300 and not df.mass_0.isnull().any()
        assert df.mass_0.nunique() == 300
        redrawn = np.flatnonzero(first < 0.3)
        assert redrawn.size > 20
        # the k systems redrawn in round 1 did not get the host values of the systems 0 .. k - 1 again
        again = df.initial_mass_0.values[redrawn]
        assert not np.any(np.isclose(again[:, None], first[None, :redrawn.size], rtol=0, atol=1e-6))
        pd.testing.assert_frame_equal(df, pop.generate(300, rng="philox", seed=seed), check_exact=True)


def test_injection_set_philox_against_numpy(monkeypatch):
    ic = tw.small_ic()
    monkeypatch.setattr(selection.InjectionSet, "_backend", tw.host_backend())
    draw = {"mass": P.FlatPrior((0.5, 1.0)), "age": P.FlatLogPrior((8.0, 8.5)), "feh": P.FlatPrior((-0.9, 0.4))}
    J = 20000
    limits = {"V": (6.5, 0.3)}
    a = selection.InjectionSet.draw(ic, draw, J, limits, seed=5, accurate=False, rng="philox")
    b = selection.InjectionSet.draw(ic, draw, J, limits, seed=5, accurate=False)
    assert a.J == b.J == J and set(a.columns) == set(draw) and not np.array_equal(a.columns["mass"], b.columns["mass"])
    again = selection.InjectionSet.draw(ic, draw, J, limits, seed=5, accurate=False, rng="philox")
    assert all(np.array_equal(a.columns[c], again.columns[c]) for c in draw) and np.array_equal(a.lnd, again.lnd)
    model = ia.PopulationModel(mass=ia.TruncatedGaussian((0.5, 1.0), mean=(0.5, 1.0), sigma=(0.05, 0.5)))
    theta = np.array([[0.6, 0.1], [0.75, 0.15], [0.9, 0.1], [0.7, 0.4]])
    la_a, ne_a, _ = selection.Selection(a, model, None).alpha(theta)
    la_b, ne_b, _ = selection.Selection(b, model, None).alpha(theta)
    se = np.sqrt((1.0 / ne_a - 1.0 / J) + (1.0 / ne_b - 1.0 / J))
    z = (la_a - la_b) / se
    print("ln alpha, Philox against numpy draws: %s standard errors; n_eff %.0f .. %.0f" % (np.round(z, 2), ne_a.min(), ne_a.max()))
    assert np.all(np.isfinite(la_a)) and np.all(np.abs(z) <= 5.0)
    assert 0.02 < np.exp(la_a).min() and np.exp(la_a).max() < 0.98          # the cut bites


def test_population_model_sample_linear_gaussian():
    model = ia.PopulationModel(age=ia.Fixed(P.FlatPrior((8.0, 10.0))),
                               feh=ia.LinearGaussian("age", (-6.0, 6.0), slope=(-2.0, 2.0), sigma=(0.05, 1.0), pivot=9.0),
                               mass=ia.PowerLaw((0.1, 10.0)))
    assert model.param_names == ("feh.intercept", "feh.slope", "feh.sigma", "mass.alpha")
    n, slope, sigma = 20000, -0.35, 0.3
    out = model.sample([0.1, slope, sigma, -2.35], n, seed=7)
    assert set(out) == {"age", "feh", "mass"} and all(v.shape == (n,) for v in out.values())
    x, y = out["age"] - 9.0, out["feh"]
    fit = np.polyfit(x, y, 1)
    se = sigma / (np.sqrt(n) * x.std())
    print("least-squares slope %.4f against %.4f: %.2f standard errors" % (fit[0], slope, (fit[0] - slope) / se))
    assert abs(fit[0] - slope) <= 5 * se and abs(fit[1] - 0.1) <= 5 * sigma / np.sqrt(n)
    assert out["mass"].min() >= 0.1 and out["mass"].max() <= 10.0
    assert np.array_equal(model.sample([0.1, slope, sigma, -2.35], 100, seed=7)["feh"], y[:100])
    with pytest.raises(ValueError, match="one row"):
        model.sample([0.1, slope], 10)


def test_population_model_sample_histograms():
    age_e, feh_e = np.array([8.0, 9.0, 9.5, 10.0]), np.array([-1.0, -0.5, 0.0, 0.25, 0.5])
    model = ia.PopulationModel(age=ia.Histogram(age_e), feh=ia.Histogram(feh_e, given="age"), mass=ia.Fixed(P.SalpeterPrior()))
    rng = np.random.default_rng(4)
    theta = rng.uniform(-1.5, 1.5, model.n_params)
    n = 60000
    out = model.sample(theta, n, seed=11)
    ct = model.cell_table(theta[None, :])
    mass = np.exp(ct["lnh"][0]).reshape(3, 4) * np.diff(age_e)[:, None] * np.diff(feh_e)[None, :]
    assert mass.sum() == pytest.approx(1.0, abs=1e-12)
    counts = np.histogram2d(out["age"], out["feh"], bins=[age_e, feh_e])[0]
    assert counts.sum() == n
    z = (counts - n * mass) / np.sqrt(n * mass * (1 - mass))
    print("cell masses of a sampled Histogram(given=): worst %.2f binomial standard errors" % np.abs(z).max())
    assert np.all(np.abs(z) <= 5.0)
    # without given: one histogram alone
    one = ia.PopulationModel(age=ia.Histogram(age_e))
    th = np.array([0.7, -0.4])
    x = one.sample(th, n, seed=3)["age"]
    m1 = np.exp(one.cell_table(th[None, :])["lnh"][0]) * np.diff(age_e)
    c1 = np.histogram(x, bins=age_e)[0]
    assert np.all(np.abs(c1 - n * m1) <= 5 * np.sqrt(n * m1 * (1 - m1)))
