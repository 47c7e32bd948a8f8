"""isochrones_amd/populations.py without a device: the evaluation goes to iso_population_eval_host and the EEP estimate to
the C oracle's interp_eep (tests/_population_twin.host_backend).  Seeding, exact_N and its cap, the distributions, and the
reference's own four population tests (isochrones/tests/test_populations.py) on the small synthetic tables."""
import numpy as np
import pandas as pd
import pytest
from scipy.stats import uniform

import isochrones_amd as ia
from isochrones_amd import populations as pp
from isochrones_amd.priors import AVPrior, FlatPrior
from isochrones_amd.utils import addmags
from tests import _population_twin as tw

#: ages the small track table has (its age column ends near log10 age = 8.6)
SFH = pp.StarFormationHistory(uniform(0.1, 0.25))


def _population(imf=FlatPrior((0.5, 1.0)), **kw):
    kw = dict(dict(sfh=SFH, feh=FlatPrior((-0.9, 0.4)), distance=FlatPrior((50.0, 500.0)), AV=AVPrior((0.0, 1.0))), **kw)
    pop = pp.StarPopulation(tw.small_ic(), imf=imf, **kw)
    pop._backend = tw.host_backend()
    return pop


@pytest.fixture(scope="module")
def on_grid():
    """A population that stays on the model and the BC grid, its frame of 400 and the dereddened frame."""
    pop = _population()
    df = pop.generate(400, seed=11)
    return pop, df, pp.deredden(df)


def test_exports_and_column_order():
    for name in ("StarPopulation", "BinaryDistribution", "StarFormationHistory", "StarFormationHistoryGrid", "deredden",
                 "evaluate_binaries"):
        assert getattr(ia, name) is getattr(pp, name)
    assert ia.populations is pp
    names = pp.column_names(["mass", "Teff"], ["J", "K"])
    one = ["mass", "Teff", "J_mag", "K_mag", "distance", "AV", "initial_feh", "requested_age", "A_J", "A_K"]
    assert names == [c + "_0" for c in one] + [c + "_1" for c in one] + ["J_mag", "A_J", "K_mag", "A_K"]


def test_same_seed_same_frame(on_grid):
    pop, df, _ = on_grid
    again = pop.generate(400, seed=11)
    pd.testing.assert_frame_equal(df, again, check_exact=True)
    assert not pop.generate(400, seed=12).equals(df)
    ic = tw.small_ic()
    assert list(df.columns) == pp.column_names(list(ic.model_grid.interp.columns), list(ic.bands))
    # filled even where the secondary is absent, as the reference
    single = df.mass_1.isnull()
    assert single.any() and not df.loc[single, ["distance_1", "AV_1", "initial_feh_1", "requested_age_1"]].isnull().any().any()
    assert df.loc[single, "V_mag_1"].isnull().all()


def test_exact_n_redraws_until_every_primary_is_on_the_grid():
    pop = _population(imf=FlatPrior((0.15, 1.0)))                # the mass axis starts at 0.3: at least one draw in six is off
    loose = pop.generate(300, seed=3, exact_N=False)
    assert 100 < len(loose) < 270 and not loose.mass_0.isnull().any()
    assert list(loose.index) == list(range(len(loose)))
    df = pop.generate(300, seed=3)
    assert len(df) == 300 and not df.mass_0.isnull().any()
    one = pop.generate(1, seed=5)                                # the corner case of the reference's test_generate
    assert len(one) == 1 and not one.mass_0.isnull().any()


def test_redraw_cap_raises():
    pop = _population(imf=FlatPrior((0.1, 0.2)))                 # entirely below the mass axis
    with pytest.raises(RuntimeError, match="still off the model grid after 100 rounds"):
        pop.generate(3, seed=1)
    assert len(pop.generate(3, seed=1, exact_N=False)) == 0


def test_single_fraction_and_mass_ratios():
    n, fB = 4000, 0.4
    m, s = pp.BinaryDistribution(FlatPrior((0.5, 1.0)), fB=fB).sample(n, np.random.default_rng(2))
    singles = int((s == 0).sum())
    assert abs(singles - n * (1 - fB)) < 5 * np.sqrt(n * fB * (1 - fB)), singles
    q = s[s > 0] / m[s > 0]
    assert q.min() >= 0.2 and q.max() <= 1.0 and ((m >= 0.5) & (m <= 1.0)).all()
    m2, s2 = pp.BinaryDistribution(FlatPrior((0.5, 1.0)), fB=fB).sample(n, np.random.default_rng(2))
    assert np.array_equal(m, m2) and np.array_equal(s, s2)


def test_star_formation_histories():
    t = np.array([0.5, 2.0, 7.0])
    ages = pp.StarFormationHistoryGrid(t, np.array([1.0, 0.0, 3.0])).sample_ages(500, np.random.default_rng(1))
    assert set(np.unique(ages)) == set(np.log10(1e9 * t[[0, 2]]))
    assert abs((ages == np.log10(7e9)).mean() - 0.75) < 5 * np.sqrt(0.75 * 0.25 / 500)
    a = pp.StarFormationHistory().sample_ages(500, np.random.default_rng(1))
    assert a.min() > 6.0 and a.max() <= 10.0
    assert np.array_equal(a, pp.StarFormationHistory().sample_ages(500, np.random.default_rng(1)))


def test_props_and_bands_subsets():
    pop = _population()
    df = pop.generate(50, seed=4, props=["mass", "radius"], bands=["K", "V"])
    assert list(df.columns) == pp.column_names(["mass", "radius"], ["K", "V"])
    full = pop.generate(50, seed=4)
    for c in df.columns:
        assert np.array_equal(df[c].values, full[c].values, equal_nan=True), c
    with pytest.raises(ValueError, match="props must include 'mass'"):
        pop.generate(5, seed=4, props=["radius"])
    with pytest.raises(ValueError, match="no band"):
        pop.generate(5, seed=4, bands=["nope"])
    with pytest.raises(TypeError):
        pop.generate(5, seed=4, nonsense=1)


# ---- the reference's tests ----------------------------------------------------------------------------------------------

def test_old_deredden(on_grid):
    """deredden() equals regenerating the population at AV = 0."""
    pop, df, dered = on_grid
    regen = pp._evaluate(pop.ic, df["initial_mass_0"].values, df["initial_mass_1"].values, df["requested_age_0"].values,
                         df["initial_feh_0"].values, df["distance_0"].values, 0.0, None, "all", False, None,
                         pop._backend).frame()
    assert list(regen.columns) == list(dered.columns)
    a, b = dered.fillna(0), regen.fillna(0)
    for c in a.columns:
        ok, dev = tw.close(a[c].values, b[c].values)
        assert ok, (c, dev)


def test_mags(on_grid):
    """No total magnitude is null."""
    pop, df, _ = on_grid
    mags = ["%s_mag" % b for b in pop.ic.bands]
    assert len(df) == 400 and df[mags].isnull().sum().sum() == 0
    assert (df.mass_1 > 0).sum() > 50


def test_dereddening(on_grid):
    pop, df, dered = on_grid
    cols = ["initial_mass_0", "initial_feh_0", "requested_age_0"]
    pd.testing.assert_frame_equal(df[cols], dered[cols])
    assert (dered.AV_0 == 0).all() and (dered.AV_1 == 0).all() and (df.AV_0 > 0).any()
    for b in pop.ic.bands:
        diff = (dered["%s_mag" % b] + df["A_%s_0" % b]) - df["%s_mag" % b]
        is_binary = df.mass_1 > 0
        assert diff.loc[~is_binary].std() < 0.0001
        assert (dered["A_%s" % b] == 0).all()


def test_extinction(on_grid):
    _, df, dered = on_grid
    want = addmags(dered["G_mag_0"] + df["A_G_0"], (dered["G_mag_1"] + df["A_G_1"]).fillna(np.inf))
    np.testing.assert_array_almost_equal(df["G_mag"], want)


def test_deredden_takes_the_dict_too(on_grid):
    _, df, dered = on_grid
    d = pp.deredden({c: df[c].values for c in df.columns})
    assert list(d) == list(df.columns)
    for c in df.columns:
        assert np.array_equal(d[c], dered[c].values, equal_nan=True), c
