"""Star-cluster model on the host: the numpy restatement (tests/_cluster_ref.py) against the reference's own numbers in
tests/golden/cluster/, and the host logic of StarClusterModel (bounds, mnest_prior, set_prior, priors, refusals)."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import priors as P

from . import _cluster_ref as R


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_matches_the_reference(case):
    fx = R.load(case)
    meta = fx["meta"]
    mag, unc, prop, punc = R.star_arrays(fx)
    lo, hi = meta["mass_bounds"]
    checked = 0
    for i, p in enumerate(fx["pars"]):
        if fx["undefined"][i]:
            continue
        n = int(fx["col_n"][i])
        like = R.like_per_star(fx["col_eep"][i, :n], fx["col_mass"][i, :n], fx["col_lndm"][i, :n], fx["col_mags"][i, :n],
                               fx["col_props"][i, :n], mag, unc, prop, punc, p[4], p[5], p[6], lo, hi, fx["minq"][i])
        want = fx["like_tot"][i]
        assert np.array_equal(np.isnan(like), np.isnan(want)) and np.array_equal(like == 0, want == 0), (case, i)
        ok = np.isfinite(want) & (want != 0)
        np.testing.assert_allclose(like[ok], want[ok], rtol=1e-12, atol=0, err_msg="%s row %d" % (case, i))
        got = R.lnlike_from_likes(like)
        ref = fx["lnlike"][i]
        if np.isfinite(ref):
            assert abs(got - ref) <= 1e-12 * abs(ref), (case, i, got, ref)
        else:
            assert (np.isnan(got) and np.isnan(ref)) or got == ref, (case, i, got, ref)
        checked += 1
    assert checked >= 15
    assert np.isfinite(fx["lnlike"]).sum() >= 10


def test_fixtures_cover_the_asked_cases():
    holes = R.load("cluster_holes_phot6")
    gaps = [np.diff(holes["col_eep"][i, :n]).max() for i, n in enumerate(holes["col_n"]) if n > 1]
    assert max(gaps) > 1                                  # non-contiguous EEP sets
    assert len(holes["meta"]["bands"]) >= 5
    assert R.load("cluster_props")["meta"]["props"] == ["parallax", "Teff"]
    for case in R.CASES:
        fx = R.load(case)
        assert len(fx["pars"]) >= 20 and (fx["minq"] > 0.1).sum() >= 3 and fx["undefined"].any()


@pytest.mark.parametrize("case", R.CASES)
def test_lnprior_matches_the_reference(case):
    fx = R.load(case)
    mod = R.make_model(fx, 0.1)
    got = mod.lnprior(fx["pars"])
    want = fx["lnprior"]
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * (1 + np.abs(want[fin])))
    for i in range(3):                                    # the scalar form
        assert mod.lnprior(fx["pars"][i]) == pytest.approx(want[i], rel=1e-12)


def _model():
    return R.make_model(R.load("cluster_jhk"), 0.1)


def test_parameter_order_and_surface():
    mod = _model()
    assert mod.param_names == ("age", "feh", "distance", "AV", "alpha", "gamma", "fB")
    assert mod.n_params == 7 and mod.bands == ("J", "H", "K") and mod.props == ()
    assert mod.labelstring == "cluster"
    mod.name = "m67"
    assert mod.labelstring == "cluster_m67"
    assert mod.bounds("eep") == (151, 196)


def test_bounds_fallbacks_and_mnest_box():
    mod = _model()
    ic = mod.ic
    assert mod.bounds("feh") == (ic.minfeh, ic.maxfeh)          # FehPrior: (-inf, inf)
    assert mod.bounds("gamma") == (0.0, 1.0)                    # GaussianPrior: unbounded
    assert mod.bounds("age") == (6.0, 10.15)
    assert mod.bounds("distance") == (0.0, 50000.0)
    assert mod.bounds("fB") == (0.0, 0.6)
    assert mod.bounds("mass") == (0.1, 300.0)
    cube = np.array([0.0, 1.0, 0.5, 0.25, 0.5, 0.5, 1.0])
    mod.mnest_prior(cube, 7, 7)
    np.testing.assert_allclose(cube, [6.0, ic.maxfeh, 25000.0, 0.25, -2.5, 0.5, 0.6])
    assert all(np.isfinite(mod.bounds(p)).all() for p in mod.param_names)


def test_set_prior_with_a_prior_subclass():
    class Triangle(P.Prior):
        bounded = 1

        def __init__(self):
            self._bounds = (0.0, 1.0)

        def _raw(self, x):
            return 2.0 * x

    mod = _model()
    x = np.array([9.0, -0.1, 400.0, 0.1, -2.5, 0.3, 0.25])
    base = mod.lnprior(x)
    mod.set_prior(fB=Triangle())
    assert mod.lnprior(x) == pytest.approx(base - np.log(1 / 0.6) + np.log(0.5), rel=1e-12)
    x2 = x.copy()
    x2[6] = 1.5
    assert mod.lnprior(x2) == -np.inf
    mod.set_prior(gamma=P.GaussianPrior(0.3, 0.1, bounds=(0.0, 0.9)))
    assert mod.bounds("gamma") == (0.0, 0.9)
    with pytest.raises(ValueError):
        mod.set_prior(mass=P.FlatPrior((0, 1)))


def test_refusals():
    fx = R.load("cluster_jhk")
    track = ia.synthetic_track(bands=("J", "H", "K"), fehs=np.array([-0.5, 0.0]), masses=np.array([0.8, 1.0, 1.2]),
                               eeps=np.arange(300.0, 320.0))
    with pytest.raises(ValueError, match="isochrone"):
        ia.StarClusterModel(track, R.catalog_frame(fx))
    mod = _model()
    with pytest.raises(NotImplementedError, match="Must provide p0"):
        mod.emcee_p0(10)
    with pytest.raises(NotImplementedError, match="Must provide p0"):
        mod.fit_mcmc(nwalkers=16)
