"""isochrones_amd.selection without a device: a host numpy chain and a host injection set go through the host entries of
libiso_hier.so and libiso_select.so.  The estimate of alpha against its closed form, the recovery of a population mean from
a truncated catalog with and without the correction, the unchanged results without an injection set, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import log_ndtr, ndtr

import isochrones_amd as ia
from isochrones_amd import _cabi, _hier_cabi as hc, priors as P
from isochrones_amd.csrc.libraries import HIER, SELECT

BOUNDS = (-6.0, 6.0)
MEANS = np.linspace(-1.2, 0.8, 41)
THETA = np.column_stack([MEANS, np.ones(41)])
SIGMA_OBS, CUT = 0.3, 0.5


@pytest.fixture(scope="module", autouse=True)
def built():
    HIER.build()
    SELECT.build()


def _model():
    return ia.PopulationModel(x=ia.TruncatedGaussian(BOUNDS, mean=(-1.2, 0.8), sigma=(0.5, 2.0)))


def _injections(J, seed):
    prior = P.FlatPrior(BOUNDS)
    x = np.asarray(prior.sample(J, np.random.default_rng(seed)), dtype=np.float64)
    return ia.InjectionSet({"x": x}, {"x": prior}, log_ndtr((CUT - x) / SIGMA_OBS))


@pytest.fixture(scope="module")
def catalog():
    """900 truths from N(0, 1) observed with sigma 0.3 and kept below 0.5; 512 posterior samples a star (32 walkers x 16
    steps) under the flat interim prior"""
    rng = np.random.default_rng(11)
    truth = rng.normal(0.0, 1.0, 900)
    obs = truth + SIGMA_OBS * rng.normal(size=900)
    obs = obs[obs < CUT]
    chain = obs[:, None, None, None] + SIGMA_OBS * rng.normal(size=(obs.size, 32, 16, 1))
    assert 550 < obs.size < 700 and np.abs(chain).max() < 6
    return chain


@pytest.fixture(scope="module")
def injections():
    return _injections(40000, 3)


@pytest.fixture(scope="module")
def posterior(catalog, injections):
    return ia.PopulationPosterior((catalog, ("x",)), None, _model(), interim={"x": P.FlatPrior(BOUNDS)}, injections=injections)


def test_alpha_against_its_closed_form(posterior, injections):
    """alpha = Phi((0.5 - mu) / hypot(1, 0.3)) (the truncation at +-6 changes it below 1e-8); every row's estimate within 5
    standard errors alpha * sqrt(1 / n_eff - 1 / J), the relative variance of a mean of weights"""
    assert ia.InjectionSet is ia.selection.InjectionSet
    la, neff = posterior.ln_alpha(THETA), posterior.selection_neff(THETA)
    assert la.shape == neff.shape == (41,) and isinstance(la, np.ndarray)
    exact = ndtr((CUT - MEANS) / math.hypot(1.0, SIGMA_OBS))
    est = np.exp(la)
    se = est * np.sqrt(1.0 / neff - 1.0 / injections.J)
    z = (est - exact) / se
    print("worst row: %.2f standard errors; n_eff %.0f .. %.0f" % (np.abs(z).max(), neff.min(), neff.max()))
    assert np.all(np.abs(z) <= 5.0)
    assert neff.min() > 5000 and neff.max() < injections.J


def test_recovery_of_the_mean_with_and_without_injections(catalog, injections, posterior):
    S = catalog.shape[0]
    plain = ia.PopulationPosterior((catalog, ("x",)), None, _model(), interim={"x": P.FlatPrior(BOUNDS)})
    with_sel, without = posterior.lnlike(THETA), plain.lnlike(THETA)
    best, biased = MEANS[np.argmax(with_sel)], MEANS[np.argmax(without)]
    print("argmax of lnlike: %.3f with injections, %.3f without" % (best, biased))
    assert abs(best) <= 0.25 and biased < -0.3
    # what lnlike is made of
    la = posterior.ln_alpha(THETA)
    assert np.array_equal(with_sel, without - S * la)
    assert np.all(posterior.selection_neff(THETA) > 4 * S)
    assert posterior.n_unmasked == S and posterior.min_neff_factor == 4.0
    # star_terms and min_ess are the uncorrected ones
    for a, b in zip(posterior.star_terms(THETA[:3]), plain.star_terms(THETA[:3])):
        assert a.tobytes() == b.tobytes()
    assert posterior.min_ess(THETA[:3]).tobytes() == plain.min_ess(THETA[:3]).tobytes()
    lp = posterior.lnpost(THETA)
    assert np.isfinite(lp).all() and np.array_equal(lp, posterior.lnprior(THETA) + with_sel)
    # a set too small for this catalog: n_eff <= 200 < 4 S, so the posterior refuses every row
    tiny = ia.PopulationPosterior((catalog, ("x",)), None, _model(), interim={"x": P.FlatPrior(BOUNDS)},
                                  injections=_injections(200, 4))
    assert np.all(tiny.selection_neff(THETA) < 4 * S) and np.isfinite(tiny.lnlike(THETA)).all()
    assert np.isneginf(tiny.lnpost(THETA)).all()
    # the same set passes a catalog of ten stars; a mask counts the unmasked ones
    mask = np.zeros(S, dtype=np.int32)
    mask[:10] = 1
    few = ia.PopulationPosterior((catalog, ("x",)), None, _model(), interim={"x": P.FlatPrior(BOUNDS)}, mask=mask,
                                 injections=_injections(200, 4))
    assert few.n_unmasked == 10 and np.isfinite(few.lnpost(THETA[10:30])).all()
    few_plain = ia.PopulationPosterior((catalog, ("x",)), None, _model(), interim={"x": P.FlatPrior(BOUNDS)}, mask=mask)
    assert np.array_equal(few.lnlike(THETA), few_plain.lnlike(THETA) - 10 * few.ln_alpha(THETA))
    # a row outside the free ranges stays -inf, and torch rows come back as tensors
    import torch
    out = posterior.lnpost(torch.tensor([[0.0, 1.0], [5.0, 1.0]], dtype=torch.float64))
    assert torch.is_tensor(out) and torch.isfinite(out[0]) and torch.isneginf(out[1])
    assert torch.is_tensor(posterior.ln_alpha(torch.from_numpy(THETA[:2])))


def test_fit_mcmc_runs_on_top(posterior):
    smp = posterior.fit_mcmc(nwalkers=16, nburn=3, niter=3, seed=2)
    df = posterior.samples
    assert np.isfinite(df["lnprob"]).all() and len(df) == 16 * 3 and smp is posterior.sampler


def test_without_injections_nothing_changes(catalog):
    """injections=None is the call path as it was: lnlike, star_terms and lnpost are the bytes of iso_hier_lnlike_host
    called directly on the same storage"""
    chain = catalog[:40]
    S, W, T = chain.shape[:3]
    model = _model()
    post = ia.PopulationPosterior((chain, ("x",)), None, model, interim={"x": P.FlatPrior(BOUNDS)}, injections=None)
    assert post.selection is None
    with pytest.raises(ValueError, match="no injection set"):
        post.ln_alpha(THETA)
    H = THETA.shape[0]
    storage = np.ascontiguousarray(chain.transpose(2, 3, 0, 1).reshape(T, 1, S * W))
    rows, interim = np.ascontiguousarray(model.pack(THETA)), ia.hierarchical.prior_record(P.FlatPrior(BOUNDS))
    ell, ess, n_bad, L, mn = np.empty((H, S)), np.empty((H, S)), np.empty(S, np.int32), np.empty(H), np.empty(H)
    p = lambda a: C.c_void_p(a.ctypes.data)
    cols = (hc.IsoHierColumn * 1)(hc.IsoHierColumn(storage.ctypes.data, 1, 0, S, 0))
    assert hc.lib().iso_hier_lnlike_host(cols, 1, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, p(interim), p(rows), H, None, p(ell),
                                         p(ess), p(n_bad), p(L), p(mn), None) == 0
    assert post.lnlike(THETA).tobytes() == L.tobytes()
    got = post.star_terms(THETA)
    assert got[0].tobytes() == ell.tobytes() and got[1].tobytes() == ess.tobytes() and got[2].tobytes() == n_bad.tobytes()
    assert post.lnpost(THETA).tobytes() == (model.lnprior(THETA) + L).tobytes()


def test_refusals(catalog):
    flat = P.FlatPrior(BOUNDS)
    x = np.linspace(-1.0, 1.0, 50)
    chain = catalog[:5]

    class Mine(P.Prior):
        bounds = BOUNDS

        def _pdf(self, x):
            return 1.0 / 12.0
    with pytest.raises(ValueError, match="evaluated on the host"):
        ia.InjectionSet({"x": x}, {"x": Mine()}, np.zeros(50))
    with pytest.raises(ValueError, match=r"lnd must be \[J\] = \[50\]"):
        ia.InjectionSet({"x": x}, {"x": flat}, np.zeros(49))
    with pytest.raises(ValueError, match="one \\[J\\] array"):
        ia.InjectionSet({"x": x, "y": x[:10]}, {"x": flat}, np.zeros(50))
    with pytest.raises(ValueError, match="not a column"):
        ia.InjectionSet({"x": x}, {"y": flat}, np.zeros(50))
    # a model column the set does not hold, or holds without its draw density
    for inj in (ia.InjectionSet({"y": x}, {"y": flat}, np.zeros(50)), ia.InjectionSet({"x": x, "y": x}, {"y": flat}, np.zeros(50))):
        with pytest.raises(ValueError, match="no column 'x' with a draw prior"):
            ia.PopulationPosterior((chain, ("x",)), None, _model(), interim={"x": flat}, injections=inj)
    with pytest.raises(TypeError, match="must be an InjectionSet"):
        ia.PopulationPosterior((chain, ("x",)), None, _model(), interim={"x": flat}, injections={"x": x})
    # a drawn column the model does not name is allowed: it follows its draw density in the population
    inj = ia.InjectionSet({"x": x, "y": x}, {"x": flat, "y": flat}, np.zeros(50))
    post = ia.PopulationPosterior((chain, ("x",)), None, _model(), interim={"x": flat}, injections=inj)
    assert np.isfinite(post.ln_alpha(THETA)).all()
