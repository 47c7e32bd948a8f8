"""InjectionSet.draw and PopulationPosterior(..., injections=) on the device, on the small synthetic track smoke() uses and
a CUDA (chain, names) source: the draw reproduces under a seed, its lnd is the stated function of the magnitudes
evaluate_binaries returns, the corrected lnlike is the uncorrected one minus S * ln_alpha, the device result matches the
host path on the downloaded chain and set, and fit_mcmc runs on top."""
import numpy as np
import pytest
from scipy.special import log_ndtr

import isochrones_amd as ia
from isochrones_amd import priors as P
from tests import _select_twin as tw

pytestmark = pytest.mark.gpu

LIMITS = {"V": (12.0, 0.2), "K": (12.5, 0.0)}
J = 2000


@pytest.fixture(scope="module")
def ic():
    return ia.synthetic_track(bands=("V", "J", "K"), fehs=np.array([-1.0, -0.5, 0.0, 0.5]),
                              masses=np.array([0.7, 0.9, 1.0, 1.1, 1.3, 2.0]), eeps=np.arange(300.0, 420.0),
                              limits=dict(mass=(0.7, 2.0), feh=(-1.0, 0.5), age=(5, 10.13)), eep_bounds=(300, 419))


def _draw_priors():
    # log10 ages that straddle the EEP range of the grid (7.1 .. 8.2 over its masses): part of the draws fall off it
    return {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "age": P.FlatPrior((7.2, 8.1)), "feh": P.FlatPrior((-1.0, 0.5)),
            "distance": P.PowerLawPrior(2.0, (10.0, 400.0))}


@pytest.fixture(scope="module")
def injections(ic):
    return ia.InjectionSet.draw(ic, _draw_priors(), J, LIMITS, seed=5)


def test_draw_is_reproducible_and_lnd_is_the_stated_function_of_the_magnitudes(ic, injections):
    import torch
    again = ia.InjectionSet.draw(ic, _draw_priors(), J, LIMITS, seed=5)
    other = ia.InjectionSet.draw(ic, _draw_priors(), J, LIMITS, seed=6)
    assert list(injections.columns) == ["mass", "age", "feh", "distance"] and injections.J == J
    for name in injections.columns:
        assert np.array_equal(injections.columns[name], again.columns[name])
        assert not np.array_equal(injections.columns[name], other.columns[name])
    assert torch.equal(injections.lnd, again.lnd) and injections.n_off == again.n_off
    assert injections.lnd.is_cuda and injections.lnd.dtype == torch.float64
    # the columns are the draws of one generator in the order of the priors
    rng = np.random.default_rng(5)
    for name, prior in _draw_priors().items():
        assert np.array_equal(injections.columns[name], np.asarray(prior.sample(J, rng), dtype=np.float64)), name
    c = injections.columns
    out = ia.evaluate_binaries(ic, c["mass"], 0.0, c["age"], c["feh"], c["distance"], 0.0, bands=("V", "K"), props=("mass",),
                               accurate="exact")
    V, K = out["V_mag"].cpu().numpy(), out["K_mag"].cpu().numpy()
    off = np.isnan(V) | np.isnan(K)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = log_ndtr((12.0 - V) / 0.2) + np.where(K <= 12.5, 0.0, -np.inf)
    want = np.where(off, -np.inf, want)
    got = injections.lnd.cpu().numpy()
    print("n_off = %d, detected with lnd > ln 0.5: %d of %d" % (off.sum(), (got > np.log(0.5)).sum(), J))
    assert injections.n_off == off.sum() and 0 < off.sum() < J
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any() and (got <= 0).all()
    fin = np.isfinite(want)
    assert fin.sum() > J // 10 and (got > np.log(0.5)).sum() > J // 20
    # torch's and scipy's log_ndtr: a few ulp of the value
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * np.maximum(1.0, np.abs(want[fin])))


@pytest.fixture(scope="module")
def posteriors(ic, injections):
    """a CUDA chain of 24 stars x 16 walkers x 20 steps in (mass, feh); the same posterior with and without injections"""
    import torch
    rng = np.random.default_rng(9)
    S, W, T = 24, 16, 20
    centre = np.stack([rng.uniform(0.8, 1.8, S), rng.uniform(-0.8, 0.3, S)], axis=1)
    chain = centre[:, None, None, :] + np.array([0.03, 0.05]) * rng.normal(size=(S, W, T, 2))
    chain[..., 0] = chain[..., 0].clip(0.7, 2.0)
    chain[..., 1] = chain[..., 1].clip(-1.0, 0.5)
    model = ia.PopulationModel(mass=ia.PowerLaw((0.7, 2.0), alpha=(-4.0, 1.0)),
                               feh=ia.TruncatedGaussian((-1.0, 0.5), mean=(-0.8, 0.4), sigma=(0.1, 1.0)))
    interim = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "feh": P.FlatPrior((-1.0, 0.5))}
    mask = np.ones(S, dtype=np.int32)
    mask[3] = 0
    dchain = torch.from_numpy(chain).cuda()
    kw = dict(interim=interim, mask=mask)
    with_sel = ia.PopulationPosterior((dchain, ("mass", "feh")), ic, model, injections=injections, min_neff_factor=1.0, **kw)
    plain = ia.PopulationPosterior((dchain, ("mass", "feh")), ic, model, **kw)
    return chain, model, kw, with_sel, plain


THETA = np.column_stack([np.linspace(-3.5, 0.5, 11), np.linspace(-0.6, 0.2, 11), np.linspace(0.2, 0.9, 11)])


def test_lnlike_is_the_uncorrected_one_minus_S_ln_alpha(posteriors):
    import torch
    chain, model, kw, with_sel, plain = posteriors
    S = 23
    assert with_sel.n_unmasked == S and not with_sel.host and with_sel.selection.x.is_cuda
    assert with_sel.selection.x.shape == (2, J)                       # the model's columns only, in its order
    got, base = with_sel.lnlike(THETA), plain.lnlike(THETA)
    la, neff = with_sel.ln_alpha(THETA), with_sel.selection_neff(THETA)
    assert isinstance(got, np.ndarray) and np.isfinite(got).all() and np.isfinite(la).all() and (la < 0).all()
    assert np.all(np.abs(got - (base - S * la)) <= 1e-12 * np.abs(got))
    assert (neff > 1).all() and (neff < J).all()
    # star_terms and min_ess are the uncorrected ones, bit for bit
    for a, b in zip(with_sel.star_terms(THETA), plain.star_terms(THETA)):
        assert a.tobytes() == b.tobytes()
    assert with_sel.min_ess(THETA).tobytes() == plain.min_ess(THETA).tobytes()
    # tensor rows give tensors there
    t = with_sel.lnlike(torch.from_numpy(THETA).cuda())
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)
    # lnpost: the n_eff condition, with a factor this small set meets and with one it cannot (n_eff < J / 2 < 100 S)
    lp = with_sel.lnpost(THETA)
    ok = neff >= 1.0 * S
    assert ok.any() and np.array_equal(np.isfinite(lp), ok) and np.array_equal(lp[ok], (with_sel.lnprior(THETA) + got)[ok])
    from isochrones_amd import _chain
    strict = ia.PopulationPosterior((_chain.from_storage(with_sel.storage, 24, 16, False), ("mass", "feh")), None, model, injections=with_sel.injections,
                                    min_neff_factor=100.0, **kw)
    assert (neff < J / 2).all() and np.isneginf(strict.lnpost(THETA)).all()


def test_device_matches_the_host_path(posteriors, injections):
    chain, model, kw, with_sel, plain = posteriors
    host_set = ia.InjectionSet({k: v for k, v in injections.columns.items()}, injections.priors, injections.lnd.cpu().numpy())
    host = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, injections=host_set, **kw)
    assert host.host and isinstance(host.selection.x, np.ndarray)
    got = dict(ln_alpha=with_sel.ln_alpha(THETA), n_eff=with_sel.selection_neff(THETA))
    ref = dict(ln_alpha=host.ln_alpha(THETA), n_eff=host.selection_neff(THETA))
    sel = host.selection
    twin = tw.alpha(sel.x, sel.lnd, sel.draw, model.pack(THETA))
    n_bad = twin.pop("n_bad")                                         # the posterior's methods return the two arrays
    tw.assert_matches(ref, twin, "host path")
    tw.assert_matches(got, twin, "device path")
    tw.assert_matches(got, dict(ref, tmax=twin["tmax"]), "device against host")
    assert int(with_sel.selection.alpha(THETA)[2].item()) == n_bad == 0
    a, b = with_sel.lnlike(THETA), host.lnlike(THETA)
    # 23 star terms within the hierarchical twin's limit each, and 23 times ln_alpha's
    assert np.all(np.abs(a - b) <= 2 * 23 * 1e-11 * np.maximum(1.0, twin["tmax"] / 100.0))


def test_fit_mcmc_runs_on_top(posteriors):
    chain, model, kw, with_sel, plain = posteriors
    smp = with_sel.fit_mcmc(nwalkers=16, nburn=5, niter=5, seed=3)
    df = with_sel.samples
    assert smp is with_sel.sampler and len(df) == 16 * 5 and np.isfinite(df["lnprob"]).all()
