"""A coupled PopulationPosterior on the chains a catalog fit left on the device: [Fe/H] against age on evolution tracks, so
the parent is a derived column.  lnlike on the device equals the host entry on the downloaded columns within the twin's
limits, and fit_mcmc over the hyper-parameters returns finite log-probabilities."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _relation_cabi as rl, derived as dv, priors as P
from tests import _hier_twin as tw, _relation_twin as rt
from tests.test_gpu_hier_catalog import _fitted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def track_fit():
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    post, smp, good = _fitted(ic, 64, seed=2)
    yield ic, smp, good
    smp.close()
    post.close()


def _model():
    return ia.PopulationModel(age=ia.Fixed(P.FlatLogPrior((5.0, 10.15))),
                              feh=ia.LinearGaussian("age", (-4.0, 0.5), (-1.0, 1.0), intercept=(-1.0, 0.5), sigma=(0.1, 1.0), pivot=9.6))


def test_coupled_population_matches_the_host_entry(track_fit):
    import torch
    ic, smp, good = track_fit
    model = _model()
    mask = good.copy()
    mask[5] = False
    pp = ia.PopulationPosterior(smp, ic, model, mask=mask)
    assert model.coupled and pp.derived_cols == ["age"] and pp.chain_cols == {"feh": list(smp.target.param_names).index("feh")} and not pp.host
    rng = np.random.default_rng(0)
    theta = np.column_stack([rng.uniform(-0.6, 0.2, 8), rng.uniform(-1.0, 1.0, 8), rng.uniform(0.15, 0.8, 8)])
    L, mn, ell, ess, n_bad = pp._evaluate(torch.as_tensor(theta, device="cuda"))
    assert all(t.is_cuda for t in (L, mn, ell, ess, n_bad)) and ell.shape == (8, 64)
    got = dict(L=L.cpu().numpy(), min_ess=mn.cpu().numpy(), ell=ell.cpu().numpy(), ess=ess.cpu().numpy(), n_bad=n_bad.cpu().numpy())
    # the same columns on the host: age from the derived chain, [Fe/H] from the sampler's
    S, W = smp.n_ensembles, smp.nwalkers
    chain = smp._chain.contiguous()
    T = chain.shape[0]
    names = list(smp.target.param_names)
    dchain, _ = dv.derive_storage(chain, S, W, ic, ("age",))
    cols = [dchain.cpu().numpy()[:, 0], chain.cpu().numpy()[:, names.index("feh")]]
    x = np.array([c.reshape(T, S, W).transpose(1, 0, 2).reshape(S, T * W) for c in cols])
    tmpl = smp.target.template
    interim = [tmpl._priors["eep"].orig_prior, tmpl._priors["feh"]]
    case = tw.fixed_case(x, interim, [list(r[:, None]) for r in model.pack(theta)], W, T, mask=mask.astype(np.int32))
    assert (case["rows"][:, 1]["kind"] == rl.LINGAUSS).all() and (case["rows"][:, 1]["reserved"] == 0).all()
    rc, host = rt.call(rl.lib(), case)
    assert rc == 0
    rt.assert_matches(host, rt.want(case), "track catalog, host")
    rt.assert_matches(got, dict(host, rmax=rt.want(case)["rmax"]), "track catalog")
    assert np.isnan(got["ell"][:, 5]).all() and np.isfinite(got["ell"][:, mask]).all() and np.isfinite(got["L"]).all()
    # the slope matters: the rows differ in nothing else that could move L this much
    assert np.ptp(got["L"]) > 1.0
    again = pp.lnlike(theta)
    assert isinstance(again, np.ndarray) and again.tobytes() == got["L"].tobytes()
    with pytest.raises(ValueError, match="uncoupled"):
        pp.star_posteriors(theta)


def test_fit_mcmc_returns_finite_lnprob(track_fit):
    ic, smp, good = track_fit
    pp = ia.PopulationPosterior(smp, ic, _model(), mask=good)
    a = pp.fit_mcmc(nwalkers=16, nburn=10, niter=10, seed=5)
    df = pp.samples
    assert list(df.columns) == ["feh.intercept", "feh.slope", "feh.sigma", "lnprob"] and len(df) == 16 * 10
    assert np.isfinite(df["lnprob"]).all() and a.flatchain.is_cuda
