"""PopulationPosterior on the chains a catalog fit left on the device: it equals the host entry on the chain copied to the
host, a star marked failed is left out, the isochrone parametrisation derives its mass column, and fit_mcmc over the
hyper-parameters reproduces under a seed."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import catalog as cat, derived as dv, priors as P
from tests import _hier_twin as tw

pytestmark = pytest.mark.gpu


def _fitted(ic, n_stars, seed):
    """A fused catalog sampler with 32 walkers x (50 + 50) on a synthetic catalog, and the stars without a start point."""
    import torch
    from isochrones_amd.sampler import FusedEnsembleSampler
    c, _ = cat.synthetic_catalog(ic, n_stars, seed=seed)
    post = cat.CatalogPosterior.from_catalog(c, ic, N=1)
    pos, lnp, failed = cat.initial_positions(post, 32, rng_seed=seed)
    good = ~failed
    assert int(good.sum()) >= n_stars - 4
    if bool(failed.any()):              # a failed star borrows a good star's walkers, which never move
        src = int(torch.nonzero(good)[0])
        pos[failed] = pos[src].clone()
        lnp = torch.where(failed[:, None], torch.zeros_like(lnp), lnp)
    smp = FusedEnsembleSampler(post, 32, seed=seed + 1)
    pos, lnp = smp.run_mcmc(pos, 50, lnprob0=lnp, store=False)
    smp.reset()
    smp.run_mcmc(pos, 50, lnprob0=lnp, store=True)
    return post, smp, good.cpu().numpy()


def _host_reference(smp, ic, columns, derived_cols, model, interim, mask, theta):
    """The same numbers from the library's host entry on the chain (and the derived chain) copied to the host."""
    S, W = smp.n_ensembles, smp.nwalkers
    chain = smp._chain.contiguous()
    T, D = chain.shape[0], chain.shape[1]
    names = list(smp.target.param_names)
    x = []
    if derived_cols:
        dchain, _ = dv.derive_storage(chain, S, W, ic, tuple(derived_cols))
        dhost = dchain.cpu().numpy()
    host = chain.cpu().numpy()
    for col in columns:
        st = host[:, names.index(col)] if col in names else dhost[:, derived_cols.index(col)]
        x.append(st.reshape(T, S, W).transpose(1, 0, 2).reshape(S, T * W))
    case = tw.fixed_case(np.array(x), [interim[c] for c in columns], [list(r[:, None]) for r in model.pack(theta)], W, T,
                         mask=mask)
    rc, got = tw.call(ia.hierarchical.hc.lib(), case)
    assert rc == 0
    return got, tw.want(case) if S * T * W * len(theta) <= 2_000_000 else None


@pytest.fixture(scope="module")
def track_fit():
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    post, smp, good = _fitted(ic, 64, seed=2)
    yield ic, smp, good
    smp.close()
    post.close()


def test_catalog_population_matches_the_host_entry(track_fit):
    import torch
    ic, smp, good = track_fit
    model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0)), age=ia.TruncatedGaussian((5.0, 10.15)))
    mask = good.copy()
    mask[5] = False                                                  # a star marked failed
    pp = ia.PopulationPosterior(smp, ic, model, mask=mask)
    assert pp.chain_cols == {"mass": 0} and pp.derived_cols == ["age"] and not pp.host
    rng = np.random.default_rng(0)
    theta = np.column_stack([rng.uniform(-3.0, 0.0, 8), rng.uniform(9.0, 10.0, 8), rng.uniform(0.3, 1.0, 8)])
    L, mn, ell, ess, n_bad = pp._evaluate(torch.as_tensor(theta, device="cuda"))
    assert all(t.is_cuda for t in (L, mn, ell, ess, n_bad)) and ell.shape == (8, 64)
    tmpl = smp.target.template
    interim = {"mass": tmpl._priors["mass"], "age": tmpl._priors["eep"].orig_prior}
    assert isinstance(interim["age"], P.FlatLogPrior)
    host, want = _host_reference(smp, ic, ("mass", "age"), ["age"], model, interim, mask.astype(np.int32), theta)
    got = dict(L=L.cpu().numpy(), min_ess=mn.cpu().numpy(), ell=ell.cpu().numpy(), ess=ess.cpu().numpy(),
               n_bad=n_bad.cpu().numpy())
    tw.assert_matches(got, dict(host, rmax=want["rmax"]), "track catalog")
    assert np.isnan(got["ell"][:, 5]).all() and np.isfinite(got["ell"][:, mask]).all() and np.isfinite(got["L"]).all()
    keep = np.flatnonzero(mask)
    assert np.allclose(got["L"], got["ell"][:, keep].sum(axis=1), rtol=1e-13, atol=0)
    # numpy in, numpy out: the same bits; slices of the stars change no bit of a star's row
    again = pp.lnlike(theta)
    assert isinstance(again, np.ndarray) and again.tobytes() == got["L"].tobytes()
    cut = ia.PopulationPosterior(smp, ic, model, mask=mask, budget_bytes=10 * 50 * 32 * 8)
    assert cut.step == 10
    e2, s2, b2 = cut.star_terms(theta)
    assert e2.tobytes() == got["ell"].tobytes() and s2.tobytes() == got["ess"].tobytes() and b2.tobytes() == got["n_bad"].tobytes()


def test_fit_mcmc_reproduces_under_its_seed(track_fit):
    ic, smp, good = track_fit
    model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0), alpha=(-4.0, 1.0)),
                               feh=ia.TruncatedGaussian((-4.0, 0.5), mean=(-1.0, 0.5), sigma=(0.1, 1.0)))
    pp = ia.PopulationPosterior(smp, ic, model, mask=good)
    assert model.param_names == ("mass.alpha", "feh.mean", "feh.sigma")
    a = pp.fit_mcmc(nwalkers=16, nburn=20, niter=20, seed=5)
    df = pp.samples
    assert list(df.columns) == ["mass.alpha", "feh.mean", "feh.sigma", "lnprob"] and len(df) == 16 * 20
    assert np.isfinite(df["lnprob"]).all() and a.flatchain.is_cuda
    first = a.flatchain.cpu().numpy().copy()
    b = pp.fit_mcmc(nwalkers=16, nburn=20, niter=20, seed=5)
    assert b.flatchain.cpu().numpy().tobytes() == first.tobytes()
    assert b.flatlnprobability.cpu().numpy().tobytes() == df["lnprob"].values.tobytes()


def test_isochrone_parametrisation_derives_its_mass_column():
    import torch
    ages = ia.grids.mist_log_ages()[60::2]
    iso = ia.synthetic_isochrone(bands=("V", "J", "K"), ages=ages, fehs=[-1.0, -0.5, 0.0, 0.5], eeps=np.arange(150.0, 700.0),
                                 eep_bounds=(150, 699), limits=dict(age=(ages[0], ages[-1]), feh=(-1.0, 0.5)))
    post, smp, good = _fitted(iso, 16, seed=4)
    try:
        model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0)), feh=ia.Fixed(P.FehPrior(bounds=(-1.0, 0.5))))
        pp = ia.PopulationPosterior(smp, iso, model, mask=good)
        assert pp.derived_cols == ["mass"] and pp.chain_cols == {"feh": 2}
        theta = np.array([[-2.35], [-1.0], [0.0]])
        ell, ess, n_bad = pp.star_terms(torch.as_tensor(theta, device="cuda"))
        tmpl = smp.target.template
        interim = {"mass": tmpl._priors["eep"].orig_prior, "feh": tmpl._priors["feh"]}
        assert isinstance(interim["mass"], P.ChabrierPrior)
        host, want = _host_reference(smp, iso, ("mass", "feh"), ["mass"], model, interim, good.astype(np.int32), theta)
        got = dict(ell=ell.cpu().numpy(), ess=ess.cpu().numpy(), n_bad=n_bad.cpu().numpy(), L=pp.lnlike(theta),
                   min_ess=pp.min_ess(theta))
        tw.assert_matches(got, dict(host, rmax=want["rmax"]), "isochrone catalog")
        assert np.isfinite(got["ell"][:, good]).all()
    finally:
        smp.close()
        post.close()
