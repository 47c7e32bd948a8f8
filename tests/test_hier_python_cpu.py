"""isochrones_amd.hierarchical without a device: a host numpy chain goes through iso_hier_lnlike_host.  Packing, names,
the flat hyper-prior, the refusals, budget slicing, and a closed-form case."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import hierarchical as hi, priors as P
from isochrones_amd.csrc.libraries import HIER as build_hier


@pytest.fixture(scope="module", autouse=True)
def _built():
    build_hier.build()


def _model():
    return ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0)), feh=ia.TruncatedGaussian((-4.0, 0.5)),
                              age=ia.Fixed(P.AgePrior()))


def test_param_names_and_exports():
    m = _model()
    assert m.param_names == ("mass.alpha", "feh.mean", "feh.sigma") and m.n_params == 3
    assert m.columns == ("mass", "feh", "age")
    assert ia.PopulationPosterior is hi.PopulationPosterior and ia.hierarchical is hi


def test_vectorised_pack_equals_row_by_row():
    m = _model()
    rng = np.random.default_rng(0)
    th = np.column_stack([rng.uniform(-5, 5, 300), rng.uniform(-4, 0.5, 300), rng.uniform(0.005, 4.5, 300)])
    th[:3, 0] = (-1.0, -1.0 + 1e-12, -2.35)
    th[3] = (0.0, 0.49, 0.01)                        # a mean next to the upper bound, a narrow sigma
    th[4] = (0.0, -3.9, 0.02)
    whole = m.pack(th)
    assert whole.shape == (300, 3) and whole.dtype == hi.hc.RECORD
    rows = np.concatenate([m.pack(th[h:h + 1]) for h in range(300)])
    assert whole.tobytes() == rows.tobytes()
    assert np.isfinite(whole["p"]).all()
    assert (whole["kind"] == [hi.hc.POWERLAW, hi.hc.TRUNCGAUSS, hi.hc.FLATLOG]).all()


def test_lnprior_is_flat_inside_the_ranges():
    m = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0), alpha=(-4.0, 0.0)),
                           feh=ia.TruncatedGaussian((-4.0, 0.5), mean=(-1.0, 0.5), sigma=(0.05, 1.0)))
    th = np.array([[-2.0, 0.0, 0.2], [-4.0, -1.0, 0.05], [0.0, 0.5, 1.0], [0.1, 0.0, 0.2], [-2.0, -1.1, 0.2], [-2.0, 0.0, 0.04],
                   [-2.0, 0.0, 1.5]])
    lp = m.lnprior(th)
    assert np.allclose(lp[:3], -np.log(4.0 * 1.5 * 0.95), rtol=0, atol=1e-15) and np.isneginf(lp[3:]).all()
    chain = np.random.default_rng(1).normal(0.0, 0.2, (4, 6, 5, 1))
    pp = ia.PopulationPosterior((chain, ("feh",)), None, ia.PopulationModel(feh=ia.TruncatedGaussian((-4.0, 0.5))),
                                interim={"feh": P.FlatPrior((-4.0, 0.5))})
    post = pp.lnpost(np.array([[0.0, 0.3], [0.0, 5.0], [-5.0, 0.3]]))
    assert np.isfinite(post[0]) and np.isneginf(post[1:]).all()
    assert post[0] == pp.lnprior(np.array([[0.0, 0.3]]))[0] + pp.lnlike(np.array([[0.0, 0.3]]))[0]


def test_refusals():
    chain = np.random.default_rng(1).normal(0.0, 0.2, (4, 6, 5, 2))
    flat = P.FlatPrior((-4.0, 4.0))
    fam = lambda: ia.TruncatedGaussian((-4.0, 4.0))
    with pytest.raises(ValueError, match="1 to 4 columns"):
        ia.PopulationModel(a=fam(), b=fam(), c=fam(), d=fam(), e=fam())
    with pytest.raises(ValueError, match="1 to 4 columns"):
        ia.PopulationModel()
    with pytest.raises(TypeError, match="PowerLaw, TruncatedGaussian or Fixed"):
        ia.PopulationModel(a=flat)
    with pytest.raises(ValueError, match="0 < lo < hi"):
        ia.PowerLaw((0.0, 1.0))

    class Mine(P.Prior):
        bounds = (-4.0, 4.0)

        def _pdf(self, x):
            return 0.125
    with pytest.raises(ValueError, match="evaluated on the host"):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(a=fam()), interim={"a": Mine()})
    with pytest.raises(ValueError, match="evaluated on the host"):
        ia.Fixed(Mine())
    with pytest.raises(ValueError, match="neither a parameter of the chain"):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(c=fam()), interim={"c": flat})
    with pytest.raises(ValueError, match="no interim prior for b"):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(a=fam(), b=fam()), interim={"a": flat})
    with pytest.raises(ValueError, match="needs interim="):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(a=fam()))
    with pytest.raises(ValueError, match="parameter names"):
        ia.PopulationPosterior((chain, ("a",)), None, ia.PopulationModel(a=fam()), interim={"a": flat})
    with pytest.raises(ValueError, match=r"mask must be \[S\]"):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(a=fam()), interim={"a": flat}, mask=[1, 1])
    with pytest.raises(ValueError, match="more than budget_bytes"):
        ia.PopulationPosterior((chain, ("a", "b")), None, ia.PopulationModel(a=fam()), interim={"a": flat}, budget_bytes=100)
    # a model-grid column is derived on the device: a host chain cannot have one
    from tests import _predict_twin
    ic = _predict_twin.ichrone("track")
    with pytest.raises(ValueError, match="derived on the device"):
        ia.PopulationPosterior((chain, ("a", "b")), ic, ia.PopulationModel(age=fam()), interim={"age": flat})

    # N > 1: refused before anything else is looked at
    from isochrones_amd.sampler import FusedEnsembleSampler

    class Target:
        N, param_names = 2, ("eep_0", "eep_1", "age", "feh", "distance", "AV")
    fake = FusedEnsembleSampler.__new__(FusedEnsembleSampler)
    fake._chain, fake.is_catalog, fake.target, fake._h = np.zeros((5, 6, 24)), False, Target(), None
    with pytest.raises(ValueError, match=r"single stars \(N = 1\)"):
        ia.PopulationPosterior(fake, ic, ia.PopulationModel(feh=fam()))


def test_budget_slices_give_the_same_bits():
    rng = np.random.default_rng(2)
    S, W, T = 5, 6, 7
    chain = np.stack([np.exp(rng.normal(0.0, 0.4, (S, W, T))), rng.normal(-0.1, 0.3, (S, W, T))], axis=3)
    model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0)), feh=ia.TruncatedGaussian((-4.0, 0.5)))
    interim = {"mass": P.ChabrierPrior(), "feh": P.FehPrior(bounds=(-4.0, 0.5))}
    mask = [1, 1, 0, 1, 1]
    th = np.column_stack([rng.uniform(-3, 0, 11), rng.uniform(-0.5, 0.2, 11), rng.uniform(0.1, 0.6, 11)])
    whole = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, interim=interim, mask=mask)
    one = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, interim=interim, mask=mask, budget_bytes=W * T * 8)
    two = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, interim=interim, mask=mask, budget_bytes=2 * W * T * 8 + 5)
    assert (whole.step, one.step, two.step) == (5, 1, 2)
    a, b, c = whole._evaluate(th), one._evaluate(th), two._evaluate(th)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert np.isnan(a[2][:, 2]).all() and np.isfinite(a[0]).all() and a[2].shape == (11, 5) and a[4].shape == (5,)
    ell, ess, n_bad = whole.star_terms(th)
    # a sample outside the interim prior's bounds is bad; the masked star reports none
    outside = ((chain[..., 1] > 0.5) | (chain[..., 1] < -4.0)).reshape(S, -1).sum(axis=1) * np.array(mask)
    assert ell.tobytes() == a[2].tobytes() and (n_bad == outside).all() and outside.sum() > 0
    assert whole.min_ess(th).tobytes() == a[1].tobytes()
    # torch in, torch out
    import torch
    t = whole.lnlike(torch.from_numpy(th))
    assert isinstance(t, torch.Tensor) and t.numpy().tobytes() == a[0].tobytes()


@pytest.fixture(scope="module")
def closed_form():
    """Stars with a Gaussian truth and Gaussian errors under a flat interim prior: the per-star term is known exactly.
    truth ~ N(-0.2, 0.15), obs = truth + N(0, 0.1), samples = obs + 0.1 N(0, 1); then
    ell = ln N(obs; mu, sqrt(sigma^2 + 0.01)) + ln 8 for the population N(mu, sigma) on (-4, 4)."""
    rng = np.random.default_rng(7)
    S, M = 200, 4096
    truth = rng.normal(-0.2, 0.15, S)
    obs = truth + rng.normal(0.0, 0.1, S)
    samples = obs[:, None] + 0.1 * rng.standard_normal((S, M))
    chain = samples.reshape(S, 64, 64, 1)
    pp = ia.PopulationPosterior((chain, ("feh",)), None, ia.PopulationModel(feh=ia.TruncatedGaussian((-4.0, 4.0))),
                                interim={"feh": P.FlatPrior((-4.0, 4.0))})
    return pp, obs, M


def test_closed_form_star_terms(closed_form):
    pp, obs, M = closed_form
    th = np.array([[-0.2, 0.15], [-0.3, 0.3]])
    ell, ess, n_bad = pp.star_terms(th)
    assert (n_bad == 0).all()
    for k, (mu, sg) in enumerate(th):
        s2 = sg * sg + 0.01
        exact = -0.5 * np.log(2 * np.pi * s2) - 0.5 * (obs - mu) ** 2 / s2 + np.log(8.0)
        err = np.abs(ell[k] - exact) / np.sqrt(1.0 / ess[k] - 1.0 / M)
        print("row", th[k], "worst |ell - exact| = %.2f standard errors" % err.max())
        assert err.max() <= 5.0


def test_closed_form_degenerate_rows_are_flagged(closed_form):
    pp, _, _ = closed_form
    mn = pp.min_ess(np.array([[0.0, 0.05], [-0.2, 0.02]]))
    print("min_ess", mn)
    assert (mn < 2.0).all()
    assert (pp.min_ess(np.array([[-0.2, 0.15]])) > 100).all()


def test_closed_form_maximum(closed_form):
    pp, _, _ = closed_form
    mus, sgs = np.linspace(-0.4, 0.0, 41), np.linspace(0.05, 0.3, 26)
    grid = np.array([(m, s) for m in mus for s in sgs])
    # rows are independent (a row alone gives the same bits as inside any H): the host entry takes the grid in eight parts
    # at once, which ctypes allows (the GIL is released during the call)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        L = np.concatenate(list(pool.map(pp.lnlike, np.array_split(grid, 8))))
    assert L.shape == (41 * 26,) and np.array_equal(L[:3], pp.lnlike(grid[:3]))
    m, s = grid[np.argmax(L)]
    print("maximum at", m, s)
    assert abs(m - (-0.23)) <= (mus[1] - mus[0]) * (1 + 1e-9) and abs(s - 0.13) <= (sgs[1] - sgs[0]) * (1 + 1e-9)


def test_fit_mcmc_on_the_host_route(closed_form):
    pp, _, _ = closed_form
    small = ia.PopulationPosterior((pp.storage.reshape(pp.T, 1, pp.S, pp.W)[:, :, :40].transpose(2, 3, 0, 1), ("feh",)), None,
                                   ia.PopulationModel(feh=ia.TruncatedGaussian((-4.0, 4.0), mean=(-1.0, 1.0), sigma=(0.05, 1.0))),
                                   interim={"feh": P.FlatPrior((-4.0, 4.0))})
    s1 = small.fit_mcmc(nwalkers=8, nburn=10, niter=10, seed=3)
    df = small.samples
    assert list(df.columns) == ["feh.mean", "feh.sigma", "lnprob"] and len(df) == 80 and np.isfinite(df["lnprob"]).all()
    s2 = small.fit_mcmc(nwalkers=8, nburn=10, niter=10, seed=3)
    assert s1.flatchain.numpy().tobytes() == s2.flatchain.numpy().tobytes()
