"""A binned PopulationPosterior on the chains a catalog fit left on the device: an age histogram on evolution tracks (age is a
derived column) and [Fe/H] bins per age bin.  The tables built in two slices under a small budget_bytes are the bits of one
slice; lnlike on the device equals the host entry on the downloaded columns within the twin's limits; fit_mcmc over the
logits returns finite log-probabilities; an injection set drawn by InjectionSet.draw gives a finite ln_alpha, the same as
the host route's."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _binned_cabi as bc, derived as dv, hierarchical as hi, priors as P
from isochrones_amd.binned import BinnedSelection
from tests import _binned_twin as bt, _hier_twin as tw
from tests.test_gpu_hier_catalog import _fitted

pytestmark = pytest.mark.gpu

AGE_EDGES = [5.0, 9.0, 9.7, 10.15]
FEH_EDGES = [-4.0, -0.3, 0.0, 0.5]


@pytest.fixture(scope="module")
def track_fit():
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    post, smp, good = _fitted(ic, 24, seed=2)
    yield ic, smp, good
    smp.close()
    post.close()


def _model():
    return ia.PopulationModel(age=ia.Histogram(AGE_EDGES), feh=ia.Histogram(FEH_EDGES, given="age"))


def test_binned_population_on_a_catalog(track_fit):
    import torch
    ic, smp, good = track_fit
    model = _model()
    mask = good.copy()
    mask[5] = False
    pp = ia.PopulationPosterior(smp, ic, model, mask=mask)
    assert model.binned and pp.derived_cols == ["age"] and not pp.host and pp.step == 24
    S, W = smp.n_ensembles, smp.nwalkers
    chain = smp._chain.contiguous()
    T = chain.shape[0]
    sliced = ia.PopulationPosterior(smp, ic, model, mask=mask, budget_bytes=T * W * 8 * 12)
    assert sliced.step == 12
    tables, two = pp.bin_tables(), sliced.bin_tables()
    assert all(t.is_cuda for t in tables) and tables[0].shape == (9, 24) and pp._dev["derived"] is None
    for a, b in zip(tables, two):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    rng = np.random.default_rng(0)
    theta = rng.uniform(-2.0, 2.0, (9, model.n_params))
    L, mn, ell, ess, n_bad = pp._evaluate(torch.as_tensor(theta, device="cuda"))
    assert all(t.is_cuda for t in (L, mn, ell, ess, n_bad)) and ell.shape == (9, 24)
    got = dict(L=L.cpu().numpy(), min_ess=mn.cpu().numpy(), ell=ell.cpu().numpy(), ess=ess.cpu().numpy())
    # the same columns on the host: age from the derived chain, [Fe/H] from the sampler's
    names = list(smp.target.param_names)
    dchain, _ = dv.derive_storage(chain, S, W, ic, ("age",))
    cols = [dchain.cpu().numpy()[:, 0], chain.cpu().numpy()[:, names.index("feh")]]
    x = np.array([c.reshape(T, S, W).transpose(1, 0, 2).reshape(S, T * W) for c in cols])
    grid = model.bin_grid()
    case = dict(x=x, interim=pp.interim, frozen=grid["frozen"], frozen_cols=grid["frozen_cols"], axes=grid["axes"],
                edges=grid["edges"], S=S, W=W, T=T, layout=bt.PM, mask=mask.astype(np.int32), extra=None,
                lnh=model.cell_table(theta)["lnh"])
    case["storages"], case["where"] = tw.place(x, W, T, bt.PM, 0)
    htab, host = bt.run(bc.lib(), case)
    bt.assert_tables_match(htab, case, "track catalog, host")
    dtab = dict(zip(("A", "A2", "mx", "n_bad", "n_out"), (t.cpu().numpy() for t in tables)))
    bt.assert_tables_match(dtab, case, "track catalog")
    bt.assert_matches(host, case, "track catalog, host")
    bt.assert_matches(got, case, "track catalog")
    # lnlike and the star terms against the host entry on the downloaded chain: ell at the limit, L at S times it
    print("track catalog: device against host max |d ell| = %.2e"
          % bt.assert_device_matches_host(dtab, got, htab, host, case, "track catalog, device against host"))
    assert np.isnan(got["ell"][:, 5]).all() and np.isfinite(got["ell"][:, mask]).all() and np.isfinite(got["L"]).all()
    assert np.array_equal(n_bad.cpu().numpy(), htab["n_bad"]) and np.ptp(got["L"]) > 1.0
    again = pp.lnlike(theta)
    assert isinstance(again, np.ndarray) and again.tobytes() == got["L"].tobytes()
    assert all(a is b for a, b in zip(pp.bin_tables(), tables))           # compressed once
    assert sliced.lnlike(theta).tobytes() == again.tobytes()


def test_fit_mcmc_returns_finite_lnprob(track_fit):
    ic, smp, good = track_fit
    pp = ia.PopulationPosterior(smp, ic, _model(), mask=good)
    tables = pp.bin_tables()
    a = pp.fit_mcmc(nwalkers=24, nburn=5, niter=5, seed=5)
    df = pp.samples
    assert list(df.columns) == list(pp.model.param_names) + ["lnprob"] and len(df) == 24 * 5
    assert np.isfinite(df["lnprob"]).all() and a.flatchain.is_cuda
    assert all(x is y for x, y in zip(pp.bin_tables(), tables))


def test_injections_give_a_finite_ln_alpha():
    import torch
    ic = ia.synthetic_track(bands=("V", "J", "K"), fehs=np.array([-1.0, -0.5, 0.0, 0.5]),
                            masses=np.array([0.7, 0.9, 1.0, 1.1, 1.3, 2.0]), eeps=np.arange(300.0, 420.0),
                            limits=dict(mass=(0.7, 2.0), feh=(-1.0, 0.5), age=(5, 10.13)), eep_bounds=(300, 419))
    draw = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "age": P.FlatPrior((7.2, 8.1)), "feh": P.FlatPrior((-1.0, 0.5)),
            "distance": P.PowerLawPrior(2.0, (10.0, 400.0))}
    J = 2000
    inj = ia.InjectionSet.draw(ic, draw, J, {"V": (12.0, 0.2), "K": (12.5, 0.0)}, seed=5)
    rng = np.random.default_rng(9)
    S, W, T = 24, 16, 20
    centre = np.stack([rng.uniform(0.8, 1.8, S), rng.uniform(-0.8, 0.3, S)], axis=1)
    chain = centre[:, None, None, :] + np.array([0.03, 0.05]) * rng.normal(size=(S, W, T, 2))
    chain[..., 0] = chain[..., 0].clip(0.7, 2.0)
    chain[..., 1] = chain[..., 1].clip(-1.0, 0.5)
    model = ia.PopulationModel(mass=ia.Fixed(P.PowerLawPrior(-1.5, (0.7, 2.0))), feh=ia.Histogram([-1.0, -0.5, 0.0, 0.5]))
    interim = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "feh": P.FlatPrior((-1.0, 0.5))}
    dev_pp = ia.PopulationPosterior((torch.from_numpy(chain).cuda(), ("mass", "feh")), ic, model, interim=interim, injections=inj,
                                    min_neff_factor=1.0)
    host_pp = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, interim=interim, injections=inj, min_neff_factor=1.0)
    assert isinstance(dev_pp.selection, BinnedSelection) and dev_pp.selection.tables[0].is_cuda
    theta = rng.uniform(-2.0, 2.0, (9, 2))
    la, neff = dev_pp.ln_alpha(theta), dev_pp.selection_neff(theta)
    assert isinstance(la, np.ndarray) and np.isfinite(la).all() and (la < 0).all() and (neff > 1).all() and (neff < J).all()
    assert np.all(np.abs(la - host_pp.ln_alpha(theta)) <= 1e-11)
    assert np.all(np.abs(neff - host_pp.selection_neff(theta)) <= 1e-10 * neff)
    cut = BinnedSelection(inj, model, torch.device("cuda", 0), chunk=300)            # six ensembles and a remainder of 200
    assert np.all(np.abs(cut.alpha(theta)[0].cpu().numpy() - la) <= 1e-11)
    got, base = dev_pp.lnlike(theta), dev_pp._evaluate(theta)[0]
    assert np.isfinite(got).all() and np.all(np.abs(got - (base - S * la)) <= 1e-12 * np.abs(got))
    assert np.all(np.abs(got - host_pp.lnlike(theta)) <= 1e-9)
    assert np.isfinite(dev_pp.lnpost(theta)).any()
