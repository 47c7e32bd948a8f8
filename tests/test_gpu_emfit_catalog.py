"""em_masses and bootstrap of a binned PopulationPosterior on the chains a catalog fit left on the device (the 24 stars on
evolution tracks of the binfit catalog test: an age histogram, where age is a derived column, and [Fe/H] bins per age bin):
one step equals N / sum N of cell_counts at the same heights, replicate 0 of a bootstrap is the unweighted fit, every
status is set, the quantiles are ordered, and the device route ends where the host route ends on the downloaded chain."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _emfit_cabi as ec, catalog as cat, derived as dv, emfit

pytestmark = pytest.mark.gpu

AGE_EDGES = [5.0, 9.0, 9.7, 10.15]
FEH_EDGES = [-4.0, -0.3, 0.0, 0.5]
LOGITS = (-30.0, 30.0)


def _model():
    return ia.PopulationModel(age=ia.Histogram(AGE_EDGES, logits=LOGITS), feh=ia.Histogram(FEH_EDGES, logits=LOGITS, given="age"))


@pytest.fixture(scope="module")
def fitted():
    """The fit of tests/test_gpu_binfit_catalog.py: a fused catalog sampler with 32 walkers x (50 + 50) on a synthetic catalog
    of 24 stars, the device posterior of the binned model and the host posterior on the downloaded chain."""
    import torch
    from isochrones_amd.sampler import FusedEnsembleSampler
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    c, _ = cat.synthetic_catalog(ic, 24, seed=2)
    post = cat.CatalogPosterior.from_catalog(c, ic, N=1)
    pos, lnp, failed = cat.initial_positions(post, 32, rng_seed=2)
    good = ~failed
    assert int(good.sum()) >= 20
    if bool(failed.any()):              # a failed star borrows a good star's walkers, which never move
        src = int(torch.nonzero(good)[0])
        pos[failed] = pos[src].clone()
        lnp = torch.where(failed[:, None], torch.zeros_like(lnp), lnp)
    smp = FusedEnsembleSampler(post, 32, seed=3)
    pos, lnp = smp.run_mcmc(pos, 50, lnprob0=lnp, store=False)
    smp.reset()
    smp.run_mcmc(pos, 50, lnprob0=lnp, store=True)
    mask = good.cpu().numpy().copy()
    mask[5] = False
    pp = ia.PopulationPosterior(smp, ic, _model(), mask=mask)
    assert not pp.host and pp.derived_cols == ["age"]
    S, W = smp.n_ensembles, smp.nwalkers
    chain = smp._chain.contiguous()
    T = chain.shape[0]
    names = list(smp.target.param_names)
    dchain, _ = dv.derive_storage(chain, S, W, ic, ("age",))
    cols = [dchain.cpu().numpy()[:, 0], chain.cpu().numpy()[:, names.index("feh")]]
    x = np.stack([col.reshape(T, S, W).transpose(1, 2, 0) for col in cols], axis=-1)          # [S, W, T, 2]
    template = smp.target.template
    interim = {"age": template._priors["eep"].orig_prior, "feh": template._priors["feh"]}
    host = ia.PopulationPosterior((np.ascontiguousarray(x), ("age", "feh")), None, _model(), interim=interim, mask=mask)
    assert host.host
    yield pp, host
    smp.close()
    post.close()


def test_one_step_is_the_normalised_cell_counts(fitted):
    pp, _ = fitted
    rng = np.random.default_rng(0)
    theta = rng.uniform(-2.0, 2.0, pp.model.n_params)
    g, objective, n_iter, status, n_live = pp.em_masses(g0=emfit.start_masses(pp, theta), max_iter=1, tol=-np.inf)
    N, live = pp.cell_counts(theta[None])
    err = float(np.max(np.abs(g[0] - N[0] / N[0].sum())))
    print("one step of em_masses against N / sum N of cell_counts: %.2e (limit 1e-11), n_live %d" % (err, n_live[0]))
    assert g.shape == (1, 9) and err <= 1e-11 and n_live[0] == live[0] and n_iter[0] == 1 and status[0] == ec.MAX_ITER
    assert np.isfinite(objective).all()


def test_bootstrap_on_the_device(fitted):
    pp, host = fitted
    bs = pp.bootstrap(n_boot=16, seed=4)
    assert isinstance(bs, ia.BinnedBootstrap) and bs.masses.shape == (17, 3, 3) and bs.theta.shape == (17, pp.model.n_params)
    assert set(np.unique(bs.status)) <= {ec.CONVERGED, ec.MAX_ITER, ec.EMPTY} and (bs.status != ec.RUNNING).all()
    assert bs.status[0] != ec.EMPTY and (bs.n_live <= pp.n_unmasked).all() and bs.n_live[0] >= pp.n_unmasked - 4
    # replicate 0 is the unweighted fit: the steps chained one by one through cell_counts give the same masses
    theta = np.zeros(pp.model.n_params)
    g = emfit.start_masses(pp, theta)
    A, mask, device = emfit._where(pp)
    for _ in range(int(bs.n_iter[0])):
        g = emfit.run(A, emfit._scale(pp), None, mask, g, 1, 1, -np.inf, device=device)[0][0]
    N, _ = pp.cell_counts(theta[None])
    first = emfit.run(A, emfit._scale(pp), None, mask, emfit.start_masses(pp, theta), 1, 1, -np.inf, device=device)[0][0]
    assert np.all(np.abs(first - N[0] / N[0].sum()) <= 1e-11)
    # (the result's masses are g renormalised once more, as _m_step does)
    assert np.array_equal(bs.point_masses.reshape(-1), g / g.sum()) and np.array_equal(bs.point_masses, bs.masses[0])
    ok = bs.status[1:] != ec.EMPTY
    assert ok.sum() >= 2 and np.isfinite(bs.mass_sd).all() and (bs.mass_sd >= 0).all()
    assert np.all(np.diff(bs.mass_q, axis=0) >= 0) and bs.mass_q.shape == (3, 3, 3)
    assert np.all(np.abs(bs.masses[np.flatnonzero(bs.status != ec.EMPTY)].sum(axis=(1, 2)) - 1.0) <= 1e-12)
    assert len(bs.frame()) == 9
    # a replicate's row is a hyper row
    r = int(np.flatnonzero(ok)[0]) + 1
    cp = pp.star_bin_probabilities(bs.theta[r:r + 1]).reshape(pp.S, 9).cpu().numpy()
    alive = np.isfinite(cp).all(axis=1)
    assert alive.sum() >= pp.n_unmasked - 4 and np.all(np.abs(cp[alive].sum(axis=1) - 1.0) <= 1e-12)
    # the host route on the downloaded chain ends in the same place
    want = host.bootstrap(n_boot=16, seed=4)
    assert np.array_equal(bs.status == ec.EMPTY, want.status == ec.EMPTY)
    assert np.all(np.abs(bs.n_iter - want.n_iter) <= 1)
    both = (bs.status != ec.EMPTY) & (bs.n_iter == want.n_iter)         # a step apart the masses differ by that step
    apart = float(np.max(np.abs(bs.masses[both] - want.masses[both])))
    print("device against host bootstrap: masses apart by %.2e where the steps agree (%d of 17), n_iter %s against %s"
          % (apart, both.sum(), bs.n_iter, want.n_iter))
    # the two tables differ by rounding (1e-13 of an entry), and a fixed point moves by that over one minus the
    # contraction rate, which a run that converges inside 2000 steps keeps below 1e4: 1e-9, and a hundred times that here
    assert both.sum() >= 9 and apart <= 1e-7
