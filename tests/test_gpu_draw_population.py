"""The Python layer over libiso_draw.so on the device: StarPopulation.generate(rng="philox") on the small synthetic tables,
InjectionSet.draw(rng="philox") with its columns on the device, and PopulationModel.sample against the host entry."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import priors as P
from tests import _population_twin as tw

pytestmark = pytest.mark.gpu


def _population(ic):
    from scipy.stats import uniform
    from isochrones_amd import populations as pp
    return pp.StarPopulation(ic, imf=P.FlatPrior((0.2, 1.2)), sfh=pp.StarFormationHistory(uniform(0.1, 0.25)),
                             feh=P.FlatPrior((-0.9, 0.4)), distance=P.FlatPrior((50.0, 500.0)), AV=P.AVPrior((0.0, 1.0)))


def test_generate_philox_on_the_device():
    import torch
    pop = _population(tw.small_ic())
    d = pop.generate(1000, rng="philox", seed=1, as_tensors=True)
    assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == (1000,) for v in d.values())
    assert not torch.isnan(d["mass_0"]).any()
    again = pop.generate(1000, rng="philox", seed=1, as_tensors=True)
    for c in d:
        assert tw.same_bits(d[c].cpu().numpy(), again[c].cpu().numpy()), c
    assert not torch.equal(pop.generate(1000, rng="philox", seed=2, as_tensors=True)["mass_0"], d["mass_0"])
    few = pop.generate(300, rng="philox", seed=1, as_tensors=True)          # system j is the same whatever N
    for c in d:
        assert tw.same_bits(d[c][:300].cpu().numpy(), few[c].cpu().numpy()), c
    df = pop.generate(300, rng="philox", seed=1)
    assert list(df.columns) == list(d) and tw.same_bits(df["mass_0"].values, few["mass_0"].cpu().numpy())


def test_injection_set_philox_columns_stay_on_the_device():
    import torch
    ic = ia.synthetic_track(bands=("V", "J", "K"), fehs=np.array([-1.0, -0.5, 0.0, 0.5]),
                            masses=np.array([0.7, 0.9, 1.0, 1.1, 1.3, 2.0]), eeps=np.arange(300.0, 420.0),
                            limits=dict(mass=(0.7, 2.0), feh=(-1.0, 0.5), age=(5, 10.13)), eep_bounds=(300, 419))
    draw = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "age": P.FlatPrior((7.2, 8.1)), "feh": P.FlatPrior((-1.0, 0.5)),
            "distance": P.PowerLawPrior(2.0, (10.0, 400.0))}
    limits = {"V": (12.0, 0.2), "K": (12.5, 0.0)}
    inj = ia.InjectionSet.draw(ic, draw, 4096, limits, seed=5, rng="philox")
    assert list(inj.columns) == list(draw) and inj.J == 4096
    assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 for v in inj.columns.values()) and inj.lnd.is_cuda
    for name, prior in draw.items():
        lo, hi = prior.bounds
        assert bool(((inj.columns[name] >= lo) & (inj.columns[name] <= hi)).all()), name
    rng = np.random.default_rng(9)
    S, W, T = 8, 16, 10
    centre = np.stack([rng.uniform(0.8, 1.8, S), rng.uniform(-0.8, 0.3, S)], axis=1)
    chain = centre[:, None, None, :] + np.array([0.03, 0.05]) * rng.normal(size=(S, W, T, 2))
    chain[..., 0], chain[..., 1] = chain[..., 0].clip(0.7, 2.0), chain[..., 1].clip(-1.0, 0.5)
    model = ia.PopulationModel(mass=ia.PowerLaw((0.7, 2.0), alpha=(-4.0, 1.0)),
                               feh=ia.TruncatedGaussian((-1.0, 0.5), mean=(-0.8, 0.4), sigma=(0.1, 1.0)))
    interim = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "feh": P.FlatPrior((-1.0, 0.5))}
    post = ia.PopulationPosterior((torch.from_numpy(chain).cuda(), ("mass", "feh")), ic, model, interim=interim, injections=inj,
                                  min_neff_factor=1.0)
    theta = np.column_stack([np.linspace(-3.5, 0.5, 5), np.linspace(-0.6, 0.2, 5), np.linspace(0.2, 0.9, 5)])
    la = post.ln_alpha(theta)
    assert np.isfinite(la).all() and (la < 0).all()
    assert post.ln_alpha(theta).tobytes() == la.tobytes()
    again = ia.InjectionSet.draw(ic, draw, 4096, limits, seed=5, rng="philox")
    assert all(torch.equal(inj.columns[c], again.columns[c]) for c in draw) and torch.equal(inj.lnd, again.lnd)


def test_population_model_sample_on_the_device_equals_the_host_entry():
    import torch
    age_e, feh_e = np.array([8.0, 9.0, 9.5, 10.0]), np.array([-1.0, -0.5, 0.0, 0.25, 0.5])
    binned = ia.PopulationModel(age=ia.Histogram(age_e), feh=ia.Histogram(feh_e, given="age"), mass=ia.Fixed(P.ChabrierPrior()))
    linked = ia.PopulationModel(age=ia.Fixed(P.FlatPrior((8.0, 10.0))),
                                feh=ia.LinearGaussian("age", (-2.0, 1.0), slope=(-2.0, 2.0), sigma=(0.05, 1.0), pivot=9.0),
                                mass=ia.PowerLaw((0.1, 10.0)), AV=ia.TruncatedGaussian((0.0, 1.0)))
    worst = 0.0
    for model, theta in ((binned, np.random.default_rng(4).uniform(-1.5, 1.5, binned.n_params)),
                         (linked, np.array([0.1, -0.35, 0.3, -2.35, 0.2, 0.3]))):
        host = model.sample(theta, 4099, seed=7)
        dev = model.sample(theta, 4099, seed=7, device="cuda")
        assert list(host) == list(dev) == list(model.columns)
        for c in host:
            assert torch.is_tensor(dev[c]) and dev[c].is_cuda
            got = dev[c].cpu().numpy()
            err = np.abs(got - host[c]) / np.maximum(1.0, np.abs(host[c])) if c != "mass" else np.abs(got - host[c]) / np.abs(host[c])
            worst = max(worst, float(err.max()))
        for c, e in (("age", age_e), ("feh", feh_e)):
            if model is binned:                                               # the bins are equal, not close
                assert np.array_equal(np.searchsorted(e, dev[c].cpu().numpy(), side="right"), np.searchsorted(e, host[c], side="right"))
    print("PopulationModel.sample, device against the host entry: %.3g" % worst)
    assert worst < 1e-11
