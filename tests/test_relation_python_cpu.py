"""LinearGaussian and a coupled PopulationModel without a GPU: the records it packs, the links it refuses, a host chain
through libiso_relation.so's host entry, what a coupled model cannot do yet, and an uncoupled model unchanged to the bit."""
import ctypes as C
import math

import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _hier_cabi as hc, _relation_cabi as rl, hierarchical as hi, priors as P, relations
from isochrones_amd.csrc.libraries import HIER, RELATION
from tests import _hier_twin as tw, _relation_twin as rt


@pytest.fixture(scope="module", autouse=True)
def _built():
    HIER.build()
    RELATION.build()


def _model():
    return ia.PopulationModel(age=ia.TruncatedGaussian((5.0, 10.15)), mass=ia.PowerLaw((0.1, 10.0)),
                              feh=ia.LinearGaussian("age", (-4.0, 0.5), (-1.0, 1.0), pivot=9.6))


def test_exports_names_and_defaults():
    assert ia.LinearGaussian is relations.LinearGaussian and ia.relations is relations
    fam = ia.LinearGaussian("age", (-4.0, 0.5), (-1.0, 1.0))
    assert isinstance(fam, hi._Family) and fam.names == ("intercept", "slope", "sigma") and fam.on == "age" and fam.pivot == 0.0
    tg = ia.TruncatedGaussian((-4.0, 0.5))
    assert fam.ranges == (tg.ranges[0], (-1.0, 1.0), tg.ranges[1])  # TruncatedGaussian's defaults of mean and sigma
    fam = ia.LinearGaussian("age", (-4.0, 0.5), (-1.0, 1.0), intercept=(-1.0, 0.5), sigma=(0.05, 1.0), pivot=9.6)
    assert fam.ranges == ((-1.0, 0.5), (-1.0, 1.0), (0.05, 1.0)) and fam.pivot == 9.6
    m = _model()
    assert m.param_names == ("age.mean", "age.sigma", "mass.alpha", "feh.intercept", "feh.slope", "feh.sigma")
    assert m.coupled and m.parents == (-1, -1, 0)
    plain = ia.PopulationModel(age=ia.TruncatedGaussian((5.0, 10.15)))
    assert not plain.coupled and plain.parents == (-1,)
    for bad in (dict(bounds=(0.5, -4.0)), dict(bounds=(-np.inf, 0.5)), dict(sigma=(0.0, 1.0)), dict(pivot=np.nan)):
        kw = dict(dict(bounds=(-4.0, 0.5)), **bad)
        with pytest.raises(ValueError):
            ia.LinearGaussian("age", kw.pop("bounds"), (-1.0, 1.0), **kw)
    with pytest.raises(TypeError):
        ia.LinearGaussian(0, (-4.0, 0.5), (-1.0, 1.0))


def test_fill_and_pack_set_the_record():
    m = _model()
    theta = np.array([[9.5, 0.3, -2.35, -0.1, 0.2, 0.15], [9.0, 0.5, -1.0, 0.3, -0.7, 0.4]])
    rec = m.pack(theta)
    assert rec.shape == (2, 3) and list(rec["kind"][0]) == [hc.TRUNCGAUSS, hc.POWERLAW, rl.LINGAUSS]
    r = rec[:, 2]
    assert list(r["reserved"]) == [0, 0] and list(rec[:, 0]["reserved"]) == [0, 0]
    assert list(r["lo"]) == [-4.0, -4.0] and list(r["hi"]) == [0.5, 0.5]
    for h, (b0, b1, sg) in enumerate(theta[:, 3:]):
        want = [b0, sg, -math.log(math.sqrt(2 * math.pi)) - math.log(sg), 1.0 / sg, b1, 9.6]
        assert np.allclose(r["p"][h], want, rtol=1e-15, atol=0) and r["p"][h][0] == b0 and r["p"][h][4] == b1
    # the parent's place is what pack writes, whichever side of the child it lies
    m2 = ia.PopulationModel(feh=ia.LinearGaussian("age", (-4.0, 0.5), (-1.0, 1.0)), mass=ia.PowerLaw((0.1, 10.0)),
                            age=ia.TruncatedGaussian((5.0, 10.15)))
    assert m2.parents == (2, -1, -1) and list(m2.pack(np.array([[0.0, 0.1, 0.2, -1.0, 9.0, 0.3]]))["reserved"][0]) == [2, 0, 0]
    # the record is the one the library reads: its density at a point
    lib = rl.lib()
    x, xp, out = np.array([-0.3]), np.array([9.9]), np.zeros(1)
    one = np.ascontiguousarray(rec[0, 2:3])
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.iso_relation_lnpdf_host(p(one), 1, p(x), p(xp), 1, p(out)) == 0
    mu = -0.1 + 0.2 * (9.9 - 9.6)
    from scipy.stats import truncnorm
    assert abs(out[0] - truncnorm.logpdf(-0.3, (-4.0 - mu) / 0.15, (0.5 - mu) / 0.15, loc=mu, scale=0.15)) < 1e-12


def test_lnprior_covers_the_links_ranges():
    m = _model()
    inside = np.array([[9.5, 0.3, -2.35, -0.1, 0.2, 0.15]])
    width = np.prod(m.ranges[:, 1] - m.ranges[:, 0])
    assert m.ranges.shape == (6, 2) and np.isclose(m.lnprior(inside)[0], -math.log(width))
    for k, v in ((3, 0.6), (4, 1.5), (4, -1.5), (5, 1e-4)):
        out = inside.copy()
        out[0, k] = v
        assert np.isneginf(m.lnprior(out)[0]), k


def test_refused_links():
    lg = lambda on: ia.LinearGaussian(on, (-4.0, 0.5), (-1.0, 1.0))
    with pytest.raises(ValueError, match="no column of the model"):
        ia.PopulationModel(feh=lg("age"), mass=ia.PowerLaw((0.1, 10.0)))
    with pytest.raises(ValueError, match="its own column"):
        ia.PopulationModel(feh=lg("feh"), age=ia.TruncatedGaussian((5.0, 10.15)))
    with pytest.raises(ValueError, match="cycle"):
        ia.PopulationModel(feh=lg("age"), age=lg("feh"))
    with pytest.raises(ValueError, match="cycle"):
        ia.PopulationModel(a=lg("b"), b=lg("c"), c=lg("a"), d=ia.TruncatedGaussian((0.0, 1.0)))
    chained = ia.PopulationModel(a=ia.TruncatedGaussian((-4.0, 0.5)), b=lg("a"), c=ia.PowerLaw((0.1, 10.0)), d=lg("b"))
    assert chained.parents == (-1, 0, -1, 1) and chained.coupled


@pytest.fixture(scope="module")
def closed():
    case, exact, slopes, model, theta = rt.closed_form_case()
    S, W, T = case["S"], case["W"], case["T"]
    chain = np.ascontiguousarray(case["x"].reshape(2, S, T, W).transpose(1, 3, 2, 0))      # [S, W, T, D]
    interim = {"x": P.FlatPrior((5.0, 14.0)), "y": P.FlatPrior((-6.0, 6.0))}
    pp = ia.PopulationPosterior((chain, ("x", "y")), None, model, interim=interim)
    return pp, case, exact, slopes, theta


def test_a_host_chain_goes_through_the_host_entry(closed):
    pp, case, exact, slopes, theta = closed
    assert pp.host and pp.model.coupled
    rc, ref = rt.call(rl.lib(), case)
    assert rc == 0
    L, mn, ell, ess, n_bad = pp._evaluate(theta)
    assert all(isinstance(a, np.ndarray) for a in (L, mn, ell, ess, n_bad))
    for got, k in ((L, "L"), (mn, "min_ess"), (ell, "ell"), (ess, "ess"), (n_bad, "n_bad")):
        assert got.tobytes() == ref[k].tobytes(), k
    assert pp.lnlike(theta).tobytes() == L.tobytes() and pp.min_ess(theta).tobytes() == mn.tobytes()
    assert pp.star_terms(theta)[0].tobytes() == ell.tobytes()
    rt.check_closed_form(dict(ell=ell, ess=ess, L=L), exact, slopes, case["W"] * case["T"])
    lp = pp.lnpost(theta)
    assert np.allclose(lp, L + pp.model.lnprior(theta)) and np.isfinite(lp).all()
    outside = theta.copy()
    outside[:, 3] = 5.0                                             # the slope's range is (-2, 2)
    assert np.isneginf(pp.lnpost(outside)).all()
    # the uncoupled library would have read the linked record as an unknown kind
    assert hi.hc.lib() is not rl.lib()


def test_fit_mcmc_on_the_host_route(closed):
    pp = closed[0]
    small = ia.PopulationPosterior((pp.storage.reshape(pp.T, 2, pp.S, pp.W)[:, :, :20].transpose(2, 3, 0, 1), ("x", "y")), None,
                                   pp.model, interim={"x": P.FlatPrior((5.0, 14.0)), "y": P.FlatPrior((-6.0, 6.0))})
    smp = small.fit_mcmc(nwalkers=12, nburn=3, niter=3, seed=1)
    df = small.samples
    assert list(df.columns) == list(pp.model.param_names) + ["lnprob"] and len(df) == 36 and np.isfinite(df["lnprob"]).all()
    assert smp is small.sampler


def test_what_a_coupled_model_cannot_do_yet(closed):
    pp = closed[0]
    theta = closed[4]
    with pytest.raises(ValueError, match="uncoupled.*y on x"):
        pp.star_posteriors(theta)
    with pytest.raises(ValueError, match="uncoupled.*y on x"):
        pp.star_weights(theta)
    with pytest.raises(ValueError, match="y on x.*injection set"):
        ia.PopulationPosterior((np.zeros((2, 4, 3, 2)), ("x", "y")), None, pp.model,
                               interim={"x": P.FlatPrior((5.0, 14.0)), "y": P.FlatPrior((-6.0, 6.0))}, injections=object())


def test_an_uncoupled_model_is_unchanged_to_the_bit():
    case = tw.random_case(4, 5, 7, 2, 6, seed=4)
    S, W, T = case["S"], case["W"], case["T"]
    chain = np.ascontiguousarray(case["x"].reshape(2, S, T, W).transpose(1, 3, 2, 0))
    model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0)), feh=ia.TruncatedGaussian((-4.0, 0.5)))
    interim = {"mass": P.PowerLawPrior(-2.35, (0.1, 10.0)), "feh": P.FlatPrior((-4.0, 0.5))}
    pp = ia.PopulationPosterior((chain, ("mass", "feh")), None, model, interim=interim)
    assert not model.coupled
    rng = np.random.default_rng(0)
    theta = np.column_stack([rng.uniform(-3.0, 0.5, 6), rng.uniform(-0.5, 0.2, 6), rng.uniform(0.1, 0.6, 6)])
    ref = dict(case, interim=pp.interim, rows=model.pack(theta), storages=[pp.storage], where=[(0, 2, 0), (0, 2, 1)])
    rc, want = tw.call(hc.lib(), ref)
    assert rc == 0
    assert pp.lnlike(theta).tobytes() == want["L"].tobytes() and pp.star_terms(theta)[0].tobytes() == want["ell"].tobytes()
    assert (model.pack(theta)["reserved"] == 0).all()
