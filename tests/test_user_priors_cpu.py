"""CPU: a user's priors (oracle/user_priors.py) on this build's base classes against what the reference's base classes made
of the SAME user code (the ``user_<parameter>_lnpdf`` / ``_call`` vectors of the user-prior fixtures, written by
oracle/make_golden.py), on the priors' bounds and one ulp outside them included; which prior objects take the device route
(priors.is_host_prior); and that everything fitted inside the kernels refuses a subclass of a device family that overrides
its density instead of evaluating its parent.

The fixtures' priors all return -inf outside their own bounds: the reference's ``BasicStarModel.lnprior`` applies no bounds
test of its own, this build applies the bounds in the kernel (priors.flat_stand_in); that documented difference is kept out
of the fixtures."""
import math

import numpy as np
import pytest

from isochrones_amd import priors as P
from oracle import user_priors
from tests import _fixtures as fx

USER = user_priors.make(P)


def _user_terms():
    for case in fx.USER_PRIOR_CASES:
        for par in fx.load(case)["meta"]["priors"]:
            yield case, par


@pytest.mark.parametrize("case,par", list(_user_terms()))
def test_user_prior_equals_the_reference_term_by_term(case, par):
    g = fx.load(case)
    meta = g["meta"]
    prior = fx.make_prior(meta["priors"][par])
    col = meta["param_names"].index(par)
    x = g["pars"][:, col]
    with np.errstate(all="ignore"):
        got = np.array([prior.lnpdf(float(v)) for v in x], dtype=float)
    # same user code, same arithmetic, the normalisation from the same quadrature: the last bits only (an absolute term
    # for log-densities that pass through zero)
    fx.assert_close(got, g["user_%s_lnpdf" % par], 1e-13, atol=1e-14, what="lnpdf")
    fx.assert_close(P.lnpdf_array(prior, x), g["user_%s_lnpdf" % par], 1e-13, atol=1e-14, what="lnpdf_array")
    if "user_%s_call" % par in g:
        with np.errstate(all="ignore"):
            got = np.array([prior(float(v)) for v in x], dtype=float)
        fx.assert_close(got, g["user_%s_call" % par], 1e-13, what="__call__")
        fx.assert_close(prior.pdf_array(x), g["user_%s_call" % par], 1e-13, what="pdf_array")
    # the fixture holds the edges: on the bounds finite, one ulp outside -inf
    lo, hi = prior.bounds
    want = g["user_%s_lnpdf" % par]
    for v, fin in ((lo, True), (hi, True), (np.nextafter(lo, -np.inf), False), (np.nextafter(hi, np.inf), False)):
        rows = np.flatnonzero(x == v)
        assert rows.size, (par, v)
        assert np.all(np.isfinite(want[rows]) if fin else np.isneginf(want[rows])), (par, v, want[rows])


class OnlyInit(P.GaussianPrior):
    def __init__(self):
        super().__init__(1.0, 2.0, bounds=(-3.0, 5.0))


class OnlySample(P.PowerLawPrior):
    def sample(self, n, rng=None):
        return np.full(n, self.bounds[0])


class Bare(P.ChabrierPrior):
    pass


class SkewChild(USER["Skew"]):
    pass


class OwnKind(P.FlatPrior):
    bounded = 0


def _overriding():
    return [USER["Skew"](0.0, 1.0, bounds=(-2.0, 2.0)), USER["Tilt"]((0.0, 1.0)), USER["Over"](2.0, (1.0, 10.0))]


def test_host_and_device_classification():
    own = [P.FlatPrior((0, 1)), P.FlatLogPrior((0, 1)), P.PowerLawPrior(1.5, (1, 2)), P.GaussianPrior(0, 1),
           P.GaussianPrior(0, 1, bounds=(-1, 1)), P.LogNormalPrior(0, 1), P.ChabrierPrior(), P.FehPrior(), P.AgePrior(),
           P.DistancePrior(), P.AVPrior(), P.QPrior(), P.SalpeterPrior(),
           P.BrokenPrior([P.LogNormalPrior(-1.0, 0.5), P.PowerLawPrior(-2.0, (0.5, 5.0))], [0.9], (0.3, 5.0))]
    # every prior class priors.py defines (the base class has no family) stays a device prior
    classes = [c for c in vars(P).values() if isinstance(c, type) and issubclass(c, P.Prior) and c is not P.Prior
               and c.__module__ == P.__name__]
    assert {type(p) for p in own} == set(classes)
    for p in own:
        assert not P.is_host_prior(p), p
    for p in (OnlyInit(), OnlySample(2.0, (1.0, 3.0)), Bare()):
        assert not P.is_host_prior(p), p
        assert type(p).lnpdf is type(p).__mro__[1].lnpdf               # nothing was installed on them
    for p in _overriding() + [SkewChild(0.0, 1.0, bounds=(-2.0, 2.0)), OwnKind((0.0, 1.0)), USER["Triangle"]((0.0, 1.0)),
                              USER["ForeignExp"](3.0, (0.0, 1.0)), object(), 1.0]:
        assert P.is_host_prior(p), p
    # decided once per class
    assert P._DEVICE_ROUTE[USER["Skew"]] is False and P._DEVICE_ROUTE[P.AVPrior] is True


def test_overriding_subclasses_resolve_as_the_reference_does():
    skew, tilt, over = _overriding()
    z = 0.5
    assert skew.lnpdf(0.5) == -0.5 * z * z - skew.lognorm + math.log1p(0.5 * math.tanh(z))     # its _lnpdf ...
    assert skew.lnpdf(2.5) == -math.inf and skew.lnpdf(-2.5) == -math.inf                       # ... behind the bounds test
    assert skew(0.5) == P.GaussianPrior(0.0, 1.0, bounds=(-2.0, 2.0))(0.5)                      # (pdf: no _pdf of its own)
    assert tilt.lnpdf(0.75) == math.log(1.0 + 0.6 * 0.25) and tilt(0.75) == 1.0 + 0.6 * 0.25    # log of its _pdf
    assert tilt.lnpdf(1.5) == -math.inf and tilt(1.5) == 0.0
    assert np.array_equal(tilt.pdf_array(np.array([0.75, 1.5])), [1.15, 0.0])
    assert over.lnpdf(5.0) == -math.log(9.0) + 0.25 * math.sin(5.0 / 40.0) and over.lnpdf(0.5) == -math.inf
    # a subclass that only writes _pdf under a family whose lnpdf is a closed form of its own keeps that lnpdf, as the
    # reference (its GaussianPrior._lnpdf is found before the log of the pdf is tried)

    class Bump(P.GaussianPrior):
        def _pdf(self, x):
            return 7.0

    b = Bump(0.0, 1.0, bounds=(-1.0, 1.0))
    assert b(0.5) == 7.0 and b.lnpdf(0.5) == P.GaussianPrior(0.0, 1.0, bounds=(-1.0, 1.0)).lnpdf(0.5)
    assert P.is_host_prior(b)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_everything_fitted_in_the_kernels_refuses_an_overriding_subclass(which):
    import isochrones_amd as ia
    from isochrones_amd import draws, hierarchical, selection
    from isochrones_amd.starmodel import EEPPrior
    p = _overriding()[which]
    with pytest.raises(ValueError, match="evaluated on the host"):
        hierarchical.prior_record(p)
    with pytest.raises(ValueError, match="evaluated on the host"):
        hierarchical.Fixed(p)
    with pytest.raises(TypeError, match="column of a DrawPlan"):
        draws.DrawPlan({"x": p})
    with pytest.raises(ValueError, match="evaluated on the host"):
        selection.InjectionSet({"x": np.linspace(1.0, 2.0, 8)}, {"x": p}, np.zeros(8))
    ic = ia.synthetic_track(bands=("V",), fehs=[-1.0, 0.5], masses=[0.5, 2.0], eeps=np.arange(1.0, 6.0))
    eep = EEPPrior(ic, P.AgePrior())
    with pytest.raises(NotImplementedError, match="not evaluable on the device"):
        eep.orig_prior = p
    eep.orig_prior = OnlyInit()
    import pandas as pd
    cat = ia.StarCatalog(pd.DataFrame(dict(V_mag=[10.0, 11.0], V_mag_unc=[0.02, 0.02])), bands=["V"])
    with pytest.raises(NotImplementedError, match="catalog"):
        cat.set_prior(feh=p)
    cat.set_prior(feh=OnlyInit())
