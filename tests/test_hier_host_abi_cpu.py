"""libiso_hier.so's host entries through ctypes, no GPU needed: iso_hier_lnpdf_host family by family against
isochrones_amd.priors (1e-12 absolute where finite, the -inf and NaN pattern identical), TRUNCGAUSS against a long-double
erf form, and iso_hier_lnlike_host against the long-double twin within the twin's limits."""
import ctypes as C
import math

import numpy as np
import pytest

from isochrones_amd import _cabi, _hier_cabi as hc, hierarchical as hi, priors as P
from isochrones_amd.csrc.libraries import HIER as build_hier
from tests import _hier_twin as tw


@pytest.fixture(scope="module")
def lib():
    build_hier.build()
    return hc.lib()


def _lnpdf(lib, rec, x):
    rec, x = np.ascontiguousarray(rec), np.ascontiguousarray(x, dtype=np.float64)
    out = np.full((rec.shape[0], x.size), -7.0)
    rc = lib.iso_hier_lnpdf_host(C.c_void_p(rec.ctypes.data), rec.shape[0], C.c_void_p(x.ctypes.data), x.size,
                                 C.c_void_p(out.ctypes.data))
    assert rc == 0, lib.iso_hier_last_error()
    return out


def _points(lo, hi, extra=()):
    """inside the bounds, at them and outside them"""
    lo_f, hi_f = (lo if np.isfinite(lo) else -3.0), (hi if np.isfinite(hi) else 8.0)
    span = hi_f - lo_f
    pts = list(np.linspace(lo_f, hi_f, 23)) + [lo_f, hi_f, np.nextafter(lo_f, -np.inf), np.nextafter(hi_f, np.inf),
                                               lo_f - 0.3 * span, hi_f + 0.3 * span] + list(extra)
    return np.array(pts, dtype=float)


FAMILIES = {
    "flat": (P.FlatPrior((-1.5, 2.5)), ()),
    "flatlog": (P.FlatLogPrior((5.0, 10.15)), ()),
    "age": (P.AgePrior(), ()),
    "powerlaw": (P.PowerLawPrior(-2.35, (0.1, 10.0)), ()),
    "salpeter": (P.SalpeterPrior(), ()),
    "distance": (P.DistancePrior(3000.0), ()),
    "gauss": (P.GaussianPrior(0.3, 0.7), (-40.0, 45.0)),
    "gauss_bounded": (P.GaussianPrior(0.3, 0.7, bounds=(-1.0, 1.0)), ()),
    "lognormal": (P.LogNormalPrior(math.log(0.079), 0.69 * math.log(10)), (1e-3, 0.079, 50.0)),
    # the break itself, the doubles next to it, the power law's bounds and beyond them
    "chabrier": (P.ChabrierPrior(), (1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.5, 99.0, 100.0, 150.0)),
    "chabrier_narrow": (P.ChabrierPrior(bounds=(0.1, 10.0)), (1.0, 0.2, 5.0, 150.0)),
    # the halo term dominates below -1: points there
    "feh": (P.FehPrior(), (-2.5, -1.5, -1.0, 0.016)),
    "feh_bounded": (P.FehPrior(bounds=(-4.0, 0.5)), (-2.5, -1.5, -1.0)),
    "feh_halo": (P.FehPrior(halo_fraction=0.3, bounds=(-4.0, 0.5)), (-2.5, -1.5)),
    "feh_not_local": (P.FehPrior(local=False, bounds=(-4.0, 0.5)), (-2.5, -0.3)),
}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_lnpdf_host_against_priors(lib, name):
    prior, extra = FAMILIES[name]
    lo, hi_ = prior.bounds
    x = _points(lo, hi_, extra)
    with np.errstate(all="ignore"):
        want = np.array([prior.lnpdf(float(v)) for v in x], dtype=float)
    got = _lnpdf(lib, hi.prior_record(prior), x)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)), name
    fin = np.isfinite(want)
    assert fin.sum() >= 10 and np.isneginf(want).any() == (name not in ("gauss", "lognormal", "feh")), name
    print(name, "max |d| = %.2e" % np.max(np.abs(got[fin] - want[fin])))
    assert np.max(np.abs(got[fin] - want[fin])) <= 1e-12, name


def test_unknown_kind_is_nan(lib):
    rec = hi.records(1)
    rec["kind"], rec["lo"], rec["hi"] = 99, -1.0, 1.0
    assert np.isnan(_lnpdf(lib, rec, [0.0, 2.0])).all()


@pytest.mark.parametrize("bounds, mean, sigma", [((-4.0, 4.0), -0.2, 0.15), ((-4.0, 0.5), 0.4, 0.3), ((0.0, 1.0), 3.0, 0.5),
                                                 ((0.0, 1.0), -2.0, 0.4), ((5.0, 10.15), 9.7, 2.0)])
def test_truncgauss_against_long_double_erf(lib, bounds, mean, sigma):
    """ln N(x; mean, sigma) - ln(Phi(b) - Phi(a)) with the mass from mpmath's erfc at 40 digits, the rest in long double"""
    import mpmath
    mpmath.mp.dps = 40
    lo, hi_ = bounds
    a, b = (mpmath.mpf(lo) - mean) / sigma, (mpmath.mpf(hi_) - mean) / sigma
    mass = (mpmath.erfc(-b / mpmath.sqrt(2)) - mpmath.erfc(-a / mpmath.sqrt(2))) / 2
    LD = np.longdouble
    lnmass = LD(str(mpmath.nstr(mpmath.log(mass), 30)))
    x = _points(lo, hi_)
    z = (x.astype(LD) - LD(mean)) / LD(sigma)
    want = -(z * z) / 2 - np.log(np.sqrt(2 * LD(np.pi))) - np.log(LD(sigma)) - lnmass
    want = np.where((x < lo) | (x > hi_), -np.inf, want).astype(float)
    rec = hi.records(1)
    hi.TruncatedGaussian(bounds, mean=(-10.0, 10.0), sigma=(0.01, 10.0)).fill(rec, np.array([[mean, sigma]]))
    assert rec["kind"][0] == hc.TRUNCGAUSS
    got = _lnpdf(lib, rec, x)[0]
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.isneginf(want).sum() == 4
    fin = np.isfinite(want)
    # the record's arithmetic in float64: z * z / 2 carries 2 ulp of its size
    lim = 1e-12 * np.maximum(1.0, np.abs(want[fin]) / 100.0)
    assert np.all(np.abs(got[fin] - want[fin]) <= lim)
    # it integrates to one on its bounds
    grid = np.linspace(lo, hi_, 20001)
    pdf = np.exp(_lnpdf(lib, rec, grid)[0])
    assert abs(np.sum((pdf[1:] + pdf[:-1]) / 2 * np.diff(grid)) - 1.0) < 1e-6


def test_powerlaw_family_against_the_prior_class(lib):
    fam = hi.PowerLaw((0.1, 10.0))
    alphas = np.array([-3.0, -2.35, -1.0 - 1e-9, -1.0, -1.0 + 1e-7, 0.0, 0.3, 2.0])
    rec = hi.records(alphas.size)
    fam.fill(rec, alphas[:, None])
    x = _points(0.1, 10.0)
    got = _lnpdf(lib, rec, x)
    inside = (x >= 0.1) & (x <= 10.0)
    for i, a in enumerate(alphas):
        if abs(a + 1.0) > 1e-3:
            want = np.array([P.PowerLawPrior(a, (0.1, 10.0)).lnpdf(float(v)) for v in x])
            assert np.array_equal(np.isneginf(got[i]), np.isneginf(want))
            assert np.max(np.abs(got[i][inside] - want[inside])) <= 1e-12
    # alpha = -1: 1 / (x ln(hi / lo)); its neighbours are continuous with it
    k = list(alphas).index(-1.0)
    assert np.max(np.abs(got[k][inside] - (-np.log(x[inside]) - math.log(math.log(100.0))))) <= 1e-12
    assert np.max(np.abs(got[k - 1][inside] - got[k][inside])) < 1e-7 and np.max(np.abs(got[k + 1][inside] - got[k][inside])) < 1e-5


SHAPES = [(Q, H, layout, split) for Q in (1, 2, 3, 4) for H in (1, 17)
          for layout, split in ((_cabi.CHAIN_PARAM_MAJOR, True), (_cabi.CHAIN_ROW_MAJOR, True))]


@pytest.mark.parametrize("Q, H, layout, split", SHAPES)
def test_lnlike_host_matches_the_twin(lib, Q, H, layout, split):
    case = tw.random_case(3, 5, 7, Q, H, seed=10 * Q + H, layout=layout, split=split)
    assert Q == 1 or len({w[1] for w in case["where"]}) == 2         # columns from two storages with different C
    rc, got = tw.call(lib, case)
    assert rc == 0, lib.iso_hier_last_error()
    want = tw.want(case)
    assert np.isfinite(want["ell"]).all() and (want["ess"] > 1).all()
    tw.assert_matches(got, want, (Q, H, layout))


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_interim_and_as_population(lib, kind):
    case = tw.kind_case(kind)
    rc, got = tw.call(lib, case)
    assert rc == 0, lib.iso_hier_last_error()
    tw.assert_matches(got, tw.want(case), kind)


def test_special_cases(lib):
    cases = tw.special_cases()
    res = {}
    for name, case in cases.items():
        rc, got = tw.call(lib, case)
        assert rc == 0, lib.iso_hier_last_error()
        tw.assert_matches(got, tw.want(case), name)
        res[name] = got
    g = res["no_support"]
    assert np.isneginf(g["ell"][0, 1]) and g["ess"][0, 1] == 0.0 and np.isfinite(g["ell"][1]).all()
    assert np.isneginf(g["L"][0]) and g["min_ess"][0] == 0.0 and np.isfinite(g["L"][1])
    g = res["nan"]
    assert list(g["n_bad"]) == [1, 0, 2] and np.isfinite(g["ell"]).all()
    g = res["masked"]
    assert np.isnan(g["ell"][:, 1]).all() and np.isnan(g["ess"][:, 1]).all() and g["n_bad"][1] == 0
    assert np.allclose(g["L"], g["ell"][:, [0, 2]].sum(axis=1), rtol=0, atol=1e-12) and np.isfinite(g["min_ess"]).all()
    g, w = res["span_700"], tw.want(cases["span_700"])
    assert w["rmax"].max() > 690 and np.isfinite(g["ell"]).all() and np.isfinite(g["ess"]).all()
    # without the max subtraction the weights' squares overflow
    x = cases["span_700"]["x"][0, 0]
    with np.errstate(over="ignore"):
        assert np.isinf(np.sum(np.exp(x * x / 2 - (x - 37.4) ** 2 / 2) ** 2))


def test_sub_range_writes_only_its_stars(lib):
    case = tw.random_case(3, 5, 7, 2, 3, seed=3)
    rc, whole = tw.call(lib, case)
    rc2, part = tw.call(lib, case, ens_begin=1, n_ens_out=1, total=False)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(part["ell"][:, 1], whole["ell"][:, 1]) and np.array_equal(part["ess"][:, 1], whole["ess"][:, 1])
    assert (part["ell"][:, [0, 2]] == -7.0).all() and (part["n_bad"][[0, 2]] == -7).all() and (part["L"] == -7.0).all()


def test_refused_arguments(lib):
    case = tw.random_case(3, 5, 7, 2, 3, seed=3)
    S, W, T = 3, 5, 7
    st = case["storages"]
    rows, interim = np.ascontiguousarray(case["rows"]), np.ascontiguousarray(case["interim"])
    out = [np.zeros((3, S)), np.zeros((3, S)), np.zeros(S, np.int32), np.zeros(3), np.zeros(3)]
    p = lambda a: C.c_void_p(a.ctypes.data)
    good_cols = [hc.IsoHierColumn(st[k].ctypes.data, n, c, S, 0) for k, n, c in case["where"]]

    def run(cols=None, Q=2, layout=_cabi.CHAIN_PARAM_MAJOR, nsteps=T, n_ens=S, W_=W, b=0, n=S, H=3, L=True, mn=True,
            interim_=True, fn=lib.iso_hier_lnlike_host):
        arr = (hc.IsoHierColumn * 4)(*(cols or good_cols))
        rc = fn(arr, Q, layout, nsteps, n_ens, W_, b, n, p(interim) if interim_ else None, p(rows), H, None, p(out[0]),
                p(out[1]), p(out[2]), p(out[3]) if L else None, p(out[4]) if mn else None, None)
        return rc, (lib.iso_hier_last_error() or b"").decode()

    assert run()[0] == 0
    for kw, text in ((dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(layout=7), "layout"),
                     (dict(nsteps=0), "at least 1"), (dict(H=0), "H must be"), (dict(b=2, n=2), "ensemble range"),
                     (dict(n=0), "ensemble range"), (dict(L=False), "both or neither"), (dict(interim_=False), "null pointer"),
                     (dict(cols=[hc.IsoHierColumn(st[0].ctypes.data, 4, 4, S, 0)] * 2), "column index"),
                     (dict(cols=[hc.IsoHierColumn(0, 4, 1, S, 0)] * 2), "null column"),
                     (dict(cols=[hc.IsoHierColumn(st[0].ctypes.data, 4, 1, 2, 0)] * 2), "does not hold"),
                     (dict(cols=[hc.IsoHierColumn(st[0].ctypes.data, 4, 1, S, 1)] * 2), "does not hold")):
        rc, msg = run(**kw)
        assert rc == hc.ERR_INVALID and text in msg and msg.startswith("iso_hier_lnlike_host: "), (kw, msg)
    # the device entry refuses the same before it touches a device
    rc, msg = run(Q=5, fn=lib.iso_hier_lnlike)
    assert rc == hc.ERR_INVALID and msg.startswith("iso_hier_lnlike: ")
    assert lib.iso_hier_lnpdf_host(None, 1, None, 1, None) == hc.ERR_INVALID
