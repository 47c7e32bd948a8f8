"""libiso_select.so's host entries through ctypes, no GPU needed: iso_select_alpha_host against the long-double twin within
the twin's limits, iso_select_lnpdf_host bit for bit equal to iso_hier_lnpdf_host, and with 0/1 detection against the route
that already existed (iso_hier_lnlike_host on the one-star chain of the detected injections)."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _hier_cabi as hc, _select_cabi as sc, hierarchical as hi, priors as P
from isochrones_amd.csrc.libraries import HIER as build_hier, SELECT as build_select
from tests import _hier_twin as ht, _select_twin as tw
from tests.test_hier_host_abi_cpu import FAMILIES, _points


@pytest.fixture(scope="module")
def lib():
    build_select.build()
    return sc.lib()


@pytest.fixture(scope="module")
def hlib():
    build_hier.build()
    return hc.lib()


def _lnpdf(fn, rec, x):
    rec, x = np.ascontiguousarray(rec), np.ascontiguousarray(x, dtype=np.float64)
    out = np.full((rec.shape[0], x.size), -7.0)
    assert fn(C.c_void_p(rec.ctypes.data), rec.shape[0], C.c_void_p(x.ctypes.data), x.size, C.c_void_p(out.ctypes.data)) == 0
    return out


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_lnpdf_host_is_the_hier_library_s_bit_for_bit(lib, hlib, name):
    prior, extra = FAMILIES[name]
    x = _points(*prior.bounds, extra)
    rec = hi.prior_record(prior)
    got, want = _lnpdf(lib.iso_select_lnpdf_host, rec, x), _lnpdf(hlib.iso_hier_lnpdf_host, rec, x)
    assert np.isfinite(want).sum() >= 10
    assert got.tobytes() == want.tobytes(), name


def test_lnpdf_host_of_the_families_with_free_parameters_and_an_unknown_kind(lib, hlib):
    rec = hi.PopulationModel(a=hi.PowerLaw((0.1, 10.0)), b=hi.TruncatedGaussian((0.1, 10.0))).pack(
        np.array([[-2.35, 1.0, 0.7], [-1.0, 0.3, 2.0], [0.4, 9.0, 0.05]])).reshape(-1)
    bad = hi.records(1)
    bad["kind"], bad["lo"], bad["hi"] = 99, -1.0, 1.0
    rec = np.concatenate([rec, bad])
    x = _points(0.1, 10.0, (-1.0, 0.0, np.nan))
    got, want = _lnpdf(lib.iso_select_lnpdf_host, rec, x), _lnpdf(hlib.iso_hier_lnpdf_host, rec, x)
    assert got.tobytes() == want.tobytes() and np.isnan(got[-1]).all()
    assert lib.iso_select_lnpdf_host(None, 1, None, 1, None) == sc.ERR_INVALID


SHAPES = [(J, Q, H) for J in (1, 37, 300, 4097) for Q, H in ((1, 1), (2, 9), (3, 17), (4, 8))]


@pytest.mark.parametrize("J, Q, H", SHAPES)
def test_alpha_host_matches_the_twin(lib, J, Q, H):
    case = tw.random_case(J, Q, H, seed=10 * Q + H + J)
    if J == 1:
        case["lnd"][:] = np.log(0.5)
    rc, got = tw.call(lib, case)
    assert rc == 0, lib.iso_select_last_error()
    want = tw.want(case)
    assert np.isfinite(want["ln_alpha"]).all() and want["n_bad"] == 0 and (J < 300 or (want["n_eff"] > 2).all())
    print((J, Q, H), "max |d ln_alpha| = %.2e" % np.max(np.abs(got["ln_alpha"] - want["ln_alpha"])))
    tw.assert_matches(got, want, (J, Q, H))


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_draw_and_as_population(lib, kind):
    case = tw.kind_case(kind)
    rc, got = tw.call(lib, case)
    assert rc == 0, lib.iso_select_last_error()
    assert np.isfinite(tw.want(case)["ln_alpha"]).all()
    tw.assert_matches(got, tw.want(case), kind)


def test_special_cases(lib):
    cases = tw.special_cases()
    keep, n_removed = cases.pop("bad_removed")
    res = {}
    for name, case in cases.items():
        rc, got = tw.call(lib, case)
        assert rc == 0, lib.iso_select_last_error()
        tw.assert_matches(got, tw.want(case), name)
        res[name] = got
    g = res["none_detected"]
    assert np.isneginf(g["ln_alpha"]).all() and (g["n_eff"] == 0.0).all() and g["n_bad"] == 0
    # the bad injections are counted and change nothing else: the sums are those of the set without them, J stays J
    g, clean = res["bad"], cases["bad"]
    assert g["n_bad"] == n_removed and res["clean"]["n_bad"] == 0
    without = tw.fixed_case(clean["x"][:, keep], clean["lnd"][keep], list(clean["draw"][:, None]),
                            [[row[q:q + 1] for q in range(len(row))] for row in clean["rows"]])
    rc, w = tw.call(lib, without)
    J = keep.size
    assert rc == 0 and w["n_bad"] == 0
    assert np.array_equal(g["n_eff"], w["n_eff"])
    assert np.max(np.abs(g["ln_alpha"] - (w["ln_alpha"] + np.log(keep.sum() / J)))) <= 1e-13
    g = res["no_support"]
    assert np.isneginf(g["ln_alpha"][0]) and g["n_eff"][0] == 0.0 and np.isfinite(g["ln_alpha"][1]) and g["n_eff"][1] > 1
    g, w = res["span_700"], tw.want(cases["span_700"])
    assert w["tmax"].max() > 690 and np.isfinite(g["ln_alpha"]).all() and np.isfinite(g["n_eff"]).all()
    x = cases["span_700"]["x"][0]
    with np.errstate(over="ignore"):                                # without the max subtraction the squares overflow
        assert np.isinf(np.sum(np.exp(x * x / 2 - (x - 37.4) ** 2 / 2) ** 2))


@pytest.mark.parametrize("J, Q, H", [(300, 1, 9), (4097, 3, 17)])
def test_zero_one_detection_is_the_hier_entry_on_the_one_star_chain(lib, hlib, J, Q, H):
    """ln_alpha = ell of the detected injections as one star's samples + ln(J_det / J), n_eff = its ess: twice the twin's
    limits, since the two results are rounded independently"""
    case = tw.random_case(J, Q, H, seed=J + Q)
    case["lnd"] = np.where(np.random.default_rng(J).random(J) < 0.6, 0.0, -np.inf)
    rc, got = tw.call(lib, case)
    assert rc == 0, lib.iso_select_last_error()
    hcase, shift = tw.one_star_chain(case)
    rc, old = ht.call(hlib, hcase)
    assert rc == 0, hlib.iso_hier_last_error()
    want = dict(ln_alpha=old["ell"][:, 0] + shift, n_eff=old["ess"][:, 0], tmax=tw.want(case)["tmax"])
    assert old["n_bad"][0] == got["n_bad"] == 0 and np.isfinite(want["ln_alpha"]).all()
    tw.assert_matches(got, want, (J, Q, H), factor=2.0)
    assert np.array_equal(old["L"], old["ell"][:, 0])


def test_refused_arguments(lib):
    case = tw.random_case(37, 2, 3, seed=3)
    x, lnd, draw, rows = (np.ascontiguousarray(case[k]) for k in ("x", "lnd", "draw", "rows"))
    out = [np.zeros(3), np.zeros(3), np.zeros(1, np.int32)]
    p = lambda a: C.c_void_p(a.ctypes.data)

    def run(Q=2, J=37, H=3, x_=True, lnd_=True, draw_=True, rows_=True, la=True, ne=True, nb=True, ws=None,
            fn=lib.iso_select_alpha_host):
        rc = fn(p(x) if x_ else None, Q, J, p(lnd) if lnd_ else None, p(draw) if draw_ else None, p(rows) if rows_ else None,
                H, ws, p(out[0]) if la else None, p(out[1]) if ne else None, p(out[2]) if nb else None, None)
        return rc, (lib.iso_select_last_error() or b"").decode()

    assert run()[0] == 0
    for kw, text in ((dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(H=0), "H must be"),
                     (dict(J=0), "J must be"), (dict(J=2 ** 31), "J must be"), (dict(x_=False), "null pointer"),
                     (dict(lnd_=False), "null pointer"), (dict(draw_=False), "null pointer"), (dict(rows_=False), "null pointer"),
                     (dict(la=False), "null pointer"), (dict(ne=False), "null pointer"), (dict(nb=False), "null pointer")):
        rc, msg = run(**kw)
        assert rc == sc.ERR_INVALID and text in msg and msg.startswith("iso_select_alpha_host: "), (kw, msg)
    # the device entry refuses the same, and a missing workspace, before it touches a device
    rc, msg = run(Q=5, ws=p(out[0]), fn=lib.iso_select_alpha)
    assert rc == sc.ERR_INVALID and msg.startswith("iso_select_alpha: ") and "Q must be" in msg
    rc, msg = run(fn=lib.iso_select_alpha)
    assert rc == sc.ERR_INVALID and "null pointer" in msg
