"""libiso_relation.so's host entries through ctypes, no GPU needed: iso_relation_lnpdf_host bit for bit equal to
iso_hier_lnpdf_host on the kinds 1 .. 8, the linked kind against mpmath at 40 digits, iso_relation_lnlike_host against the
long-double twin within the twin's limits, the special cases, the closed-form case and the refusals."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _cabi, _hier_cabi as hc, _relation_cabi as rl, hierarchical as hi
from isochrones_amd.csrc.libraries import HIER as build_hier, RELATION as build_relation
from tests import _hier_twin as tw, _relation_twin as rt

PM, RM = _cabi.CHAIN_PARAM_MAJOR, _cabi.CHAIN_ROW_MAJOR
TILE = rl.ROW_TILE


@pytest.fixture(scope="module")
def lib():
    build_relation.build()
    return rl.lib()


def _lnpdf(lib, rec, x, xp=None):
    rec, x = np.ascontiguousarray(rec), np.ascontiguousarray(x, dtype=np.float64)
    xp = None if xp is None else np.ascontiguousarray(xp, dtype=np.float64)
    out = np.full((rec.shape[0], x.size), -7.0)
    rc = lib.iso_relation_lnpdf_host(C.c_void_p(rec.ctypes.data), rec.shape[0], C.c_void_p(x.ctypes.data),
                                     C.c_void_p(0 if xp is None else xp.ctypes.data), x.size, C.c_void_p(out.ctypes.data))
    assert rc == 0, lib.iso_relation_last_error()
    return out


def test_kinds_1_to_8_equal_the_hier_library_bit_for_bit(lib):
    build_hier.build()
    hlib = hc.lib()
    kinds = tw.all_kinds()
    rec = np.concatenate([kinds[k] for k in range(1, 9)] + [hi.records(1)])
    rec["kind"][-1] = 99                                            # unknown: NaN in both
    x = np.concatenate([np.linspace(-5.0, 12.0, 400), [0.0, -0.0, 0.1, 10.0, 1.0, np.nextafter(1.0, 0.0), np.nan, np.inf, -np.inf]])
    want = np.full((rec.shape[0], x.size), -7.0)
    assert hlib.iso_hier_lnpdf_host(C.c_void_p(rec.ctypes.data), rec.shape[0], C.c_void_p(x.ctypes.data), x.size,
                                    C.c_void_p(want.ctypes.data)) == 0
    for xp in (None, np.zeros_like(x)):
        got = _lnpdf(lib, rec, x, xp)
        assert got.tobytes() == want.tobytes()
    assert np.isnan(want[-1]).all() and np.isfinite(want[:-1]).sum() > 1000


def test_linked_kind_against_mpmath(lib):
    """2 000 (record, x, xp): the header's definition in mpmath at 40 digits from the record's own doubles; the means reach
    30 sigma outside the bounds, where the mass is some 1e-198"""
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(31)
    n = 2000
    lo, hi_ = -4.0, 0.5
    sigma = rng.uniform(0.03, 1.5, n)
    off = rng.uniform(-30.0, 30.0, n) * (rng.random(n) < 0.5)       # half of the means inside the bounds
    mean = np.where(off > 0, hi_ + off * sigma, np.where(off < 0, lo + off * sigma, rng.uniform(lo, hi_, n)))
    slope, pivot, xp = rng.uniform(-1.0, 1.0, n), 9.6, rng.uniform(8.5, 10.1, n)
    intercept = mean - slope * (xp - pivot)
    x = rng.uniform(lo, hi_, n)
    rec = hi.records(n)
    from isochrones_amd.relations import LinearGaussian
    LinearGaussian("age", (lo, hi_), (-1.0, 1.0), pivot=pivot).fill(rec, np.column_stack([intercept, slope, sigma]))
    assert (rec["kind"] == rl.LINGAUSS).all()
    got = np.array([_lnpdf(lib, rec[i:i + 1], x[i:i + 1], xp[i:i + 1])[0, 0] for i in range(n)])
    mp = mpmath.mpf
    want = np.empty(n)
    far = 0
    for i in range(n):
        r = rec[i]
        mu = mp(r["p"][0]) + mp(r["p"][4]) * (mp(xp[i]) - mp(r["p"][5]))
        sg = mp(r["p"][1])
        a, b = (mp(lo) - mu) / sg, (mp(hi_) - mu) / sg
        if a > 0:                                                   # the same mass, free of 2 - 2 at any precision
            a, b = -b, -a
        mass = (mpmath.erfc(-b / mpmath.sqrt(2)) - mpmath.erfc(-a / mpmath.sqrt(2))) / 2
        z = (mp(x[i]) - mu) / sg
        want[i] = float(-z * z / 2 - mpmath.log(mpmath.sqrt(2 * mpmath.pi)) - mpmath.log(sg) - mpmath.log(mass))
        far += mass < 1e-100
    assert far > 50 and np.isfinite(got).all()
    d = np.abs(got - want)
    print("linked kind against mpmath: max |d| = %.2e at |value| = %.0f" % (d.max(), abs(want[d.argmax()])))
    assert np.all(d <= 1e-11)
    # outside the bounds, at them, and a NaN on either side
    one = rec[:1]
    edge = _lnpdf(lib, one, [lo, hi_, np.nextafter(lo, -9.0), np.nextafter(hi_, 9.0), 0.0, np.nan], [9.0, 9.0, 9.0, 9.0, np.nan, 9.0])[0]
    assert np.isfinite(edge[:2]).all() and np.isneginf(edge[2:5]).all() and np.isnan(edge[5])


SHAPES = rt.SHAPES


@pytest.mark.parametrize("S, W, T, Q, H, layout, links", SHAPES)
def test_lnlike_host_matches_the_twin(lib, S, W, T, Q, H, layout, links):
    case = rt.linked_case(S, W, T, Q, H, seed=7 * Q + H + W, links=links, layout=layout)
    assert len({w[1] for w in case["where"]}) == 2                  # columns from two storages with different C
    assert all(case["where"][c][0] != case["where"][p][0] for c, p in links.items() if (c - p) % 2)
    rc, got = rt.call(lib, case)
    assert rc == 0, lib.iso_relation_last_error()
    want = rt.want(case)
    assert np.isfinite(want["ell"]).all()
    rt.assert_matches(got, want, (S, W, T, Q, H, layout))


@pytest.mark.parametrize("name", ["parent_nan", "child_out", "mean_60_sigma", "bad_parent", "masked", "span_700"])
def test_special_cases(lib, name):
    case = rt.special_cases()[name]
    rc, got = rt.call(lib, case)
    assert rc == 0, lib.iso_relation_last_error()
    rt.assert_matches(got, rt.want(case), name)
    rt.check_special(name, case, got)


def test_slope_zero_is_the_truncated_gaussian(lib):
    build_hier.build()
    linked, plain = rt.slope_zero_pair()
    rc, got = rt.call(lib, linked)
    rc2, ref = tw.call(hc.lib(), plain)
    assert rc == 0 and rc2 == 0
    lim = 2e-11 * np.maximum(1.0, tw.want(plain)["rmax"] / 100.0)   # each side is within the twin's limit
    assert np.all(np.abs(got["ell"] - ref["ell"]) <= lim) and np.array_equal(got["n_bad"], ref["n_bad"])


def test_unlinked_records_give_the_hier_entry_exactly(lib):
    build_hier.build()
    case = tw.random_case(3, 5, 7, 4, TILE + 1, seed=6)
    rc, got = rt.call(lib, case)
    rc2, ref = tw.call(hc.lib(), case)
    assert rc == 0 and rc2 == 0
    for k in ("ell", "ess", "n_bad", "L", "min_ess"):
        assert got[k].tobytes() == ref[k].tobytes(), k


def test_closed_form(lib):
    case, exact, slopes, _, _ = rt.closed_form_case()
    rc, got = rt.call(lib, case)
    assert rc == 0, lib.iso_relation_last_error()
    assert (got["n_bad"] == 0).all()
    rt.check_closed_form(got, exact, slopes, case["W"] * case["T"])


def test_refused_arguments(lib):
    case = rt.linked_case(3, 5, 7, 2, 3, seed=3, links={1: 0})
    S, W, T = 3, 5, 7
    st = case["storages"]
    rows, interim = np.ascontiguousarray(case["rows"]), np.ascontiguousarray(case["interim"])
    out = [np.zeros((3, S)), np.zeros((3, S)), np.zeros(S, np.int32), np.zeros(3), np.zeros(3)]
    p = lambda a: C.c_void_p(a.ctypes.data)
    good_cols = [hc.IsoHierColumn(st[k].ctypes.data, n, c, S, 0) for k, n, c in case["where"]]

    def run(cols=None, Q=2, layout=PM, nsteps=T, n_ens=S, b=0, n=S, H=3, L=True, interim_=interim, fn=lib.iso_relation_lnlike_host):
        arr = (hc.IsoHierColumn * 4)(*(cols or good_cols))
        rc = fn(arr, Q, layout, nsteps, n_ens, W, b, n, None if interim_ is None else p(interim_), p(rows), H, None, p(out[0]),
                p(out[1]), p(out[2]), p(out[3]) if L else None, p(out[4]), None)
        return rc, (lib.iso_relation_last_error() or b"").decode()

    assert run()[0] == 0
    linked_interim = interim.copy()
    linked_interim[1] = rows[0, 1]
    for kw, text in ((dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(layout=7), "layout"),
                     (dict(nsteps=0), "at least 1"), (dict(H=0), "H must be"), (dict(b=2, n=2), "ensemble range"),
                     (dict(L=False), "both or neither"), (dict(interim_=None), "null pointer"),
                     (dict(interim_=linked_interim), "an interim record is linked"),
                     (dict(cols=[hc.IsoHierColumn(st[0].ctypes.data, 4, 4, S, 0)] * 2), "column index"),
                     (dict(cols=[hc.IsoHierColumn(0, 4, 1, S, 0)] * 2), "null column"),
                     (dict(cols=[hc.IsoHierColumn(st[0].ctypes.data, 4, 1, 2, 0)] * 2), "does not hold")):
        rc, msg = run(**kw)
        assert rc == rl.ERR_INVALID and text in msg and msg.startswith("iso_relation_lnlike_host: "), (kw, msg)
    # the device entry refuses the same before it touches a device
    rc, msg = run(Q=5, fn=lib.iso_relation_lnlike)
    assert rc == rl.ERR_INVALID and msg.startswith("iso_relation_lnlike: ")
    assert lib.iso_relation_lnpdf_host(None, 1, None, None, 1, None) == rl.ERR_INVALID
    x = np.zeros(1)
    assert lib.iso_relation_lnpdf_host(p(rows[0, 1:2].copy()), 1, p(x), None, 1, p(out[3])) == rl.ERR_INVALID
    assert b"xp" in lib.iso_relation_last_error()
