"""The long-double reference of iso_cluster_lnlike (tests/_cluster_hp.py) against the reference's own numbers in
tests/golden/cluster/ and against the float64 restatement (tests/_cluster_ref.py), and every argument refusal of the C ABI
(all of them return before any HIP call, so no device is needed)."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd.csrc.libraries import CLUSTER as B

from . import _cluster_hp as H
from . import _cluster_ref as R

TINY = np.finfo(np.float64).tiny


def test_long_double_has_a_64_bit_significand():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("case", R.CASES)
def test_long_double_reference_matches_the_fixtures(case):
    fx = R.load(case)
    a = H.fixture_inputs(fx)
    checked = tight = 0
    for i in np.flatnonzero(~fx["undefined"]):
        tot, ln = H.lnlike(a["cols"][i:i + 1], a["n_valid"][i:i + 1], a["rowpar"][i:i + 1], a["star_val"], a["star_w"],
                           a["minq"][i], a["n_bands"], a["n_props"])
        like = np.exp(ln[0])
        want = fx["like_tot"][i]
        assert np.array_equal(np.isnan(like), np.isnan(want)), (case, i)
        assert np.array_equal(like == 0, want == 0), (case, i)
        ok = np.isfinite(want) & (want != 0)
        normal = ok & (want >= TINY)
        with np.errstate(divide="ignore"):
            lw = np.log(want[normal])
        assert np.all(np.abs(ln[0][normal].astype(float) - lw) <= 1e-12 * (1 + np.abs(lw))), (case, i)
        # a subnormal like_s keeps few bits in the fixture's float64 trapezoids: compared with an absolute floor
        assert np.all(np.abs(like[ok & ~normal] - want[ok & ~normal]) <= 1e-300), (case, i)
        ref, got = fx["lnlike"][i], float(tot[0])
        if not np.isfinite(ref):
            assert (np.isnan(got) and np.isnan(ref)) or got == ref, (case, i, got, ref)
        elif np.all(normal == ok):
            assert abs(got - ref) <= 1e-12 * (1 + abs(ref)), (case, i, got, ref)
            tight += 1
        checked += 1
    assert checked >= 15 and tight >= 8


def _random_row(rng, n, ns, nb, npr, minq):
    eep = np.cumsum(rng.uniform(0.3, 3.0, n)) + 200.0
    mass = np.sort(rng.uniform(0.3, 1.5, n))
    lndm = np.log(rng.uniform(1e-3, 2e-2, n))
    mags = rng.uniform(4.0, 9.0, nb)[None, :] - 3.0 * (mass[:, None] - 0.3)
    props = rng.uniform(-1.0, 1.0, (n, npr))
    pick = rng.integers(0, n, ns)
    star_mag = mags[pick] + rng.normal(0.0, 0.05, (ns, nb))
    star_unc = rng.uniform(0.02, 0.2, (ns, nb))
    star_prop = props[pick] + rng.normal(0.0, 0.1, (ns, npr))
    star_unc_p = rng.uniform(0.1, 0.3, (ns, npr))
    return eep, mass, lndm, mags, props, star_mag, star_unc, star_prop, star_unc_p


@pytest.mark.parametrize("seed", range(6))
def test_long_double_reference_matches_the_float64_restatement(seed):
    rng = np.random.default_rng(700 + seed)
    n, ns, nb, npr = int(rng.integers(2, 40)), int(rng.integers(1, 20)), int(rng.integers(1, 5)), int(rng.integers(0, 3))
    minq = float(rng.choice([0.1, 0.3, 0.6]))
    alpha, gamma, fB = rng.uniform(-3.5, -1.5), rng.uniform(0.1, 0.6), rng.uniform(0.05, 0.6)
    eep, mass, lndm, mags, props, sm, su, sp, spu = _random_row(rng, n, ns, nb, npr, minq)
    want = R.like_per_star(eep, mass, lndm, mags, props, sm, su, sp, spu, alpha, gamma, fB, 0.1, 300.0, minq)
    ld = n + int(rng.integers(0, 5))
    c, rp = H.row_columns(eep, mass, lndm, mags, props, alpha, gamma, fB, minq, 0.1, 300.0, ld)
    val = np.concatenate([sm.T, sp.T])
    w = 1.0 / np.concatenate([su.T, spu.T]) ** 2
    tot, ln = H.lnlike(c[None], [n], rp[None], val, w, minq, nb, npr)
    like = np.exp(ln[0]).astype(float)
    assert np.all(want > 1e-200), want
    np.testing.assert_allclose(like, want, rtol=1e-12, atol=0)
    assert abs(float(tot[0]) - R.lnlike_from_likes(want)) <= 1e-12 * (1 + abs(float(tot[0])))


def test_n_valid_is_clamped_to_the_leading_dimension():
    rng = np.random.default_rng(3)
    eep, mass, lndm, mags, props, sm, su, sp, spu = _random_row(rng, 12, 4, 2, 0, 0.1)
    c, rp = H.row_columns(eep, mass, lndm, mags, props, -2.5, 0.3, 0.3, 0.1, 0.1, 300.0)
    args = (np.repeat(c[None], 4, axis=0), np.array([12, 40, -5, 0]), np.repeat(rp[None], 4, axis=0), sm.T, 1 / su.T ** 2,
            0.1)
    tot, ln = H.lnlike(*args)
    assert np.isfinite(tot[0]) and tot[1] == tot[0] and np.array_equal(ln[1], ln[0])
    assert tot[2] == tot[3] == -np.inf and np.all(ln[2:] == -np.inf)


# -- argument refusals of iso_cluster_lnlike -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    from isochrones_amd import _cluster_cabi
    return _cluster_cabi.lib()


_BUF = (C.c_double * 16)()                 # a host address: none of the refusals below may dereference or launch


def _good(**kw):
    p = C.cast(_BUF, C.c_void_p)
    a = dict(cols=p, ld=10, n_rows=1, n_valid=p, rowpar=p, star_val=p, star_w=p, n_stars=5, n_bands=3, n_props=1,
             minq=0.1, work=p, lnlike=p, lnlike_star=None, stream=None)
    a.update(kw)
    return a


def _call(lib, a):
    return lib.iso_cluster_lnlike(a["cols"], a["ld"], a["n_rows"], a["n_valid"], a["rowpar"], a["star_val"], a["star_w"],
                                  a["n_stars"], a["n_bands"], a["n_props"], a["minq"], a["work"], a["lnlike"],
                                  a["lnlike_star"], a["stream"])


BAD = [dict(ld=0), dict(ld=-3), dict(n_stars=0), dict(n_stars=-1), dict(n_bands=0), dict(n_bands=33), dict(n_props=-1),
       dict(n_props=9), dict(n_rows=-1)]
BAD += [{name: None} for name in ("cols", "n_valid", "rowpar", "star_val", "star_w", "work", "lnlike")]
BAD += [dict(n_rows=2, ld=1 << 30, n_stars=64),                   # 2 x 1 x 2^30 = 2^31 workgroups
        dict(n_rows=1, ld=1 << 24, n_stars=64 * 128 + 1)]          # 129 tiles x 2^24 > INT32_MAX


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_bad_arguments_are_refused(lib, bad):
    assert _call(lib, _good(**bad)) == -1           # ISO_CLUSTER_ERR_INVALID
    assert lib.iso_cluster_last_error()
    assert _call(lib, _good(n_rows=0)) == 0         # ... and the next good call clears the message
    assert lib.iso_cluster_last_error() == b""


def test_limits_themselves_are_accepted_with_no_rows(lib):
    for kw in (dict(n_bands=1), dict(n_bands=32), dict(n_props=0), dict(n_props=8), dict(ld=1, n_stars=1)):
        assert _call(lib, _good(n_rows=0, **kw)) == 0, kw
