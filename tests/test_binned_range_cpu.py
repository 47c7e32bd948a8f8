"""The host entries of the binned-population family where a row's log cell heights, or a fit's start masses, span hundreds
of nats (tests/_range_cases.py), no GPU needed: iso_binned_lnlike_host, iso_binfit_moments_host, iso_shrink_cells_host and
iso_emfit_run_host against their long-double twins with that module's limits, and what has to hold between the outputs: ess
is never NaN for an unmasked star, min_ess is the minimum of ess, L the sum of ell, a star is live in the moments and in a
fit exactly where its ell is finite, a fit returns no NaN mass and is never EMPTY while the twin has live stars."""
import numpy as np
import pytest

from isochrones_amd import _binfit_cabi as fc, _binned_cabi as bc, _emfit_cabi as ec, _shrink_cabi as sc
from isochrones_amd.csrc.libraries import BINFIT, BINNED, EMFIT, SHRINK
from tests import _binfit_twin as ft, _binned_twin as bt, _emfit_twin as et, _range_cases as rg, _shrink_twin as st

SHAPES = [(6, 4), (6, 9), (257, 4), (257, 64)]
NINF = -np.inf


@pytest.fixture(scope="module")
def libs():
    for spec in (BINNED, SHRINK, BINFIT, EMFIT):
        spec.build()
    return dict(binned=bc.lib(), shrink=sc.lib(), binfit=fc.lib(), emfit=ec.lib())


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "S%d-B%d" % p)
def case(request):
    return rg.case(*request.param)


def test_the_cases_are_what_they_say():
    for S, B in SHAPES:
        tab, lnh, names = rg.case(S, B)
        pos = tab["A"] > 0
        assert np.array_equal(pos, tab["A2"] > 0) and tab["A"][pos].min() >= 1e-3 and tab["A2"][pos].min() >= 1e-3
        assert np.all(tab["A"] ** 2 <= tab["A2"] * tab["M"] * (1 + 1e-12))            # Cauchy-Schwarz: A2 is consistent with A
        for kind in (rg.EVERY, rg.ONE, rg.TWO, rg.DEAD, rg.MASKED):
            assert kind in tab["kinds"]
        one, two = tab["kinds"].index(rg.ONE), tab["kinds"].index(rg.TWO)
        assert np.flatnonzero(pos[:, one]).tolist() == [rg.LOW] and np.flatnonzero(pos[:, two]).tolist() == [rg.LOW, rg.MID]
        assert pos[:, tab["kinds"].index(rg.EVERY)].all() and sorted(tab["mx"][np.isfinite(tab["mx"]) & (np.abs(tab["mx"]) > 100)]) == [-1e4, 1e4]
        assert rg.straddles(tab, lnh) and len(names) == lnh.shape[0] == len(rg.GAPS) + 2 + 3
        if S > 256:
            assert tab["kinds"][256] == rg.TWO and rg.ONE in tab["kinds"][250:256]
    g0 = rg.em_starts(4)
    assert g0[:, rg.LOW].tolist() == list(rg.TINY) and 0 < g0[2, rg.LOW] < 2.2250738585072014e-308


def test_binned_lnlike_host(libs, case):
    tab, lnh, names = case
    rc, out = bt.call_lnlike(libs["binned"], tab, lnh, tab["M"], tab["mask"])
    assert rc == 0, libs["binned"].iso_binned_last_error()
    worst = rg.assert_binned(out, tab, lnh, "host")
    print("S = %d, B = %d: worst |d ell| / limit %.2e, |d ess| / limit %.2e" % (tab["A"].shape[1], lnh.shape[1], *worst))
    # the rows of height 0 and of NaN are one row; a star with weight only under such cells has no support there
    assert np.array_equal(out["ell"][-1], out["ell"][-2], equal_nan=True) and np.array_equal(out["ess"][-1], out["ess"][-2], equal_nan=True)
    one = tab["kinds"].index(rg.ONE)
    assert out["ell"][-1, one] == NINF and out["ess"][-1, one] == 0.0 and out["L"][-1] == NINF and out["min_ess"][-1] == 0.0
    # the shift by +700 moves ell by 700 and nothing else
    h, k = names.index("G=500"), names.index("G=500+700")
    on = (tab["mask"] != 0) & np.isfinite(out["ell"][h])
    assert np.all(np.abs((out["ell"][k, on] - 700.0) - out["ell"][h, on]) <= 2e-11)
    np.testing.assert_allclose(out["ess"][k, on], out["ess"][h, on], rtol=1e-10, atol=0)
    # every row alone gives the bits it has among the others
    for h in (0, names.index("G=746"), len(names) - 1):
        rc, single = bt.call_lnlike(libs["binned"], tab, lnh[h:h + 1], tab["M"], tab["mask"])
        assert rc == 0 and all(np.array_equal(single[key][0], out[key][h], equal_nan=True) for key in ("ell", "ess", "L", "min_ess"))


@pytest.mark.parametrize("pairs", [True, False])
def test_binfit_moments_host(libs, case, pairs):
    tab, lnh, names = case
    rc, out = ft.call(libs["binfit"], tab["A"], lnh, tab["mask"], pairs=pairs)
    assert rc == 0, libs["binfit"].iso_binfit_last_error()
    rc, like = bt.call_lnlike(libs["binned"], tab, lnh, tab["M"], tab["mask"])
    assert rc == 0
    worst = rg.assert_binfit(out, like["ell"], tab, lnh, pairs=pairs, what="host")
    print("S = %d, B = %d, pairs %s: worst error / limit %.2e" % (tab["A"].shape[1], lnh.shape[1], pairs, worst))
    if not pairs:
        assert (out["C"] == -7.0).all()


def test_shrink_cells_host(libs, case):
    tab, lnh, names = case
    ell = bt.lnlike(tab, lnh, tab["M"], tab["mask"])["ell"]
    rc, out = st.call_cells(libs["shrink"], tab, lnh, ell, tab["mask"])
    assert rc == 0, libs["shrink"].iso_shrink_last_error()
    lnG, cellp = st.cells(tab["A"], tab["mx"], lnh, ell, tab["mask"])
    worst = st.close(out["lnG"], lnG, log=True), st.close(out["cellp"], cellp)
    print("S = %d, B = %d: lnG %.2e, cellp %.2e of the limit" % (tab["A"].shape[1], lnh.shape[1], *worst))


@pytest.mark.parametrize("steps", [0, 1, 2, 7])
@pytest.mark.parametrize("S, B", SHAPES)
def test_emfit_run_host(libs, S, B, steps):
    c = rg.em_case(S, B)
    rc, out = et.call(libs["emfit"], max_iter=steps, tol=NINF, **c)
    assert rc == 0, libs["emfit"].iso_emfit_last_error()
    ref = et.run(max_iter=steps, tol=NINF, **c)
    worst = rg.assert_emfit(out, ref, c, "host")
    print("S = %d, B = %d, %d steps: worst error / limit %.2e" % (S, B, steps, worst))
    assert (ref["n_live"] > 0).all() and (out["status"] == ec.MAX_ITER).all()
    # a star is live in a fit exactly where its ell under the start's heights is finite
    tab = rg.wide_tables(S, B)
    with np.errstate(divide="ignore"):
        lnv = np.asarray(np.log(c["g0"].astype(rg.LD)) + np.log(c["scale"].astype(rg.LD)), np.float64)
    if steps == 0:
        rc, like = bt.call_lnlike(libs["binned"], tab, lnv, tab["M"], tab["mask"])
        assert rc == 0 and np.array_equal(out["n_live"], np.isfinite(like["ell"]).sum(axis=1))
    # a start of 0 stays 0, every other mass of LOW is carried by the stars that have nothing else
    zero = c["g0"][:, rg.LOW] == 0
    assert (out["g"][zero, rg.LOW] == 0).all() and (steps == 0 or (out["g"][~zero, rg.LOW] > 1e-3).all())


def test_emfit_one_replicate_is_its_bits_in_the_batch(libs):
    c = rg.em_case(257, 9)
    rc, out = et.call(libs["emfit"], max_iter=3, tol=NINF, **c)
    assert rc == 0
    for r in (2, 7, 9, 13):
        rc, single = et.call(libs["emfit"], c["A"], c["scale"], c["w"][r:r + 1], c["mask"], c["g0"][r:r + 1], max_iter=3, tol=NINF)
        assert rc == 0 and et.same_bits(single, {k: v[r:r + 1] for k, v in out.items()})
