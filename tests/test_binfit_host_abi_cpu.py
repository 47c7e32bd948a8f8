"""libiso_binfit.so's host entry through ctypes, no GPU needed: iso_binfit_moments_host against the long-double twin of
tests/_binfit_twin.py within 1e-11 relative to max(1, n_live), both identities, the star-sum of iso_shrink_cells_host's cell
probabilities, the edge cases of the stars, the cells and the rows, every refusal with its message, and the twin's own
gradient against central differences of its long-double likelihood."""
import numpy as np
import pytest

from isochrones_amd import _binfit_cabi as fc, _binned_cabi as bc, _shrink_cabi as sc
from isochrones_amd.csrc.libraries import BINFIT, BINNED, HIER, SHRINK
from tests import _binfit_twin as ft, _binned_twin as bt, _shrink_twin as st

LD = ft.LD


@pytest.fixture(scope="module")
def lib():
    for spec in (HIER, BINNED, SHRINK, BINFIT):
        spec.build()
    return fc.lib()


def _err(lib):
    return lib.iso_binfit_last_error().decode()


@pytest.mark.parametrize("S, B, H", [(1, 1, 1), (7, 1, 3), (5, 2, 1), (300, 12, 4), (257, 63, 2), (64, 64, 9), (130, 15, 8)])
def test_host_entry_matches_the_twin(lib, S, B, H):
    A = ft.random_table(S, B, seed=S + B, dead=(S // 2,) if S > 2 else ())
    lnh = ft.random_lnh(H, B, seed=H + B) if B > 1 else np.random.default_rng(H).normal(size=(H, 1))
    mask = None
    if S > 4:
        mask = np.ones(S, np.int32)
        mask[[1, S - 1]] = 0                                           # masked stars
    rc, out = ft.call(lib, A, lnh, mask)
    assert rc == 0, _err(lib)
    worst = ft.assert_matches(out, A, lnh, mask)
    print("against the twin: worst error / limit = %.2e, n_live = %s" % (worst, out["n_live"]))
    if S > 4:
        # the dead star and the two masked ones are counted out wherever every other star has weight
        assert out["n_live"].max() <= S - 3 and (out["n_live"] >= 0).all()
    # without C the same N and n_live, bit for bit, and C is not touched
    rc, again = ft.call(lib, A, lnh, mask, pairs=False)
    assert rc == 0 and again["N"].tobytes() == out["N"].tobytes() and np.array_equal(again["n_live"], out["n_live"])
    assert (again["C"] == -7.0).all()
    # a sub-range of the rows is the same bits
    if H >= 3:
        rc, part = ft.call(lib, A, lnh, mask, rows=(1, 2))
        assert rc == 0 and part["N"].tobytes() == out["N"][1:3].tobytes() and part["C"].tobytes() == out["C"][1:3].tobytes()
        assert np.array_equal(part["n_live"], out["n_live"][1:3])


def test_dead_stars_zero_heights_and_nan(lib):
    S, B = 40, 6
    A = ft.random_table(S, B, seed=1, dead=(0, 17), sparse=0.0)
    A[1:, 5] = 0.0                                                     # star 5 has weight in cell 0 only
    lnh = np.zeros((4, B))
    lnh[1, 0] = -np.inf                                                # star 5 is not live under row 1
    lnh[2, 0] = np.nan                                                 # nor under row 2: a NaN counts as height 0
    lnh[3, 1:] = -np.inf                                               # one cell left: every live star is in it
    rc, out = ft.call(lib, A, lnh)
    assert rc == 0, _err(lib)
    ft.assert_matches(out, A, lnh)
    assert list(out["n_live"]) == [S - 2, S - 3, S - 3, S - 2]
    assert out["N"][1, 0] == 0.0 and out["N"][2, 0] == 0.0 and out["N"][1].tobytes() == out["N"][2].tobytes()
    assert (out["C"][1, 0] == 0.0).all() and (out["C"][1, :, 0] == 0.0).all()
    assert out["N"][3, 0] == S - 2 and (out["N"][3, 1:] == 0.0).all() and out["C"][3, 0, 0] == S - 2
    # a row without any height: nobody is live
    rc, none = ft.call(lib, A, np.full((1, B), -np.inf))
    assert rc == 0 and none["n_live"][0] == 0 and (none["N"] == 0.0).all() and (none["C"] == 0.0).all()
    # everybody masked
    rc, none = ft.call(lib, A, lnh, np.zeros(S, np.int32))
    assert rc == 0 and (none["n_live"] == 0).all() and (none["N"] == 0.0).all() and (none["C"] == 0.0).all()


@pytest.mark.parametrize("n_bins, n_frozen", [((5,), 1), ((3, 4), 1), ((64,), 0)])
def test_counts_are_the_star_sum_of_the_cell_probabilities(lib, n_bins, n_frozen):
    """H = 1: N is the sum over the stars of iso_shrink_cells_host's cellp under the row's own ell."""
    blib, slib = bc.lib(), sc.lib()
    case = bt.make_case(11, 6, 9, n_bins, 1, seed=5 + len(n_bins), n_frozen=n_frozen)
    tab, out = bt.run(blib, case)
    rc, cel = st.call_cells(slib, tab, case["lnh"], out["ell"])
    assert rc == 0
    rc, got = ft.call(lib, tab["A"], case["lnh"])
    assert rc == 0, _err(lib)
    live = np.isfinite(cel["cellp"]).all(axis=0)
    assert got["n_live"][0] == live.sum() > 0
    want = cel["cellp"][:, live].sum(axis=1)
    assert np.all(np.abs(got["N"][0] - want) <= 1e-11 * max(1, live.sum()))
    ft.assert_matches(got, tab["A"], case["lnh"])


def test_refusals(lib):
    A, lnh = ft.random_table(5, 3, seed=0), np.zeros((2, 3))
    bad = lnh.copy()
    bad[1, 2] = np.inf
    rc, _ = ft.call(lib, A, bad)
    assert rc == fc.ERR_INVALID and "+inf" in _err(lib) and "iso_binfit_moments_host" in _err(lib)
    N, live = np.zeros((2, 3)), np.zeros(2, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    fn = lib.iso_binfit_moments_host
    for args, word in (((p(A), 0, 5, p(lnh), 2, None, p(N), None, p(live), None, None), "B must be"),
                       ((p(A), 65, 5, p(lnh), 2, None, p(N), None, p(live), None, None), "B must be"),
                       ((p(A), 3, 0, p(lnh), 2, None, p(N), None, p(live), None, None), "n_ens"),
                       ((p(A), 3, 5, p(lnh), 0, None, p(N), None, p(live), None, None), "H must be"),
                       ((None, 3, 5, p(lnh), 2, None, p(N), None, p(live), None, None), "null"),
                       ((p(A), 3, 5, p(lnh), 2, None, None, None, p(live), None, None), "null"),
                       ((p(A), 3, 5, p(lnh), 2, None, p(N), None, None, None, None), "null")):
        assert fn(*args) == fc.ERR_INVALID and word in _err(lib), (args, _err(lib))
    # the device entry needs its workspace, and says so without touching a device
    assert lib.iso_binfit_moments(p(A), 3, 5, p(lnh), 2, None, p(N), None, p(live), None, None) == fc.ERR_INVALID
    assert "null" in _err(lib)
    assert fn(p(A), 3, 5, p(lnh), 2, None, p(N), None, p(live), None, None) == 0 and _err(lib) == ""


@pytest.mark.parametrize("shape, sel", [(("one", 12), True), (("one", 5), False), (("given", 3, 4), True), (("indep", 3, 4), False)])
def test_the_twin_gradient_against_central_differences(shape, sel):
    """The twin's analytic gradient against central differences of its own long-double L: step 1e-5, tolerance 1e-6 max(1,
    max |g|).  The truncation error h^2 f''' / 6 ~ 1e-10 |f'''| and the round-off 1e-19 |L| / h ~ 1e-11 at |L| ~ 10^3 are
    both orders of magnitude below it.  The Hessian against central differences of the analytic gradient likewise."""
    P, B, _ = ft.blocks(shape)
    rng = np.random.default_rng(P)
    S = 300
    A = ft.random_table(S, B, seed=B, dead=(3,))
    mask = np.ones(S, np.int32)
    mask[7] = 0
    lnvol = rng.normal(0.0, 0.3, B)
    a_sel = np.exp(rng.normal(0.0, 1.0, B)) if sel else None
    theta = rng.normal(0.0, 0.7, P)
    f = lambda th: ft.objective(shape, th, lnvol, A, mask, a_sel)
    g, hess = ft.derivatives(shape, theta, lnvol, A, mask, a_sel)
    num = ft.central_gradient(f, theta)
    err = float(np.max(np.abs(num - g)))
    print("twin gradient: |L| = %.3g, max |g| = %.3g, worst difference %.2e" % (abs(f(theta)), np.max(np.abs(g)), err))
    assert err <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    numh = np.stack([ft.central_gradient(lambda th, i=i: ft.derivatives(shape, th, lnvol, A, mask, a_sel)[0][i], theta)
                     for i in range(P)])
    errh = float(np.max(np.abs(numh - hess)))
    assert errh <= 1e-6 * max(1.0, float(np.max(np.abs(hess)))), errh
    assert np.max(np.abs(hess - hess.T)) <= 1e-12 * max(1.0, float(np.max(np.abs(hess))))
