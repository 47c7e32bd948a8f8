"""The kernels of the binned-population family where a row's log cell heights, or a fit's start masses, span hundreds of
nats (tests/_range_cases.py): iso_binned_lnlike, iso_binfit_moments (with and without C), iso_shrink_cells and iso_emfit_run
(one launch, and launches of one step) against the host entries on the same inputs and against the long-double twins, with
that module's limits; the bit identities of the family on these inputs (a (row, star) alone, in a batch and in a range of
stars that starts at 250; a row alone and in any tiling of the rows; a repeated call; a replicate alone and in a batch); and
the fill value -7 beyond what a call writes.  Every input is a call the host entries accept; no table is larger than
257 x 64 doubles."""
import numpy as np
import pytest

from isochrones_amd import _binfit_cabi as fc, _binned_cabi as bc, _emfit_cabi as ec, _shrink_cabi as sc
from tests import _binfit_twin as ft, _binned_twin as bt, _emfit_twin as et, _range_cases as rg, _shrink_twin as st

pytestmark = pytest.mark.gpu
SHAPES = [(6, 4), (6, 9), (257, 4), (257, 64)]
NINF = -np.inf
OUT = ("ell", "ess", "L", "min_ess")


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def libs():
    return dict(binned=bc.lib(), shrink=sc.lib(), binfit=fc.lib(), emfit=ec.lib())


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "S%d-B%d" % p)
def case(request):
    return rg.case(*request.param)


def _lnlike(libs, tab, lnh, device=None, **kw):
    rc, out = bt.call_lnlike(libs["binned"], tab, lnh, tab["M"], tab["mask"], device=device, **kw)
    assert rc == 0, libs["binned"].iso_binned_last_error()
    return out


def _same(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a)


def _special_equal(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN")
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(got)], ref[np.isinf(ref)]), (what, "inf")
    fin = np.isfinite(ref)
    assert np.array_equal(got[fin] == 0, ref[fin] == 0), (what, "zeros")
    return fin


def test_binned_lnlike(libs, device, case):
    tab, lnh, names = case
    got, ref = _lnlike(libs, tab, lnh, device), _lnlike(libs, tab, lnh)
    f = rg.factor(tab["A"], lnh)
    worst = {}
    for k, lim in (("ell", 1e-11 * f), ("ess", 1e-11 * f * np.abs(ref["ess"]))):
        fin = _special_equal(got[k], ref[k], k)
        worst[k] = float(np.max(np.abs(got[k][fin] - ref[k][fin]) / np.where(lim[fin] > 0, lim[fin], 1.0)))
    twin = rg.assert_binned(got, tab, lnh, "device")
    print("S = %d, B = %d: device against host, |d ell| %.2e and |d ess| %.2e of the limit; against the twin %.2e and %.2e"
          % (tab["A"].shape[1], lnh.shape[1], worst["ell"], worst["ess"], *twin))
    assert worst["ell"] <= 1.0 and worst["ess"] <= 1.0
    _special_equal(got["L"], ref["L"], "L")
    _special_equal(got["min_ess"], ref["min_ess"], "min_ess")
    assert _same(got, _lnlike(libs, tab, lnh, device))                  # a repeated call


def test_binned_rows_and_stars_are_bit_identical(libs, device):
    tab, lnh, names = rg.case(257, 9)
    H, S = lnh.shape[0], 257
    full = _lnlike(libs, tab, lnh, device)
    # a row alone, and the rows in tiles of 1, 3, 8 and 9 rows from 0 and of 8 from row 5
    for step, first in ((1, 0), (3, 0), (8, 0), (9, 0), (8, 5)):
        for a in range(first, H, step):
            part = _lnlike(libs, tab, lnh[a:a + step], device)
            assert all(part[k].tobytes() == full[k][a:a + step].tobytes() for k in OUT), (step, a)
    # a range of stars that starts at 250 and reaches into the second block, and single stars of every type
    ranges = [(250, 7), (256, 1)] + [(tab["kinds"].index(k), 1) for k in (rg.EVERY, rg.ONE, rg.TWO, rg.DEAD, rg.MASKED)]
    for s0, n in ranges:
        part = _lnlike(libs, tab, lnh, device, ens_begin=s0, n_ens_out=n, total=False)
        inside = np.zeros(S, bool)
        inside[s0:s0 + n] = True
        for k in ("ell", "ess"):
            assert part[k][:, inside].tobytes() == full[k][:, inside].tobytes(), (s0, n, k)
            assert (part[k][:, ~inside] == -7.0).all(), (s0, n, k)
        assert (part["L"] == -7.0).all() and (part["min_ess"] == -7.0).all()
    # one (row, star) alone
    one, h = tab["kinds"].index(rg.ONE), names.index("G=746")
    part = _lnlike(libs, tab, lnh[h:h + 1], device, ens_begin=one, n_ens_out=1, total=False)
    assert part["ell"][0, one] == full["ell"][h, one] and part["ess"][0, one] == full["ess"][h, one]
    assert (np.delete(part["ell"][0], one) == -7.0).all()


@pytest.mark.parametrize("pairs", [True, False])
def test_binfit_moments(libs, device, case, pairs):
    tab, lnh, names = case
    lib = libs["binfit"]
    rc, got = ft.call(lib, tab["A"], lnh, tab["mask"], device=device, pairs=pairs, guard=True)
    assert rc == 0, lib.iso_binfit_last_error()
    rc, ref = ft.call(lib, tab["A"], lnh, tab["mask"], pairs=pairs)
    assert rc == 0
    ell = _lnlike(libs, tab, lnh, device)["ell"]
    f = rg.factor(tab["A"], lnh)[:, tab["mask"] != 0].max(axis=1)
    lim = ft.LIMIT * f * np.maximum(1, ref["n_live"])
    assert np.array_equal(got["n_live"], ref["n_live"])
    dN = float(np.max(np.abs(got["N"] - ref["N"]) / lim[:, None]))
    dC = float(np.max(np.abs(got["C"] - ref["C"]) / lim[:, None, None])) if pairs else 0.0
    twin = rg.assert_binfit(got, ell, tab, lnh, pairs=pairs, what="device")
    print("S = %d, B = %d, pairs %s: device against host, N %.2e and C %.2e of the limit; against the twin %.2e"
          % (tab["A"].shape[1], lnh.shape[1], pairs, dN, dC, twin))
    assert dN <= 1.0 and dC <= 1.0 and np.array_equal(got["N"] == 0, ref["N"] == 0)
    if not pairs:
        assert (got["C"] == -7.0).all()
    # a repeated call, a row alone and the rows from 5 on
    rc, again = ft.call(lib, tab["A"], lnh, tab["mask"], device=device, pairs=pairs)
    assert rc == 0 and _same(got, again)
    for first, count in ((names.index("G=746"), 1), (5, lnh.shape[0] - 5)):
        rc, part = ft.call(lib, tab["A"], lnh, tab["mask"], device=device, pairs=pairs, rows=(first, count))
        assert rc == 0 and all(part[k].tobytes() == got[k][first:first + count].tobytes() for k in ("N", "C", "n_live"))


def test_shrink_cells(libs, device, case):
    tab, lnh, names = case
    lib = libs["shrink"]
    ell = bt.lnlike(tab, lnh, tab["M"], tab["mask"])["ell"]
    rc, got = st.call_cells(lib, tab, lnh, ell, tab["mask"], device=device)
    assert rc == 0, lib.iso_shrink_last_error()
    rc, ref = st.call_cells(lib, tab, lnh, ell, tab["mask"])
    assert rc == 0
    host = st.close(got["lnG"], ref["lnG"], log=True), st.close(got["cellp"], ref["cellp"])
    lnG, cellp = st.cells(tab["A"], tab["mx"], lnh, ell, tab["mask"])
    twin = st.close(got["lnG"], lnG, log=True), st.close(got["cellp"], cellp)
    print("S = %d, B = %d: device against host, lnG %.2e and cellp %.2e of the limit; against the twin %.2e and %.2e"
          % (tab["A"].shape[1], lnh.shape[1], *host, *twin))
    rc, again = st.call_cells(lib, tab, lnh, ell, tab["mask"], device=device)
    assert rc == 0 and _same(got, again)
    S = tab["A"].shape[1]
    if S > 256:
        rc, part = st.call_cells(lib, tab, lnh, ell, tab["mask"], device=device, ens_begin=250, n_ens_out=7)
        assert rc == 0
        for k in ("lnG", "cellp"):
            assert part[k][:, 250:].tobytes() == got[k][:, 250:].tobytes() and (part[k][:, :250] == -7.0).all()


@pytest.mark.parametrize("steps", [0, 1, 7])
@pytest.mark.parametrize("S, B", SHAPES)
def test_emfit_run(libs, device, S, B, steps):
    c = rg.em_case(S, B)
    lib = libs["emfit"]
    rc, got = et.call(lib, max_iter=steps, tol=NINF, device=device, guard=True, **c)
    assert rc == 0, lib.iso_emfit_last_error()
    rc, ref = et.call(lib, max_iter=steps, tol=NINF, **c)
    assert rc == 0
    twin = et.run(max_iter=steps, tol=NINF, **c)
    for k in ("n_iter", "status", "n_live"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    lim = et.LIMIT * rg.em_factor(c)
    absln = np.maximum(1.0, twin["absln"].astype(np.float64))
    eg = float(np.max(np.abs(got["g"] - ref["g"]).max(axis=1) / lim))
    eq = float(np.max(np.abs(got["objective"] - ref["objective"]) / absln / lim))
    ew = float(np.max(np.abs(got["wsum"] - ref["wsum"]) / np.maximum(1.0, ref["wsum"]) / lim))
    worst = rg.assert_emfit(got, twin, c, "device")
    print("S = %d, B = %d, %d steps: device against host, g %.2e, objective %.2e, wsum %.2e of the limit; against the twin %.2e"
          % (S, B, steps, eg, eq, ew, worst))
    assert max(eg, eq, ew) <= 1.0 and np.array_equal(got["g"] == 0, ref["g"] == 0)
    if steps:
        # the same steps in launches of one, and a repeated call
        rc, chained = et.call(lib, max_iter=steps, tol=NINF, steps=1, device=device, **c)
        assert rc == 0 and et.same_bits(chained, got)
        rc, again = et.call(lib, max_iter=steps, tol=NINF, device=device, **c)
        assert rc == 0 and et.same_bits(again, got)


def test_emfit_a_replicate_alone_and_in_the_batch(libs, device):
    c = rg.em_case(257, 9)
    lib = libs["emfit"]
    rc, full = et.call(lib, max_iter=3, tol=NINF, device=device, **c)
    assert rc == 0
    for r in (2, 7, 9, 13):
        rc, single = et.call(lib, c["A"], c["scale"], c["w"][r:r + 1], c["mask"], c["g0"][r:r + 1], max_iter=3, tol=NINF, device=device)
        assert rc == 0 and et.same_bits(single, {k: v[r:r + 1] for k, v in full.items()}), r
