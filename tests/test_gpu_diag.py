"""iso_diag_chain (the HIP kernel of libiso_diag.so) on device tensors against the numpy twin: synthetic AR(1) chains
written straight into parameter-major storage, tau / ess / rhat within 1e-9 relative, window and window_ok exactly;
bit-identity of a star's row alone and in a batch; the long shapes again with a window that never closes, so that every
lag sum is seen; the row-major layout, the > 64 KB launch among small ones and the refusal past a CU's LDS through the C
ABI; the diagnostics columns of a real catalog fit; the sampler methods after a single model's fit_mcmc."""
import ctypes as C

import numpy as np
import pytest

import isochrones_amd as ia
from tests import _diag_twin as tw

pytestmark = pytest.mark.gpu


def _device(st, S, W, c=5.0, max_lag=1024):
    import torch
    from isochrones_amd.diagnostics import diag_storage
    out = diag_storage(torch.as_tensor(np.array(st), device="cuda"), S, W, c, max_lag)
    torch.cuda.synchronize()
    return out


SENTINEL = -7.0


def _abi(chain, layout, T, S, W, D, c=5.0, max_lag=1024):
    """(rc, out [S, D, 5] on the device) of iso_diag_chain itself on a device tensor, on the current stream; out starts as
    SENTINEL everywhere."""
    import torch
    from isochrones_amd import _diag_cabi, device as dev
    out = torch.full((S, D, tw.NOUT), SENTINEL, dtype=torch.float64, device=chain.device)
    rc = _diag_cabi.lib().iso_diag_chain(dev.ptr(chain), layout, T, S, W, D, c, max_lag, dev.ptr(out),
                                         dev.stream_ptr(chain.device.index))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", [sh[0] for sh in tw.SHAPES])
def test_kernel_matches_the_twin(name):
    st, (S, D, W, T, max_lag), want = tw.fixture(name)
    got = _device(st, S, W, 5.0, max_lag).cpu().numpy()
    tw.assert_matches(got, want)


@pytest.mark.parametrize("name", tw.LONG_SHAPES)
def test_every_lag_enters_tau(name):
    """tau sums rho(1..M*) only, so at c = 5 a wrong lag sum beyond the window changes nothing.  With c = 1000 the slowest
    parameter's window stays open (open_window asserts window == K, window_ok == 0 on the twin) and all K lags count."""
    st, (S, D, W, T, max_lag), want = tw.open_window(name)
    got = _device(st, S, W, tw.OPEN_C, max_lag).cpu().numpy()
    tw.assert_matches(got, want)


@pytest.mark.parametrize("name", ["plain", "reference", "uneven_tiles"])
def test_row_major_chain_on_the_device(name):
    """ISO_DIAG_ROW_MAJOR ([T][S * W][D]) reaches the kernel through the C ABI only.  The layout changes the addresses a
    tile is staged from, not the order of any sum: the result is the parameter-major one bit for bit."""
    import torch
    from isochrones_amd import _cabi
    st, (S, D, W, T, max_lag), want = tw.fixture(name)
    cols = torch.as_tensor(np.array(st), device="cuda")
    rows = cols.permute(0, 2, 1).contiguous()
    rc, by_param = _abi(cols, _cabi.CHAIN_PARAM_MAJOR, T, S, W, D, 5.0, max_lag)
    assert rc == 0
    rc, by_row = _abi(rows, _cabi.CHAIN_ROW_MAJOR, T, S, W, D, 5.0, max_lag)
    assert rc == 0
    assert torch.equal(by_row.view(torch.int64), by_param.view(torch.int64))
    tw.assert_matches(by_row.cpu().numpy(), want)


def test_large_lds_launch_between_small_ones():
    """The > 64 KB launch raises a function attribute of the kernel; a small launch after it, and the large one again,
    give what they give on their own."""
    import torch
    big, (S, D, W, T, max_lag), want_big = tw.fixture("large_lds")
    small, (s, d, w, t, ml), want_small = tw.fixture("plain")
    assert tw.tile_plan(W, T, max_lag)[2] and not tw.tile_plan(w, t, ml)[2]
    first = _device(big, S, W, 5.0, max_lag)
    between = _device(small, s, w, 5.0, ml)
    third = _device(big, S, W, 5.0, max_lag)
    assert torch.equal(first.view(torch.int64), third.view(torch.int64))
    tw.assert_matches(first.cpu().numpy(), want_big)
    tw.assert_matches(between.cpu().numpy(), want_small)


def test_shape_just_past_a_cus_lds_is_refused():
    """One walker of 16 400 steps needs 164 056 bytes of LDS, 216 more than a CU has: refused on the host with a text,
    before any launch, out untouched.  (near_limit, 160 856 bytes, is answered.)"""
    import torch
    from isochrones_amd import _cabi, _diag_cabi
    with pytest.raises(ValueError, match="exceed a CU's 160 KB"):
        tw.tile_plan(1, 16400, 1024)
    chain = torch.zeros(16400, 1, 1, dtype=torch.float64, device="cuda")
    rc, out = _abi(chain, _cabi.CHAIN_PARAM_MAJOR, 16400, 1, 1, 1)
    assert rc == -1                                                      # ISO_DIAG_ERR_INVALID
    assert "exceed a CU's 160 KB" in _diag_cabi.lib().iso_diag_last_error().decode()
    assert (out == SENTINEL).all()
    with pytest.raises(ia.IsoError, match="exceed a CU's 160 KB"):
        ia.chain_diagnostics(chain, n_ens=1, nwalkers=1)
    torch.cuda.synchronize()                                             # nothing was launched that could fail


def test_two_steps():
    """T = 2: K = 1 and the window closes at M = 1 = T - 1, where tau is zero in exact arithmetic (rho(1) = -1/2): ess is
    W T over rounding noise and is not compared.  No split chain has two steps, so rhat is NaN."""
    st = np.random.default_rng(23).standard_normal((2, 2, 5))
    got = _device(st, 1, 5).cpu().numpy()
    assert got.shape == (1, 2, tw.NOUT)
    assert (got[..., tw.WINDOW] == 1).all() and (got[..., tw.WINDOW_OK] == 1).all()
    assert np.isnan(got[..., tw.RHAT]).all()
    assert (np.abs(got[..., tw.TAU]) <= 1e-12).all(), got[..., tw.TAU]


def test_a_nan_or_an_infinity_anywhere_makes_the_row_nan():
    import torch
    st, (S, D, W, T, max_lag), want = tw.fixture("nonfinite")
    assert np.isnan(want[0, :2]).all() and np.isfinite(want[0, 2]).all()
    got = _device(st, S, W, 5.0, max_lag)
    tw.assert_matches(got.cpu().numpy(), want)
    clean = _device(np.where(np.isfinite(st), st, 0.0), S, W, 5.0, max_lag)   # the finite parameter does not see the others
    assert torch.isfinite(clean).all()
    assert torch.equal(got[0, 2].view(torch.int64), clean[0, 2].view(torch.int64))


def test_other_window_factor_and_max_lag():
    st, (S, D, W, T, _), _ = tw.fixture("reference")
    sub = np.ascontiguousarray(st[:, :2, :W])
    margins = []
    want = tw.storage_diagnostics(sub, 1, W, 3.0, 7, margins)
    tw.check_fixture(want, T, margins)
    tw.assert_matches(_device(sub, 1, W, 3.0, 7).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["reference", "edge_pairs", "plain", "large_lds", "uneven_tiles"])
def test_a_row_is_bit_identical_alone_and_in_a_batch(name):
    import torch
    st, (S, D, W, T, max_lag), _ = tw.fixture(name)
    batch = _device(st, S, W, 5.0, max_lag)
    for s in range(S):
        alone = _device(np.ascontiguousarray(st[:, :, s * W:(s + 1) * W]), 1, W, 5.0, max_lag)
        assert torch.equal(alone[0].view(torch.int64), batch[s].view(torch.int64)), (name, s)
    # and behind other stars, in a larger batch, with one parameter only
    big = np.concatenate([st[:, :1, :W]] * 3 + [st[:, :1, :]], axis=2)
    far = _device(big, S + 3, W, 5.0, max_lag)
    assert torch.equal(far[3:, 0].view(torch.int64), batch[:, 0].view(torch.int64))


def test_chain_views_and_refusals():
    import torch
    st, (S, D, W, T, max_lag), want = tw.fixture("plain")
    storage = torch.as_tensor(np.array(st), device="cuda")
    view = storage.view(T, D, S, W).permute(2, 3, 0, 1)                  # what sampler.chain returns: no copy is made
    r = ia.chain_diagnostics(view)
    assert r.tau.shape == (S, D) and r.tau.is_cuda
    tw.assert_matches(torch.stack(list(r), dim=-1).cpu().numpy(), want)
    r1 = ia.chain_diagnostics(view[2].contiguous())                      # a [W, T, D] chain in its own memory
    tw.assert_matches(torch.stack(list(r1), dim=-1).cpu().numpy(), want[2])
    r2 = ia.chain_diagnostics(storage, n_ens=S, nwalkers=W)
    assert torch.equal(r2.ess.view(torch.int64), r.ess.view(torch.int64))
    # a series too long for the kernel's LDS staging is refused with a text, not answered
    long = torch.zeros(20481, 1, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ia.IsoError, match="nsteps too large"):
        ia.chain_diagnostics(long, n_ens=1, nwalkers=2)
    with pytest.raises(ValueError):
        ia.chain_diagnostics(storage.float(), n_ens=S, nwalkers=W)


def _small_track(bands=("G", "BP", "RP")):
    fehs = np.array([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5])
    masses = ia.grids.mist_masses()[25:140:2]
    eeps = np.arange(150.0, 700.0)
    return ia.synthetic_track(bands=bands, fehs=fehs, masses=masses, eeps=eeps, eep_bounds=(150, 699),
                              limits=dict(mass=(masses[0], masses[-1]), feh=(-1.0, 0.5), age=(5, 10.13)))


def test_catalog_fit_with_diagnostics_columns():
    import torch
    from isochrones_amd.catalog import fit_stars_gpu, result_columns, synthetic_catalog
    ic = _small_track()
    cat, _ = synthetic_catalog(ic, 8, bands=["G", "BP", "RP"], seed=5, mag_unc=0.01)
    idx = np.arange(8)
    kw = dict(nwalkers=32, nburn=20, niter=40, seed=3)
    base = fit_stars_gpu(cat, ic, idx, **kw)
    rows, chain, _ = fit_stars_gpu(cat, ic, idx, diagnostics=True, return_chains=True, **kw)
    names = tuple(ic.param_names)
    D = len(names)
    cols = result_columns(names, diagnostics=True)
    assert cols[: 3 * D + 2] == result_columns(names)[: 3 * D + 2] and cols[-1] == "ok"
    assert cols[3 * D + 2: 3 * D + 5] == ["%s_%s" % (names[0], s) for s in ("tau", "ess", "rhat")]
    assert cols[-4:-1] == ["tau_max", "rhat_max", "window_ok"]
    assert rows.shape == (8, len(cols)) == (8, 6 * D + 6) and base.shape == (8, 3 * D + 3)
    assert np.array_equal(rows[:, : 3 * D + 2], base[:, : 3 * D + 2], equal_nan=True)
    assert np.array_equal(rows[:, -1], base[:, -1]) and rows[:, -1].all()
    assert chain.shape == (8, 32, 40, D)
    r = ia.chain_diagnostics(chain)
    want = torch.stack([r.tau, r.ess, r.rhat], dim=2).reshape(8, 3 * D).cpu().numpy()
    d0 = 3 * D + 2
    assert np.array_equal(rows[:, d0: d0 + 3 * D], want, equal_nan=True)
    assert np.array_equal(rows[:, d0 + 3 * D], r.tau.amax(dim=1).cpu().numpy(), equal_nan=True)
    assert np.array_equal(rows[:, d0 + 3 * D + 1], r.rhat.amax(dim=1).cpu().numpy(), equal_nan=True)
    assert np.array_equal(rows[:, d0 + 3 * D + 2], r.window_ok.amin(dim=1).cpu().numpy(), equal_nan=True)
    # the same numbers from the twin on the chain that came back
    st = chain.permute(2, 3, 0, 1).reshape(40, D, 8 * 32).cpu().numpy()
    margins = []
    twin = tw.storage_diagnostics(st, 8, 32, 5.0, 1024, margins)
    tw.check_fixture(twin, 40, margins)
    tw.assert_matches(torch.stack(list(r), dim=-1).cpu().numpy(), twin)
    with pytest.raises(ValueError):
        fit_stars_gpu(cat, ic, idx, diagnostics=True, fused=False, **kw)


def test_fit_catalog_passes_the_switch_through():
    from isochrones_amd.catalog import fit_catalog, result_columns, synthetic_catalog
    ic = _small_track()
    cat, _ = synthetic_catalog(ic, 8, bands=["G", "BP", "RP"], seed=5, mag_unc=0.01)
    kw = dict(nwalkers=32, nburn=20, niter=40, seed=3)
    plain = fit_catalog(cat, ic, **kw)
    off = fit_catalog(cat, ic, diagnostics=False, **kw)
    on = fit_catalog(cat, ic, diagnostics=True, **kw)
    assert list(off.columns) == list(plain.columns) and np.array_equal(off.values, plain.values, equal_nan=True)
    assert "diag_s" not in plain.attrs["timings"]["phases"] and "diag_s" not in off.attrs["timings"]["phases"]
    assert on.attrs["timings"]["phases"]["diag_s"] > 0
    assert list(on.columns) == result_columns(tuple(ic.param_names), diagnostics=True)
    assert np.array_equal(on[list(plain.columns)].values, plain.values, equal_nan=True)
    assert np.isfinite(on["tau_max"]).all() and (on["rhat_max"] > 0.9).all()
    with pytest.raises(ValueError):
        fit_catalog(cat, ic, method="nested", diagnostics=True)


def test_sampler_methods_after_a_single_model_fit():
    import torch
    from isochrones_amd.sampler import FusedEnsembleSampler
    ic = _small_track()
    mod = ia.SingleStarModel(ic, Teff=(5770, 100), logg=(4.4, 0.1), feh=(0.0, 0.15), G=(10.0, 0.05), parallax=(10.0, 0.1))
    fresh = FusedEnsembleSampler(mod, 32, seed=1)
    for call in (fresh.get_autocorr_time, fresh.effective_sample_size, fresh.split_rhat, fresh.diagnostics):
        with pytest.raises(ValueError, match="no stored chain"):
            call()
    mod.fit_mcmc(nwalkers=32, nburn=20, niter=40, seed=2, fused=True)
    s = mod.sampler
    assert isinstance(s, FusedEnsembleSampler)
    tau = s.get_autocorr_time()
    assert tau.shape == (s.ndim,) and tau.is_cuda
    st = s._chain.cpu().numpy()
    margins = []
    twin = tw.storage_diagnostics(st, 1, 32, 5.0, 1024, margins)[0]
    tw.check_fixture(twin, 40, margins)
    d = s.diagnostics()
    tw.assert_matches(torch.stack(list(d), dim=-1).cpu().numpy(), twin)
    assert torch.equal(tau, d.tau) and torch.equal(s.effective_sample_size(), d.ess)
    assert torch.equal(s.split_rhat().view(torch.int64), d.rhat.view(torch.int64))
    short = s.get_autocorr_time(c=3.0, max_lag=5)
    assert short.shape == tau.shape
