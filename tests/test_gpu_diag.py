"""iso_diag_chain (the HIP kernel of libiso_diag.so) on device tensors against the numpy twin: synthetic AR(1) chains
written straight into parameter-major storage, tau / ess / rhat within 1e-9 relative, window and window_ok exactly;
bit-identity of a star's row alone and in a batch; the diagnostics columns of a real catalog fit; the sampler methods
after a single model's fit_mcmc."""
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


@pytest.mark.parametrize("name", [sh[0] for sh in tw.SHAPES])
def test_kernel_matches_the_twin(name):
    st, (S, D, W, T, max_lag), want = tw.fixture(name)
    got = _device(st, S, W, 5.0, max_lag).cpu().numpy()
    tw.assert_matches(got, want)


def test_other_window_factor_and_max_lag():
    st, (S, D, W, T, _), _ = tw.fixture("reference")
    sub = np.ascontiguousarray(st[:, :2, :W])
    margins = []
    want = tw.storage_diagnostics(sub, 1, W, 3.0, 7, margins)
    tw.check_fixture(want, T, margins)
    tw.assert_matches(_device(sub, 1, W, 3.0, 7).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["reference", "edge_pairs", "plain"])
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
