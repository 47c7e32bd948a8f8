"""iso_derived_chain (the HIP kernel of libiso_derived.so) on device tensors against the numpy twin, bit identity of a
star's derived values across batch, ensemble range and layout, the call forms of ia.chain_derived, the derived columns of
a real catalog fit against numpy.percentile of the derived chain, budget slicing, NaN reporting, a binary (N = 2) and the
sampler methods after a single model's fit_mcmc."""
import numpy as np
import pytest

import isochrones_amd as ia
from tests import _derived_twin as tw
from tests._derived_gpu import device as _device, host as _host

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("S,W,T", tw.GPU_SHAPES)
def test_kernel_matches_the_twin_and_the_host_entry(S, W, T):
    for Q in tw.QS:
        for Cn in tw.CS:
            kind = "track" if (Q + Cn) % 2 else "iso"
            cols, axes = tw.packed(kind, Q)
            x = np.array(tw.chain(kind, S, W, T))
            comps = tw.comps_for(Cn)
            want, want_nan = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
            got, nan_count = _device(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
            assert tw.close(got, want), (Q, Cn)
            np.testing.assert_array_equal(nan_count, want_nan)
            host, host_nan = _host(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
            assert tw.close(got, host), (Q, Cn)
            np.testing.assert_array_equal(nan_count, host_nan)


@pytest.mark.parametrize("S,W,T", [(3, 10, 7), (5, 26, 4)])
def test_a_star_is_bit_identical_alone_in_a_batch_in_a_range_and_in_either_layout(S, W, T):
    for Q, Cn in ((1, 1), (3, 2), (8, 3), (4, 2)):
        cols, axes = tw.packed("track", Q)
        x = np.array(tw.chain("track", S, W, T))
        comps = tw.comps_for(Cn)
        full, full_nan = _device(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
        rows = np.ascontiguousarray(x.transpose(0, 2, 1))
        got_r, nan_r = _device(rows, tw.ROW_MAJOR, S, W, cols, axes, comps)
        np.testing.assert_array_equal(_bits(got_r), _bits(full))
        np.testing.assert_array_equal(nan_r, full_nan)
        for b, n in ((0, S), (1, 2), (S - 1, 1)):
            sub, nan_sub = _device(x, tw.PARAM_MAJOR, S, W, cols, axes, comps, ens_begin=b, n_out=n)
            np.testing.assert_array_equal(_bits(sub), _bits(full[:, :, b * W:(b + n) * W]))
            np.testing.assert_array_equal(nan_sub, full_nan[b:b + n])
        for s in range(S):
            alone, nan_alone = _device(np.ascontiguousarray(x[:, :, s * W:(s + 1) * W]), tw.PARAM_MAJOR, 1, W, cols, axes, comps)
            np.testing.assert_array_equal(_bits(alone), _bits(full[:, :, s * W:(s + 1) * W]))
            np.testing.assert_array_equal(nan_alone[0], full_nan[s])


def test_device_entry_refuses_bad_arguments():
    cols, axes = tw.packed("iso", 3)
    x = np.array(tw.chain("iso", 3, 10, 7))
    for kw, comps in ((dict(ens_begin=2, n_out=2), [(2, 3, 0)]), (dict(), [(2, 6, 0)]), (dict(), [(2, 3, 0)] * 4)):
        with pytest.raises(ia.IsoError, match="iso_derived_chain"):
            _device(x, tw.PARAM_MAJOR, 3, 10, cols, axes, comps, **kw)


def _small_track(bands=("G", "BP", "RP")):
    fehs = np.array([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5])
    masses = ia.grids.mist_masses()[25:140:2]
    eeps = np.arange(150.0, 700.0)
    return ia.synthetic_track(bands=bands, fehs=fehs, masses=masses, eeps=eeps, eep_bounds=(150, 699),
                              limits=dict(mass=(masses[0], masses[-1]), feh=(-1.0, 0.5), age=(5, 10.13)))


def _track_storage(ic, S, W, T, seed=0):
    """Parameter-major storage [T, 5, S * W] of (mass, eep, feh, distance, AV) drawn inside the table."""
    rng = np.random.default_rng(seed)
    fehs, masses, eeps = ic.model_grid.interp.index_columns
    x = np.empty((T, 5, S * W))
    x[:, 0] = rng.uniform(masses[2], masses[-3], (T, S * W))
    x[:, 1] = rng.uniform(200.0, 400.0, (T, S * W))
    x[:, 2] = rng.uniform(fehs[0], fehs[-1], (T, S * W))
    x[:, 3] = 100.0
    x[:, 4] = 0.1
    return x


def _bare_sampler(storage, S, W, stacked=True):
    """A FusedEnsembleSampler that holds ``storage`` as its stored chain and nothing else (no native sampler behind it)."""
    from isochrones_amd.sampler import FusedEnsembleSampler
    s = object.__new__(FusedEnsembleSampler)
    s._h = None
    s._chain, s.n_ensembles, s.nwalkers, s.ndim = storage, S, W, storage.shape[1]
    s.is_catalog, s.multi_ensemble = stacked, False
    s.device, s.device_index = storage.device, storage.device.index
    return s


def test_chain_derived_call_forms():
    import torch
    ic = _small_track()
    S, W, T = 3, 10, 7
    x = _track_storage(ic, S, W, T)
    storage = torch.as_tensor(x, device="cuda")
    view = storage.view(T, 5, S, W).permute(2, 3, 0, 1)                     # what sampler.chain returns
    # the view goes to the kernel as it lies: no copy is made on the way
    assert view.permute(2, 3, 0, 1).contiguous().data_ptr() == storage.data_ptr()
    props = ("radius", "Teff", ("mass_now", "mass"))
    d, names = ia.chain_derived(view, ic, props)
    assert names == ("radius", "Teff", "mass_now") and d.shape == (S, W, T, 3) and d.is_cuda
    g = ic.model_grid.interp
    cols = np.ascontiguousarray(g.grid[..., [g.column_index[c] for c in ("radius", "Teff", "mass")]])
    want, _ = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, g.index_columns, [(2, 0, 1)])
    want = want.reshape(T, 3, S, W).transpose(2, 3, 0, 1)
    assert tw.close(d.cpu().numpy(), want) and np.isfinite(want).all()
    d1, _ = ia.chain_derived(view[2].contiguous(), ic, props)              # a [W, T, D] chain in its own memory
    assert d1.shape == (W, T, 3) and torch.equal(d1.view(torch.int64), d[2].view(torch.int64))
    d2, names2 = ia.chain_derived(storage, ic, props, n_ens=S, nwalkers=W)
    assert names2 == names and torch.equal(d2.view(torch.int64), d.view(torch.int64))
    # the packed table is made once per (device, columns) and dropped by release()
    key = (storage.device.index, ("radius", "Teff", "mass"))
    first = ic._derived_tables[key][1][0]
    ia.chain_derived(view, ic, props)
    assert ic._derived_tables[key][1][0] is first
    with pytest.raises(ValueError, match="float64"):
        ia.chain_derived(storage.float(), ic, props, n_ens=S, nwalkers=W)
    with pytest.raises(ValueError, match=r"\(label, column\)"):
        ia.chain_derived(view, ic, ("mass",))
    with pytest.raises(ValueError):
        ia.chain_derived(storage, ic, props, n_ens=S)
    # more than 8 columns: several launches, the same values
    many = ("radius", "Teff", "logg", "logL", "Mbol", "density", "age", "logTeff", "phase", ("mass_now", "mass"))
    dm, nm = ia.chain_derived(view, ic, many)
    assert dm.shape == (S, W, T, 10) and nm[-1] == "mass_now"
    assert torch.equal(dm[..., 0].view(torch.int64), d[..., 0].view(torch.int64))
    assert torch.equal(dm[..., 9].view(torch.int64), d[..., 2].view(torch.int64))
    ic.release()
    assert "_derived_tables" not in ic.__dict__


@pytest.fixture(scope="module")
def fitted():
    """The 8-star catalog tests/test_gpu_diag.py fits, with and without the switch."""
    from isochrones_amd.catalog import fit_stars_gpu, synthetic_catalog
    ic = _small_track()
    cat, _ = synthetic_catalog(ic, 8, bands=["G", "BP", "RP"], seed=5, mag_unc=0.01)
    idx = np.arange(8)
    kw = dict(nwalkers=32, nburn=20, niter=40, seed=3)
    props = ("radius", "Teff", ("mass_now", "mass"))
    base = fit_stars_gpu(cat, ic, idx, **kw)
    timings = {}
    rows, chain, _ = fit_stars_gpu(cat, ic, idx, derived=props, return_chains=True, timings=timings, **kw)
    return dict(ic=ic, cat=cat, idx=idx, kw=kw, props=props, base=base, rows=rows, chain=chain, timings=timings)


def _percentiles(d):
    """[S, W, T, K] derived chain on the host -> [S, 3 K] in result-row order."""
    S, K = d.shape[0], d.shape[3]
    return np.stack([np.percentile(d[s, :, :, j].ravel(), [50, 16, 84]) for s in range(S) for j in range(K)]).reshape(S, 3 * K)


def test_catalog_fit_with_derived_columns(fitted):
    from isochrones_amd.catalog import fit_stars_gpu, result_columns
    ic, base, rows, chain, props = (fitted[k] for k in ("ic", "base", "rows", "chain", "props"))
    names = tuple(ic.param_names)
    D = len(names)
    cols = result_columns(names, derived=("radius", "Teff", "mass_now"))
    assert rows.shape == (8, len(cols)) == (8, 3 * D + 3 + 9) and base.shape == (8, 3 * D + 3)
    assert np.array_equal(rows[:, : 3 * D + 2], base[:, : 3 * D + 2], equal_nan=True)
    assert np.array_equal(rows[:, -1], base[:, -1]) and rows[:, -1].all()            # all 8 stars ok, none hidden
    assert chain.shape == (8, 32, 40, D) and "derived" in fitted["timings"]
    d, labels = ia.chain_derived(chain, ic, props)
    assert labels == ("radius", "Teff", "mass_now")
    dh = d.cpu().numpy()
    assert np.isfinite(dh).all()
    np.testing.assert_array_equal(_bits(rows[:, 3 * D + 2: -1]), _bits(_percentiles(dh)))
    # the derived chain is the interpolator's own answer on the same samples
    flat = chain.reshape(-1, D).cpu().numpy()
    want = ic.interp_value([flat[:, 0], flat[:, 1], flat[:, 2]], ["radius", "Teff", "mass"])
    assert tw.close(dh.reshape(-1, 3), np.asarray(want))
    # with the diagnostics columns in front
    both, chain2, _ = fit_stars_gpu(fitted["cat"], ic, fitted["idx"], derived=props, diagnostics=True, return_chains=True,
                                    **fitted["kw"])
    cols2 = result_columns(names, diagnostics=True, derived=labels)
    assert both.shape == (8, len(cols2)) and cols2[-10:-1] == cols[-10:-1]
    assert np.array_equal(both[:, : 3 * D + 2], base[:, : 3 * D + 2], equal_nan=True) and both[:, -1].all()
    np.testing.assert_array_equal(_bits(both[:, -10:-1]), _bits(rows[:, -10:-1]))
    assert cols2[-13:-10] == ["tau_max", "rhat_max", "window_ok"] and np.isfinite(both[:, -13:-10]).all()
    with pytest.raises(ValueError):
        fit_stars_gpu(fitted["cat"], ic, fitted["idx"], derived=props, fused=False, **fitted["kw"])


def test_fit_catalog_passes_the_switch_through(fitted):
    from isochrones_amd.catalog import fit_catalog, result_columns
    ic, cat, kw = fitted["ic"], fitted["cat"], fitted["kw"]
    plain = fit_catalog(cat, ic, **kw)
    off = fit_catalog(cat, ic, derived=None, **kw)
    on = fit_catalog(cat, ic, derived=fitted["props"], max_stars_per_batch=8, **kw)
    assert list(off.columns) == list(plain.columns) and np.array_equal(off.values, plain.values, equal_nan=True)
    assert "derived_s" not in plain.attrs["timings"]["phases"] and "derived_s" not in off.attrs["timings"]["phases"]
    assert on.attrs["timings"]["phases"]["derived_s"] > 0
    assert list(on.columns) == result_columns(tuple(ic.param_names), derived=("radius", "Teff", "mass_now"))
    assert np.array_equal(on[list(plain.columns)].values, plain.values, equal_nan=True)
    np.testing.assert_array_equal(_bits(on.values), _bits(fitted["rows"]))
    auto = fit_catalog(cat, ic, derived=True, **kw)
    assert [c for c in auto.columns if c not in plain.columns] == [
        "%s_%s" % (l, s) for l in ("radius", "age", "Teff", "logg") for s in ("median", "p16", "p84")]
    np.testing.assert_array_equal(_bits(auto["radius_median"].values), _bits(on["radius_median"].values))
    # through the max_stars_per_batch slicing: other seeds per slice, so only shape and finiteness are compared
    sliced = fit_catalog(cat, ic, derived=("radius",), max_stars_per_batch=3, **kw)
    assert sliced.shape == (8, len(plain.columns) + 3) and np.isfinite(sliced["radius_p84"]).all()
    with pytest.raises(ValueError):
        fit_catalog(cat, ic, method="nested", derived=("radius",))
    with pytest.raises(ValueError):
        fit_catalog(cat, ic, fused=False, derived=("radius",), **kw)


def test_budget_slicing_returns_the_same_bits(fitted):
    import torch
    ic, chain, props = fitted["ic"], fitted["chain"], fitted["props"]
    S, W, T, D = chain.shape
    storage = chain.permute(2, 3, 0, 1).reshape(T, D, S * W).contiguous()
    s = _bare_sampler(storage, S, W)
    q1, n1 = s.derived_quantiles(ic, props)
    assert q1.shape == (S, 3, 3) and n1.shape == (S, 3) and n1.dtype == torch.int32 and int(n1.abs().sum()) == 0
    np.testing.assert_array_equal(_bits(q1.reshape(S, 9).cpu().numpy()), _bits(fitted["rows"][:, 3 * D + 2: -1]))
    per_ens = T * 3 * W * 8
    q3, n3 = s.derived_quantiles(ic, props, budget_bytes=3 * per_ens + 5)          # 3 + 3 + 2 stars
    assert torch.equal(q3.view(torch.int64), q1.view(torch.int64)) and torch.equal(n3, n1)
    with pytest.raises(ValueError, match="budget"):
        s.derived_quantiles(ic, props, budget_bytes=per_ens - 1)
    with pytest.raises(ValueError, match="8 quantile levels"):
        s.derived_quantiles(ic, props, q=np.linspace(0.1, 0.9, 9))
    d, names = s.derived(ic, props)
    assert d.shape == (S, W, T, 3) and names == ("radius", "Teff", "mass_now")
    five = s.derived_quantiles(ic, ("radius",), q=(0.05, 0.25, 0.5, 0.75, 0.95))[0]
    want = np.stack([np.percentile(d[k, :, :, 0].cpu().numpy().ravel(), [5, 25, 50, 75, 95]) for k in range(S)])
    np.testing.assert_array_equal(_bits(five[:, 0].cpu().numpy()), _bits(want))


def test_nan_reporting_is_per_star_and_column():
    import torch
    # a table that reaches the ragged end of the tracks (the small one of the catalog tests has no NaN padding)
    ic = ia.synthetic_track(bands=("G", "BP", "RP"), fehs=np.array([-0.5, 0.0, 0.5]), masses=ia.grids.mist_masses()[25:140:8],
                            eeps=np.arange(150.0, 1710.0, 8.0))
    g = ic.model_grid.interp
    fehs, masses, eeps = g.index_columns
    rad = g.grid[..., g.column_index["radius"]]
    # a cell whose eight corners are finite next to one, higher in EEP, with a NaN corner (the ragged end of a track)
    fin = np.isfinite(rad)
    cell_ok = (fin[:-1, :-1, :-1] & fin[1:, :-1, :-1] & fin[:-1, 1:, :-1] & fin[1:, 1:, :-1]
               & fin[:-1, :-1, 1:] & fin[1:, :-1, 1:] & fin[:-1, 1:, 1:] & fin[1:, 1:, 1:])
    edge = np.argwhere(cell_ok[:, :, :-1] & ~cell_ok[:, :, 1:])
    assert len(edge), "the table has no ragged end"
    i, j, k = (int(v) for v in edge[0])
    S, W, T = 4, 10, 6
    x = np.empty((T, 5, S * W))
    rng = np.random.default_rng(1)
    x[:, 0] = rng.uniform(masses[j], masses[j + 1], (T, S * W))
    x[:, 2] = rng.uniform(fehs[i], fehs[i + 1], (T, S * W))
    x[:, 1] = rng.uniform(eeps[k], eeps[k + 1], (T, S * W))                  # every star inside the finite cell ...
    x[:, 3:] = 1.0
    clean = torch.as_tensor(x, device="cuda")
    x[:, 1, 2 * W:3 * W] = rng.uniform(eeps[k + 1] + 0.25, eeps[k + 1] + 0.75, (T, W))     # ... star 2 inside the cell above
    dirty = torch.as_tensor(x, device="cuda")
    props = ("radius", "Teff")
    q0, n0 = _bare_sampler(clean, S, W).derived_quantiles(ic, props)
    q1, n1 = _bare_sampler(dirty, S, W).derived_quantiles(ic, props)
    assert int(n0.abs().sum()) == 0 and bool(torch.isfinite(q0).all())
    assert n1[2].tolist() == [T * W, T * W] and int(n1.sum()) == 2 * T * W
    assert bool(torch.isnan(q1[2]).all())
    keep = [0, 1, 3]
    assert torch.equal(q1[keep].view(torch.int64), q0[keep].view(torch.int64))


def test_a_binary_on_an_isochrone_table():
    import torch
    iso = ia.synthetic_isochrone(bands=("J", "K"), ages=[9.0, 9.3, 9.6, 10.0], fehs=[-0.5, 0.0, 0.5], eeps=np.arange(250.0, 420.0))
    g = iso.model_grid.interp
    ages, fehs, eeps = g.index_columns
    S, W, T = 2, 12, 5
    rng = np.random.default_rng(4)
    x = np.empty((T, 6, S * W))                                              # (eep_0, eep_1, age, feh, distance, AV)
    x[:, 0] = rng.uniform(eeps[0], eeps[-1], (T, S * W))
    x[:, 1] = rng.uniform(eeps[0], eeps[-1], (T, S * W))
    x[:, 2] = rng.uniform(ages[0], ages[-1], (T, S * W))
    x[:, 3] = rng.uniform(fehs[0], fehs[-1], (T, S * W))
    x[:, 4:] = 1.0
    d, names = ia.chain_derived(torch.as_tensor(x, device="cuda"), iso, ("radius", "mass"), N=2, n_ens=S, nwalkers=W)
    assert names == ("radius_0", "mass_0", "radius_1", "mass_1") and d.shape == (S, W, T, 4)
    cols = np.ascontiguousarray(g.grid[..., [g.column_index["radius"], g.column_index["mass"]]])
    want, _ = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, g.index_columns, [(2, 3, 0), (2, 3, 1)])
    assert tw.close(d.cpu().numpy(), want.reshape(T, 4, S, W).transpose(2, 3, 0, 1))
    assert np.isfinite(want).sum() > want.size // 2


def test_sampler_methods_after_a_single_model_fit():
    from isochrones_amd.sampler import FusedEnsembleSampler
    ic = _small_track()
    mod = ia.SingleStarModel(ic, Teff=(5770, 100), logg=(4.4, 0.1), feh=(0.0, 0.15), G=(10.0, 0.05), parallax=(10.0, 0.1))
    fresh = FusedEnsembleSampler(mod, 32, seed=1)
    for call in (fresh.derived, fresh.derived_quantiles):
        with pytest.raises(ValueError, match="no stored chain"):
            call(ic, ("radius",))
    mod.fit_mcmc(nwalkers=32, nburn=20, niter=40, seed=2, fused=True)
    s = mod.sampler
    assert isinstance(s, FusedEnsembleSampler)
    q, n = s.derived_quantiles(ic, ("radius",))
    assert q.shape == (1, 3) and n.shape == (1,) and int(n[0]) == 0
    d, names = s.derived(ic, ("radius",))
    assert d.shape == (32, 40, 1) and names == ("radius",)
    want = np.percentile(d[:, :, 0].cpu().numpy().ravel(), [50, 16, 84])
    np.testing.assert_array_equal(_bits(q[0].cpu().numpy()), _bits(want))
