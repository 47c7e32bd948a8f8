"""The Python surface of the posterior-predictive check that needs no device: column order, argument checks."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import catalog as cat, predictive as pv
from tests import _predict_twin as tw


def test_result_columns_order():
    names = ["mass", "eep", "feh", "distance", "AV"]
    base = cat.result_columns(names)
    cols = cat.result_columns(names, diagnostics=True, derived=("radius",), predictive=("V", "J"))
    tail = ["radius_median", "radius_p16", "radius_p84", "ppc", "ppc_nbad", "V_mag_median", "V_mag_p16", "V_mag_p84",
            "J_mag_median", "J_mag_p16", "J_mag_p84", "chi2_V", "chi2_J", "chi2_Teff", "chi2_logg", "chi2_feh",
            "chi2_parallax", "map_mass", "map_eep", "map_feh", "map_distance", "map_AV", "ok"]
    assert cols[-len(tail):] == tail and cols[:len(base) - 1] == base[:-1]
    assert cat.result_columns(names, predictive=()) == base and len(set(cols)) == len(cols)


def test_fit_catalog_refuses_nested_and_unfused():
    ic = tw.ichrone("track")
    import pandas as pd
    df = pd.DataFrame({"V_mag": [10.0, 11.0], "V_mag_unc": [0.02, 0.02], "parallax": [5.0, 4.0], "parallax_unc": [0.1, 0.1]})
    c = cat.StarCatalog(df, bands=("V",), props=("parallax",))
    with pytest.raises(ValueError, match="predictive is for method='mcmc'"):
        cat.fit_catalog(c, ic, method="nested", predictive=True)
    with pytest.raises(ValueError, match="predictive needs the fused sampler"):
        cat.fit_catalog(c, ic, predictive=True, fused=False)
    with pytest.raises(ValueError, match="predictive needs the fused sampler"):
        cat.fit_stars_gpu(c, ic, np.arange(2), predictive=True, fused=False)


def test_predict_storage_checks_before_any_device_call():
    import torch
    ic = tw.ichrone("track")
    obs = (np.zeros((2, 7)), np.ones((2, 7)))
    with pytest.raises(ValueError, match="float64 CUDA tensor"):
        pv.predict_storage(torch.zeros(4, 5, 20, dtype=torch.float64), None, 2, 10, ic, ("V", "J", "K"), obs)
    with pytest.raises(ValueError, match="float64 CUDA tensor"):
        pv.predict_storage(torch.zeros(4, 5, 20, dtype=torch.float32), None, 2, 10, ic, ("V", "J", "K"), obs)
    with pytest.raises(ValueError, match="float64 CUDA tensor"):
        pv.chain_predictive(torch.zeros(2, 10, 4, 5, dtype=torch.float64), None, ic, ("V",), obs)
    meta = torch.zeros(4, 5, 20, dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match="band"):
        pv.predict_storage(meta, None, 2, 10, ic, ("nope",), obs)
    with pytest.raises(ValueError, match="1 to 32 bands"):
        pv.predict_storage(meta, None, 2, 10, ic, (), obs)

    class FakeCuda(torch.Tensor):
        is_cuda = True
    fake = torch.zeros(4, 5, 20, dtype=torch.float64).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="n_ens \\* nwalkers"):
        pv.predict_storage(fake, None, 3, 10, ic, ("V", "J", "K"), obs)
    with pytest.raises(ValueError, match="B \\+ 4"):
        pv.predict_storage(fake, None, 2, 10, ic, ("V", "J", "K"), (np.zeros((2, 6)), np.ones((2, 6))))
    with pytest.raises(ValueError, match="range"):
        pv.predict_storage(fake, None, 2, 10, ic, ("V", "J", "K"), obs, ens_begin=1, n_ens_out=2)


def test_pack_obs_forms():
    val, unc = pv.pack_obs({"V": (10.0, 0.1), "Teff": (5800.0, 80.0)}, ("V", "J"), 2)
    assert val.shape == (2, 6) and val[1, 0] == 10.0 and np.isnan(val[0, 1]) and val[0, 2] == 5800.0 and unc[1, 2] == 80.0
    cols = dict(mag_val=np.array([[1.0, np.nan]]), mag_unc=np.ones((1, 2)), spec_val=np.full((1, 3), np.nan),
                spec_unc=np.full((1, 3), np.nan), has_plx=np.array([1], dtype=np.int32), plx_val=np.array([4.0]),
                plx_unc=np.array([0.2]))
    val, unc = pv.pack_obs(cols, ("V", "J"), 1)
    np.testing.assert_array_equal(np.isnan(val[0]), [False, True, True, True, True, False])
    assert val[0, 5] == 4.0 and unc[0, 5] == 0.2
    assert pv.result_labels(("V",), ["a"]) == ["ppc", "ppc_nbad", "V_mag_median", "V_mag_p16", "V_mag_p84", "chi2_V",
                                               "chi2_Teff", "chi2_logg", "chi2_feh", "chi2_parallax", "map_a"]
    assert ia.chain_predictive is pv.chain_predictive
