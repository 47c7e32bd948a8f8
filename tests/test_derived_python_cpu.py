"""Host logic of isochrones_amd.derived and of the catalog's ``derived`` switch that needs no device: result columns,
labels, refusals, what ``derived=True`` means for each grid kind, the component triples."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import derived as dv
from isochrones_amd.catalog import _derived_request, result_columns


def _track():
    return ia.synthetic_track(bands=("J",), fehs=np.array([-0.5, 0.0, 0.5]), masses=np.array([0.8, 1.0, 1.2]),
                              eeps=np.arange(300.0, 340.0))


def _iso():
    return ia.synthetic_isochrone(bands=("J", "K"), ages=[9.0, 9.5, 10.0], fehs=[-0.5, 0.0, 0.5], eeps=np.arange(300.0, 340.0))


def test_result_columns_with_derived():
    names = ("mass", "eep", "feh", "distance", "AV")
    base = result_columns(names)
    assert result_columns(names, derived=()) == base and result_columns(names, diagnostics=False, derived=()) == base
    assert base[-3:] == ["lnpost_max", "acceptance", "ok"] and len(base) == 18
    cols = result_columns(names, derived=("radius", "mass_now"))
    assert cols[:17] == base[:17] and cols[-1] == "ok"
    assert cols[17:-1] == ["radius_median", "radius_p16", "radius_p84", "mass_now_median", "mass_now_p16", "mass_now_p84"]
    diag = result_columns(names, diagnostics=True)
    both = result_columns(names, diagnostics=True, derived=("radius",))
    assert both[:len(diag) - 1] == diag[:-1] and both[len(diag) - 1:] == ["radius_median", "radius_p16", "radius_p84", "ok"]
    # N = 2: the caller passes the expanded labels
    names2 = ("eep_0", "eep_1", "age", "feh", "distance", "AV")
    labels = dv.expand_labels(("radius", "Teff"), 2)
    assert labels == ("radius_0", "Teff_0", "radius_1", "Teff_1")
    cols2 = result_columns(names2, derived=labels)
    assert cols2[-13:-1] == ["%s_%s" % (l, s) for l in labels for s in ("median", "p16", "p84")] and cols2[-1] == "ok"
    assert dv.expand_labels(("radius",), 1) == ("radius",)


def test_default_props_and_components_per_grid_kind():
    trk, iso = _track(), _iso()
    # a track fit samples the initial mass under the name "mass": the grid's current-mass column is not offered under it
    assert dv.default_props(trk) == ("radius", "age", "Teff", "logg")
    assert dv.default_props(iso) == ("mass", "radius", "Teff", "logg")
    assert dv.default_props(iso, 2) == ("mass", "radius", "Teff", "logg")
    assert dv.components(trk) == [(2, 0, 1)] and dv.components(iso) == [(1, 2, 0)]
    assert dv.components(iso, 2) == [(2, 3, 0), (2, 3, 1)]
    assert dv.components(iso, 3) == [(3, 4, 0), (3, 4, 1), (3, 4, 2)]
    with pytest.raises(ValueError):
        dv.components(trk, 2)
    with pytest.raises(ValueError):
        dv.components(iso, 4)
    assert dv.fit_param_names(iso, 2) == ("eep_0", "eep_1", "age", "feh", "distance", "AV")
    assert _derived_request(trk, True, 1) == (("radius", "age", "Teff", "logg"), ("radius", "age", "Teff", "logg"))
    assert _derived_request(iso, ("radius", ("m", "mass")), 2) == (("radius", ("m", "mass")), ("radius_0", "m_0", "radius_1", "m_1"))
    for off in (None, False, (), []):
        assert _derived_request(trk, off, 1) == ((), ())


def test_refusals():
    trk, iso = _track(), _iso()
    with pytest.raises(ValueError, match=r"\(label, column\)"):
        dv.resolve_props(trk, ("radius", "mass"))
    with pytest.raises(ValueError, match=r"\(label, column\)"):
        dv.resolve_props(iso, ("age",))
    with pytest.raises(ValueError, match=r"\(label, column\)"):
        dv.resolve_props(iso, (("eep_1", "radius"),), N=2)
    assert dv.resolve_props(trk, ("radius", ("mass_now", "mass"))) == (("radius", "mass_now"), ("radius", "mass"))
    assert dv.resolve_props(iso, ("mass",)) == (("mass",), ("mass",))
    with pytest.raises(ValueError, match="no column"):
        dv.resolve_props(trk, ("luminosity",))
    with pytest.raises(ValueError, match="twice"):
        dv.resolve_props(trk, ("radius", ("radius", "Teff")))
    with pytest.raises(ValueError):
        dv.resolve_props(trk, ())
    assert dv.DERIVED_BUDGET_BYTES == 2 << 30
    assert ia.chain_derived is dv.chain_derived
    with pytest.raises(ValueError, match="float64 CUDA"):
        ia.chain_derived(np.zeros((2, 4, 8, 5)), trk, ("radius",))


def test_fit_entry_points_refuse_what_has_no_stored_chain():
    from isochrones_amd.catalog import fit_catalog, fit_stars_gpu, StarCatalog
    import pandas as pd
    trk = _track()
    cat = StarCatalog(pd.DataFrame({"J_mag": [10.0, 11.0], "J_mag_unc": [0.02, 0.02]}), bands=["J"])
    with pytest.raises(ValueError, match="fused"):
        fit_stars_gpu(cat, trk, np.arange(2), fused=False, derived=("radius",))
    with pytest.raises(ValueError, match="fused"):
        fit_catalog(cat, trk, fused=False, derived=True)
    with pytest.raises(ValueError, match="nested"):
        fit_catalog(cat, trk, method="nested", derived=("radius",))
    with pytest.raises(ValueError, match=r"\(label, column\)"):
        fit_catalog(cat, trk, derived=("mass",))


def test_release_drops_the_packed_tables():
    trk = _track()
    trk.__dict__["_derived_tables"] = {"x": 1}
    trk.release()
    assert "_derived_tables" not in trk.__dict__
