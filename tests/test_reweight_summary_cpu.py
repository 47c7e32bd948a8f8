"""iso_reweight_summary_host (the weighted summaries of weights the caller supplies, libiso_reweight.so) through ctypes, no
GPU needed: fed the weights iso_reweight_stars_host wrote, it returns that call's mean, sd, quant and n_nan bit for bit,
for 1 and 8 value columns, 1 and 8 probabilities, masked stars, a sub-range of stars and NaN values; its refusals."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _hier_cabi as hc, _reweight_cabi as rc
from isochrones_amd.csrc.libraries import HIER, REWEIGHT
from tests import _reweight_twin as rt

PROBS8 = (0.025, 0.16, 0.25, 0.5, 0.75, 0.84, 0.975, 0.999)


@pytest.fixture(scope="module")
def lib():
    HIER.build()
    REWEIGHT.build()
    return rc.lib()


def _summary(lib, case, weights, ens_begin=0, n_ens_out=None, **over):
    """iso_reweight_summary_host of the case's value columns, placed as tests/_reweight_twin.call places them, under
    ``weights`` [S, M] (the rows of the call's stars are passed).  The fill value is -7."""
    S, W, T = case["S"], case["W"], case["T"]
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    probs = np.ascontiguousarray(over.get("probs", case["probs"]), dtype=np.float64)
    V, K = over.get("V", len(case["values"])), over.get("K", probs.size)
    storages = list(case["storages"]) + [rt._value_storage(case, 0, S)]
    vals = (hc.IsoHierColumn * max(len(case["values"]), 1))()
    for i, (kind, j) in enumerate(case["values"]):
        if kind == "x":
            k, ncols, col = case["where"][j]
            vals[i] = hc.IsoHierColumn(storages[k].ctypes.data, ncols, col, S, 0)
        else:
            vals[i] = hc.IsoHierColumn(storages[-1].ctypes.data, case["y"].shape[0] + 1, j + 1, S, 0)
    nv, nk = len(case["values"]), probs.size
    out = dict(mean=np.full((S, nv), -7.0), sd=np.full((S, nv), -7.0), quant=np.full((S, nv, nk), -7.0),
               n_nan=np.full((S, nv), -7, np.int32))
    u = np.ascontiguousarray(weights[ens_begin:ens_begin + max(n_ens_out, 1)])
    ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)
    code = lib.iso_reweight_summary_host(vals, V, over.get("layout", case["layout"]), over.get("T", T), S, W, ens_begin, n_ens_out,
                                         ptr(case["mask"]), probs.ctypes.data_as(C.POINTER(C.c_double)), K,
                                         ptr(None if over.get("no_weights") else u), ptr(out["mean"]), ptr(out["sd"]),
                                         ptr(out["quant"]), ptr(out["n_nan"]), None)
    return code, out


def _same(got, want, stars=slice(None)):
    for k in ("mean", "sd", "quant", "n_nan"):
        assert got[k][stars].tobytes() == want[k][stars].tobytes(), k


@pytest.mark.parametrize("V, probs", [(1, (0.5,)), (8, (0.5,)), (1, PROBS8), (8, PROBS8), (3, rt.PROBS3)])
def test_the_summaries_of_the_stars_call_bit_for_bit(lib, V, probs):
    case = rt.random_case(4, 7, 37, 2, 5, V, seed=20 + V + len(probs), probs=probs)
    code, want = rt.call(lib, case)
    assert code == 0 and np.isfinite(want["mean"]).all() and (want["wsum"] > 0).all()
    code, got = _summary(lib, case, want["weights"])
    assert code == 0, lib.iso_reweight_last_error()
    _same(got, want)
    # a sub-range writes its stars and leaves the rest alone
    code, part = _summary(lib, case, want["weights"], ens_begin=1, n_ens_out=2)
    assert code == 0
    _same(part, want, slice(1, 3))
    assert (part["mean"][[0, 3]] == -7.0).all() and (part["n_nan"][[0, 3]] == -7).all() and (part["quant"][[0, 3]] == -7.0).all()


@pytest.mark.parametrize("name", ["one_dead_row", "all_dead_rows", "bad_and_nan", "masked"])
def test_special_cases_bit_for_bit(lib, name):
    case = rt.special_cases()[name]
    code, want = rt.call(lib, case)
    assert code == 0
    weights = want["weights"].copy()
    if case["mask"] is not None:
        weights[np.asarray(case["mask"]) == 0] = np.nan             # a masked star's weights are not read
    code, got = _summary(lib, case, weights)
    assert code == 0, lib.iso_reweight_last_error()
    _same(got, want)
    assert np.isnan(got["mean"]).any() or name == "one_dead_row"


def test_row_major_layout(lib):
    from isochrones_amd import _cabi
    case = rt.random_case(3, 5, 11, 2, 3, 4, seed=5, layout=_cabi.CHAIN_ROW_MAJOR)
    code, want = rt.call(lib, case)
    assert code == 0
    code, got = _summary(lib, case, want["weights"])
    assert code == 0
    _same(got, want)


def test_refusals(lib):
    case = rt.random_case(2, 3, 4, 1, 1, 2, seed=1)
    code, want = rt.call(lib, case)
    assert code == 0
    err = lambda: lib.iso_reweight_last_error().decode()
    for over, message in ((dict(V=0), "V must be 1 to 8"), (dict(V=9), "V must be 1 to 8"), (dict(K=0), "K must be 1 to 8"),
                          (dict(K=9), "K must be 1 to 8"), (dict(layout=7), "unknown chain layout"), (dict(T=0), "at least 1"),
                          (dict(probs=(0.5, 1.0, 0.2)), "outside (0, 1)"), (dict(no_weights=True), "null pointer")):
        code, got = _summary(lib, case, want["weights"], **over)
        assert code == rc.ERR_INVALID and message in err(), (over, err())
        assert err().startswith("iso_reweight_summary_host: ") and (got["mean"] == -7.0).all()
    for kw in (dict(ens_begin=2, n_ens_out=1), dict(ens_begin=0, n_ens_out=0)):
        assert _summary(lib, case, want["weights"], **kw)[0] == rc.ERR_INVALID and "ensemble range" in err()
