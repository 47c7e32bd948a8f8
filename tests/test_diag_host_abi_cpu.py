"""iso_diag_chain_host (libiso_diag.so's plain C++ statement of the chain diagnostics) through ctypes against the numpy
twin, on the shapes the GPU test uses; no GPU needed.  tau, ess and rhat within 1e-9 relative, window and window_ok
exactly.  Also the conditions the shared fixtures rest on: the tile size and LDS path each long shape was chosen for, and
the open window of the c = 1000 evaluations."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _cabi, _diag_cabi
from isochrones_amd.csrc.libraries import DIAG as build_diag
from tests import _diag_twin as tw


@pytest.fixture(scope="module")
def lib():
    build_diag.build()
    return _diag_cabi.lib()


def _call(lib, st, S, W, c=5.0, max_lag=1024, layout=_cabi.CHAIN_PARAM_MAJOR, D=None):
    D = st.shape[1] if D is None else D
    out = np.full((S, D, tw.NOUT), -7.0)
    rc = lib.iso_diag_chain_host(st.ctypes.data_as(C.c_void_p), layout, st.shape[0], S, W, D, c, max_lag,
                                 out.ctypes.data_as(C.c_void_p), None)
    return rc, out


@pytest.mark.parametrize("name", [sh[0] for sh in tw.SHAPES])
def test_host_abi_matches_the_twin(lib, name):
    st, (S, D, W, T, max_lag), want = tw.fixture(name)
    rc, got = _call(lib, np.ascontiguousarray(st), S, W, 5.0, max_lag)
    assert rc == 0, lib.iso_diag_last_error()
    tw.assert_matches(got, want)


@pytest.mark.parametrize("name", tw.LONG_SHAPES)
def test_every_lag_enters_tau(lib, name):
    """tau sums rho(1..M*) only, so at c = 5 a lag sum beyond the window is invisible.  With c = 1000 the slowest
    parameter's window stays open (open_window asserts window == K, window_ok == 0 on the twin) and all K lags count."""
    st, (S, D, W, T, max_lag), want = tw.open_window(name)
    rc, got = _call(lib, np.ascontiguousarray(st), S, W, tw.OPEN_C, max_lag)
    assert rc == 0, lib.iso_diag_last_error()
    tw.assert_matches(got, want)


def test_long_shapes_get_the_tiles_they_were_chosen_for():
    """The selection arithmetic of iso_diag_chain, replayed by tile_plan: an edit of a shape cannot silently stop reaching
    its branch of the kernel."""
    dims = {sh[0]: sh[1:] for sh in tw.SHAPES}
    assert set(tw.PLANS) == set(tw.LONG_SHAPES)
    for name, plan in tw.PLANS.items():
        S, D, W, T, max_lag = dims[name]
        assert tw.tile_plan(W, T, max_lag) == plan, name
    lanes = {}                                                   # name -> lags per lane (1..4) of every quad of 256 lags
    for name in tw.LONG_SHAPES:
        K1 = min(dims[name][3] - 1, dims[name][4]) + 1
        lanes[name] = [min(4, (K1 - 256 * q + 63) // 64) for q in range((K1 + 255) // 256)]
    assert lanes == {"two_quads": [4, 3], "uneven_tiles": [4, 2], "large_lds": [4, 4, 4, 4, 1], "max_lag_mid_lane": [4, 2],
                     "near_limit": [4, 4, 4, 4, 1]}
    # tiles that start at a walker index that is no multiple of 4, and a partial last tile after more than two tiles
    W, WT = dims["uneven_tiles"][2], tw.PLANS["uneven_tiles"][0]
    assert [min(WT, W - w0) for w0 in range(0, W, WT)] == [5, 5, 5, 5, 1]
    # max_lag binds inside a lane's lags: the lane's first lag is kept, a later one is summed and dropped
    for name, dropped in (("max_lag_mid_lane", range(36, 64)), ("uneven_tiles", range(11, 64))):
        K = dims[name][4]
        assert [l for l in range(64) if 256 + l <= K < 256 + 64 + l] == list(dropped), name
    # the library's two refusals, just past the shapes it takes
    with pytest.raises(ValueError, match="exceed a CU's 160 KB"):
        tw.tile_plan(1, 16400, 1024)
    with pytest.raises(ValueError, match="nsteps too large"):
        tw.tile_plan(2, 20481, 1024)
    # every earlier shape stays inside 64 KB
    assert not any(tw.tile_plan(W, T, ml)[2] for n, (S, D, W, T, ml) in dims.items() if n not in tw.PLANS)


def test_a_nan_or_an_infinity_anywhere_makes_the_row_nan(lib):
    st, (S, D, W, T, max_lag), want = tw.fixture("nonfinite")
    assert np.isposinf(st[:, 0]).sum() == 1 and np.isneginf(st[:, 1]).sum() == 1 and not np.isnan(st).any()
    assert np.isnan(want[0, :2]).all() and np.isfinite(want[0, 2]).all()
    rc, got = _call(lib, np.ascontiguousarray(st), S, W, 5.0, max_lag)
    assert rc == 0
    tw.assert_matches(got, want)
    clean = np.where(np.isfinite(st), st, 0.0)                           # the finite parameter does not see its neighbours
    rc, alone = _call(lib, np.ascontiguousarray(clean), S, W, 5.0, max_lag)
    assert rc == 0 and np.isfinite(alone).all()
    assert np.array_equal(got[0, 2].view(np.int64), alone[0, 2].view(np.int64))
    rows = np.ascontiguousarray(st.transpose(0, 2, 1))
    rc, got_rows = _call(lib, rows, S, W, 5.0, max_lag, layout=_cabi.CHAIN_ROW_MAJOR, D=D)
    assert rc == 0
    tw.assert_matches(got_rows, want)


def test_row_major_layout_and_python_surface(lib):
    import isochrones_amd as ia
    st, (S, D, W, T, max_lag), want = tw.fixture("plain")
    rows = np.ascontiguousarray(st.transpose(0, 2, 1))                   # [T, S * W, D]
    rc, got = _call(lib, rows, S, W, 5.0, max_lag, layout=_cabi.CHAIN_ROW_MAJOR, D=D)
    assert rc == 0
    tw.assert_matches(got, want)
    chain = st.reshape(T, D, S, W).transpose(2, 3, 0, 1)                 # the [S, W, T, D] view sampler.chain returns
    r = ia.chain_diagnostics(chain)
    assert r.tau.shape == (S, D)
    tw.assert_matches(np.stack(r, axis=-1), want)
    one = ia.chain_diagnostics(chain[1])                                 # [W, T, D]: a single model's chain
    assert one.rhat.shape == (D,)
    tw.assert_matches(np.stack(one, axis=-1), want[1])
    r2 = ia.chain_diagnostics(np.array(st), n_ens=S, nwalkers=W)         # the storage itself, with its sizes
    assert np.array_equal(np.stack(r2, axis=-1), np.stack(r, axis=-1), equal_nan=True)


def test_other_window_factor_and_max_lag(lib):
    st, (S, D, W, T, _), _ = tw.fixture("reference")
    sub = np.ascontiguousarray(st[:, :2, :W])
    margins = []
    want = tw.storage_diagnostics(sub, 1, W, 3.0, 7, margins)
    tw.check_fixture(want, T, margins)
    rc, got = _call(lib, sub, 1, W, 3.0, 7)
    assert rc == 0
    tw.assert_matches(got, want)


def test_bad_arguments_are_refused(lib):
    st = np.zeros((8, 2, 12))
    for kw in (dict(c=0.0), dict(c=-1.0), dict(c=float("nan")), dict(c=float("inf")), dict(max_lag=0), dict(layout=2)):
        rc, out = _call(lib, st, 3, 4, **kw)
        assert rc == -1 and lib.iso_diag_last_error(), kw      # ISO_DIAG_ERR_INVALID
        assert (out == -7.0).all()
    assert lib.iso_diag_chain_host(None, 1, 8, 3, 4, 2, 5.0, 1024, st.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.iso_diag_chain_host(st.ctypes.data_as(C.c_void_p), 1, 0, 3, 4, 2, 5.0, 1024, st.ctypes.data_as(C.c_void_p), None) == -1
    import isochrones_amd as ia
    with pytest.raises(ValueError):
        ia.chain_diagnostics(np.zeros((2, 4, 8, 2)), max_lag=0)
    with pytest.raises(ValueError):
        ia.chain_diagnostics(np.zeros((2, 4, 8, 2)), c=0.0)
    with pytest.raises(ValueError):
        ia.chain_diagnostics(np.zeros((8, 2, 12)), n_ens=3)


def test_result_columns_switch():
    from isochrones_amd.catalog import result_columns
    names = ("mass", "eep", "feh", "distance", "AV")
    base = result_columns(names)
    assert result_columns(names, diagnostics=False) == base and base[-3:] == ["lnpost_max", "acceptance", "ok"]
    cols = result_columns(names, diagnostics=True)
    assert cols[:17] == base[:17] and cols[-1] == "ok" and len(cols) == 2 * len(base)
    assert cols[17:20] == ["mass_tau", "mass_ess", "mass_rhat"] and cols[-4:-1] == ["tau_max", "rhat_max", "window_ok"]
