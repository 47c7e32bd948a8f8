"""iso_derived_chain_host (libiso_derived.so's plain C++ statement of the derived chain) through ctypes against the numpy
twin, on the shapes the GPU test uses; no GPU needed.  Values within 1e-12 (1 + |b|), NaN positions and nan_count
exactly; and bit for bit for every Q and every component-reuse pattern."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _cabi, _derived_cabi
from isochrones_amd.csrc.libraries import DERIVED as build_derived
from tests import _derived_twin as tw


@pytest.fixture(scope="module")
def lib():
    build_derived.build()
    return _derived_cabi.lib()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def call_host(lib, chain, layout, S, W, cols, axes, comps, ens_begin=0, n_out=None, ndim=None, Q=None, n0=None, n_comps=None):
    """-> (rc, out [T, C*Q, R], nan_count [n_out, C*Q]); out prefilled with -7, nan_count with -7."""
    n_out = S - ens_begin if n_out is None else n_out
    T = chain.shape[0]
    ndim = (chain.shape[1] if layout == tw.PARAM_MAJOR else chain.shape[2]) if ndim is None else ndim
    Qr = cols.shape[3]
    Cn = len(comps)
    table = _derived_cabi.IsoDerivedTable(cols.ctypes.data, axes[0].ctypes.data, axes[1].ctypes.data, axes[2].ctypes.data,
                                          cols.shape[0] if n0 is None else n0, cols.shape[1], cols.shape[2],
                                          Qr if Q is None else Q)
    carr = (C.c_int32 * (3 * Cn))(*[i for comp in comps for i in comp])
    out = np.full((T, Cn * Qr, max(n_out, 1) * W), -7.0)
    nan_count = np.full((max(n_out, 1), Cn * Qr), -7, dtype=np.int32)
    rc = lib.iso_derived_chain_host(C.byref(table), _vp(chain), layout, T, S, W, ndim, ens_begin, n_out, carr,
                                    Cn if n_comps is None else n_comps, _vp(out), _vp(nan_count), None)
    return rc, out, nan_count


@pytest.mark.parametrize("S,W,T", tw.SHAPES)
@pytest.mark.parametrize("Q", tw.QS)
@pytest.mark.parametrize("Cn", tw.CS)
def test_host_abi_matches_the_twin(lib, S, W, T, Q, Cn):
    kind = "track" if (Q + Cn) % 2 else "iso"
    cols, axes = tw.packed(kind, Q)
    x = np.array(tw.chain(kind, S, W, T))
    comps = tw.comps_for(Cn)
    want, want_nan = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
    rc, full, nan_count = call_host(lib, x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
    assert rc == 0, lib.iso_derived_last_error()
    assert tw.close(full, want)
    assert tw.same_bits(full, want)
    np.testing.assert_array_equal(nan_count, want_nan)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1))
    rc, got_r, nan_r = call_host(lib, rows, tw.ROW_MAJOR, S, W, cols, axes, comps)
    assert rc == 0, lib.iso_derived_last_error()
    np.testing.assert_array_equal(got_r.view(np.int64), full.view(np.int64))          # the layout changes no bit
    np.testing.assert_array_equal(nan_r, nan_count)
    # ensemble sub-ranges: bitwise the matching slice of the full output
    for b, n in {(0, S), (min(1, S - 1), min(2, S - min(1, S - 1))), (S - 1, 1)}:
        rc, sub, nan_sub = call_host(lib, x, tw.PARAM_MAJOR, S, W, cols, axes, comps, ens_begin=b, n_out=n)
        assert rc == 0, lib.iso_derived_last_error()
        np.testing.assert_array_equal(sub.view(np.int64), full[:, :, b * W:(b + n) * W].view(np.int64))
        np.testing.assert_array_equal(nan_sub, nan_count[b:b + n])
        tw_sub, tw_nan = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, axes, comps, ens_begin=b, n_ens_out=n)
        assert tw.close(sub, tw_sub)
        np.testing.assert_array_equal(nan_sub, tw_nan)


@pytest.mark.parametrize("S,W,T", [tw.EDGE_SHAPES[0], tw.EDGE_SHAPES[3]])
@pytest.mark.parametrize("Q", range(1, 9))
def test_host_abi_is_the_twin_bit_for_bit(lib, S, W, T, Q):
    """Every Q, every reuse pattern, both table kinds, on a two-chunk shape and on the 2 100-step one: the plain C++
    statement and the numpy one are the same float64 operations, so they agree in every bit, not within 1e-12."""
    for kind in ("track", "iso"):
        cols, axes = tw.packed(kind, Q)
        x = np.array(tw.chain7(kind, S, W, T))
        for comps in tw.COMP_PATTERNS:
            want, want_nan = tw.derive(x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
            rc, got, nan_count = call_host(lib, x, tw.PARAM_MAJOR, S, W, cols, axes, comps)
            assert rc == 0, lib.iso_derived_last_error()
            assert tw.close(got, want), (kind, comps)
            assert tw.same_bits(got, want), (kind, comps)
            np.testing.assert_array_equal(nan_count, want_nan)
            assert np.isfinite(want).mean() > 0.5 and np.isnan(want).mean() > 0.05


def test_rules_through_the_host_abi(lib):
    cols, axes = tw.rule_table()
    pts = np.array([(0.5, 15.0, 3.0), (1.0, 20.0, 2.0), (2.0, 15.0, 3.0), (0.5, 40.0, 3.0), (0.5, 15.0, 8.0), (-0.1, 15.0, 3.0),
                    (0.5, 15.0, 8.5), (np.nan, 15.0, 3.0), (1.0, 20.0, 4.0), (2.0, 40.0, 8.0)])
    x = np.ascontiguousarray(pts.T[None])                                      # [1, 3, 10]: one ensemble of 10 walkers
    rc, out, nan_count = call_host(lib, x, tw.PARAM_MAJOR, 1, 10, cols, axes, [(0, 1, 2)])
    assert rc == 0
    want = tw.interp(cols, axes, pts[:, 0], pts[:, 1], pts[:, 2])
    np.testing.assert_array_equal(out[0].T, want)
    np.testing.assert_array_equal(out[0, :, :5].T, [[56.5, 2.5], [111.0, 2.5], [206.5, 3.25], [71.5, 3.25], [58.0, 5.75]])
    np.testing.assert_array_equal(nan_count, [[5, 5]])
    # every query of the twin's rule test, with its exact numbers
    pts = np.array([q for q, _ in tw.RULES])
    x = np.ascontiguousarray(pts.T[None])
    rc, out, nan_count = call_host(lib, x, tw.PARAM_MAJOR, 1, len(pts), cols, axes, [(0, 1, 2)])
    assert rc == 0
    np.testing.assert_array_equal(out[0].T, [w for _, w in tw.RULES])


def test_bad_arguments_are_refused(lib):
    cols, axes = tw.packed("iso", 3)
    S, W, T = 3, 10, 7
    x = np.array(tw.chain("iso", S, W, T))
    one = [(2, 3, 0)]
    bad = (dict(Q=0), dict(Q=9), dict(comps=[(2, 3, 0)] * 4), dict(comps=[(2, 6, 0)]), dict(comps=[(-1, 3, 0)]),
           dict(ens_begin=2, n_out=2), dict(ens_begin=3, n_out=1), dict(ens_begin=0, n_out=0), dict(ens_begin=-1, n_out=1),
           dict(n0=1), dict(layout=2), dict(comps=one, n_comps=0))
    for kw in bad:
        kw = dict(kw)
        rc, out, nan_count = call_host(lib, x, kw.pop("layout", tw.PARAM_MAJOR), S, W, cols, axes, kw.pop("comps", one), **kw)
        assert rc == _derived_cabi.ERR_INVALID and lib.iso_derived_last_error(), kw
        assert (out == -7.0).all() and (nan_count == -7).all(), kw
    table = _derived_cabi.IsoDerivedTable(cols.ctypes.data, axes[0].ctypes.data, axes[1].ctypes.data, axes[2].ctypes.data,
                                          *cols.shape)
    carr = (C.c_int32 * 3)(2, 3, 0)
    out = np.zeros((T, 3, S * W))
    nc = np.zeros((S, 3), dtype=np.int32)
    args = [C.byref(table), _vp(x), 1, T, S, W, 6, 0, S, carr, 1, _vp(out), _vp(nc), None]
    assert lib.iso_derived_chain_host(*args) == 0
    for i in (0, 1, 9, 11, 12):                                                # table, chain, comps, out, nan_count
        a = list(args)
        a[i] = None
        assert lib.iso_derived_chain_host(*a) == _derived_cabi.ERR_INVALID
    a = list(args)
    a[3] = 0                                                                   # nsteps
    assert lib.iso_derived_chain_host(*a) == _derived_cabi.ERR_INVALID
    assert _cabi.CHAIN_PARAM_MAJOR == tw.PARAM_MAJOR and _cabi.CHAIN_ROW_MAJOR == tw.ROW_MAJOR
