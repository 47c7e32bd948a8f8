"""iso_population_eval_host against the numpy twin of include/isochrones_amd_population.h: model columns bit for bit,
magnitudes and extinctions within 1e-9 (log10 and pow come from two math libraries) with identical NaN patterns, every
argument error with its message, null outputs skipped, N = 0 a no-op."""
import ctypes as C

import numpy as np
import pytest

from tests import _population_twin as tw


@pytest.mark.parametrize("Cn", (1, 2))
@pytest.mark.parametrize("Q,B", [(4, 1), (5, 3), (8, 7), (9, 3), (18, 7)] + list(tw.WIDE))
def test_host_entry_equals_the_twin(Q, B, Cn):
    tab = tw.tables(Q, B)
    x, d, a = tw.inputs(257, Cn)
    got, want = tw.host(tab, x, d, a), tw.evaluate(tab, x, d, a)
    tw.assert_same(got, want, "Q=%d B=%d C=%d" % (Q, B, Cn))
    assert np.isnan(want["sys_mag"]).any() and np.isfinite(want["sys_mag"]).all(axis=0).sum() > 100


def test_the_edge_rows_do_what_they_are_there_for():
    tab = tw.tables()
    edges = tw.edge_rows(tab)
    n = len(edges)
    assert n < 257
    x, d, a = tw.inputs(257, 2)
    w = tw.evaluate(tab, x, d, a)
    # an absent secondary leaves the primary's light, the extinction included
    assert np.isnan(w["mag_out"][1, :, 1]).all() and np.array_equal(w["cols_out"][0, :, 1], w["cols_out"][0, :, 0])
    ok, dev = tw.close(w["sys_mag"][:, 1], w["mag_out"][0, :, 1])
    assert ok and np.isfinite(w["sys_mag"][:, 1]).all(), dev
    ok, dev = tw.close(w["sys_A"][:, 1], w["A_out"][0, :, 1])
    assert ok, dev
    # the poked nodes: on an end of a BC axis the magnitudes are finite, one ulp outside they are NaN
    first = 2 + 2 * 15
    for k, (h, which) in enumerate(tw._POKES):
        row = first + 2 * k
        hot = tab[2][h]
        assert w["cols_out"][0, hot, row] == tw._poke_value(tab[4][h], which)
        assert np.isfinite(w["mag_out"][0, :, row]).all() == (which in ("first", "last")), (h, which)
        assert np.isfinite(w["mag_out"][1, :, row + 1]).all() == (which in ("first", "last")), (h, which)
        assert np.isfinite(w["sys_mag"][:, row + 1]).all()                   # the secondary off the BC grid: the primary's
    # AV = 0: no extinction; a NaN primary gives NaN; Teff beyond the BC table: model columns but no magnitude
    av0 = first + 2 * len(tw._POKES)
    assert a[av0] == 0.0 and np.array_equal(w["A_out"][:, :, av0], np.zeros((2, 7)))
    assert a[av0 + 1] == tab[4][3][-1] and np.isfinite(w["sys_A"][:, av0 + 1]).all()
    assert np.isnan(w["mag_out"][:, :, av0 + 2]).all() and np.isnan(w["mag_out"][:, :, av0 + 3]).all()
    assert np.isnan(w["sys_mag"][:, 2 + 2 * 4]).all()                        # ax0 of the primary NaN
    hotrow = n - 2
    assert np.isfinite(w["cols_out"][0, :, hotrow]).all() and np.isnan(w["mag_out"][0, :, hotrow]).all()
    assert w["cols_out"][0, tab[2][0], hotrow] > tab[4][0][-1]


def test_null_outputs_are_skipped_and_n_zero_writes_nothing():
    tab = tw.tables(9, 3)
    x, d, a = tw.inputs(65, 2)
    full = tw.host(tab, x, d, a)
    for want in (("sys_mag",), ("cols_out", "A_out"), ("mag_out", "sys_A"), ()):
        got = tw.host(tab, x, d, a, want=want)
        for k in tw.OUTPUTS:
            if k in want:
                assert tw.same_bits(got[k], full[k]), (want, k)
            else:
                assert (got[k] == tw.SENTINEL).all(), (want, k)
    none = tw.host(tab, x, d, a, N=0)
    assert all((none[k] == tw.SENTINEL).all() for k in tw.OUTPUTS)


def test_a_system_does_not_depend_on_its_batch():
    tab = tw.tables(18, 7)
    x, d, a = tw.inputs(257, 2)
    full = tw.host(tab, x, d, a)
    for i in (0, 1, 40, 128, 256):
        one = tw.host(tab, np.ascontiguousarray(x[:, :, i:i + 1]), d[i:i + 1].copy(), a[i:i + 1].copy())
        for k in tw.OUTPUTS:
            assert tw.same_bits(one[k][..., 0], full[k][..., i]), (i, k)


def _rc(tab, x, d, a, **kw):
    from isochrones_amd import _population_cabi as pc
    rc = tw.host(tab, x, d, a, rc_only=True, **kw)
    return rc, pc.lib().iso_population_last_error().decode()


def test_argument_errors():
    from isochrones_amd import _population_cabi as pc
    cols, ax3, hot, bc, ax4 = tab = tw.tables(8, 3)
    x, d, a = tw.inputs(2, 2)
    assert _rc(tab, x, d, a) == (0, "")
    cases = [
        ((None, ax3, hot, bc, ax4), {}, "null model table pointer"),
        ((cols, (ax3[0], None, ax3[2]), hot, bc, ax4), {}, "null model table pointer"),
        ((cols, ax3, hot, None, ax4), {}, "null BC table pointer"),
        ((cols, ax3, hot, bc, ax4[:3] + (None,)), {}, "null BC table pointer"),
        ((cols[..., :3], ax3, (0, 1, 2, 2), bc, ax4), {}, "Q must be 4 to 32 columns"),
        ((cols, ax3, (0, 1, 8, 3), bc, ax4), {}, "a hot column index is outside [0, Q)"),
        ((cols, ax3, (0, -1, 2, 3), bc, ax4), {}, "a hot column index is outside [0, Q)"),
        ((cols, ax3, hot, bc[..., :0], ax4), {}, "B must be 1 to 32 bands"),
        (tab, dict(Cn=0), "C must be 1 or 2 components"),
        (tab, dict(Cn=3), "C must be 1 or 2 components"),
        (tab, dict(N=-1), "N must not be negative"),
        ((cols[:1], ax3, hot, bc, ax4), {}, "every model axis needs at least 2 nodes"),
        ((cols, ax3, hot, bc[:, :, :, :1], ax4), {}, "every BC axis needs at least 2 nodes"),
    ]
    for bad, kw, msg in cases:
        bad = tuple(np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t for t in bad)
        if bad[0] is None or bad[3] is None:                    # the shapes a null table cannot give
            p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
            mt = pc.IsoPopulationModelTable(p(bad[0]), p(ax3[0]), p(ax3[1]), p(ax3[2]), 5, 10, 48, 8, (C.c_int32 * 4)(*hot))
            bt = pc.IsoPopulationBcTable(p(bad[3]), *[p(v) for v in ax4], 5, 5, 6, 4, 3, 0)
            o = np.zeros(2 * 8 * 2)
            out = pc.IsoPopulationOut(o.ctypes.data, None, None, None, None)
            rc = pc.lib().iso_population_eval_host(C.byref(mt), C.byref(bt), x.ctypes.data, d.ctypes.data, a.ctypes.data, 2, 2,
                                                   C.byref(out), None)
            err = pc.lib().iso_population_last_error().decode()
        else:
            rc, err = _rc(bad, x, d, a, **kw)
        assert rc == pc.ERR_INVALID and err == "iso_population_eval_host: " + msg, (msg, rc, err)
    # null inputs and a null output struct
    mt, bt = tw.structs(pc, lambda v: v.ctypes.data, tab)
    out = pc.IsoPopulationOut(None, None, None, None, None)
    L = pc.lib()
    for args in ((None, d.ctypes.data, a.ctypes.data, C.byref(out)), (x.ctypes.data, None, a.ctypes.data, C.byref(out)),
                 (x.ctypes.data, d.ctypes.data, None, C.byref(out)), (x.ctypes.data, d.ctypes.data, a.ctypes.data, None)):
        assert L.iso_population_eval_host(C.byref(mt), C.byref(bt), args[0], args[1], args[2], 2, 2, args[3], None) == pc.ERR_INVALID
        assert L.iso_population_last_error().decode() == "iso_population_eval_host: null pointer"
    with pytest.raises(pc.IsoError) as e:
        pc.check(L.iso_population_eval_host(None, C.byref(bt), x.ctypes.data, d.ctypes.data, a.ctypes.data, 2, 2, C.byref(out), None))
    assert e.value.rc == pc.ERR_INVALID and "null model table pointer" in str(e.value)
    assert L.iso_population_eval_host(C.byref(mt), C.byref(bt), x.ctypes.data, d.ctypes.data, a.ctypes.data, 2 ** 31, 2,
                                      C.byref(out), None) == pc.ERR_INVALID
