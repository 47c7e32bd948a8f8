"""iso_predict_chain_host (plain C++, no device) against the numpy twin and the C oracle; no GPU needed.

The model-grid part of a sample is not an output of its own.  It is seen bit for bit in two ways: with a BC table of
zeros and every distance 10 pc the magnitude of a single star is Mbol + 0 - 0; and an ensemble of one sample has
term_chi2 = z, the float64 (obs - model)^2 / unc^2 of Teff, logg, feh and parallax, which the twin computes with the same
operations.  Magnitudes are held to 1e-9 of the oracle, term_chi2 and ppc to rtol 1e-9 of the long-double twin (the
kernel's tree of 128 float64 partials over at most a few hundred terms stays within a few 1e-16 of it)."""
import numpy as np
import pytest

from isochrones_amd import _predict_cabi as pc
from tests import _predict_twin as tw


def _case(kind, shape, B, Cn):
    S, W, T = shape
    x, lp = tw.chain(kind, S, W, T, Cn)
    comps, i_dist, i_AV = tw.comps_for(Cn)
    val, unc = tw.observations(kind, S, B)
    return tw.tables(kind, B), x, lp, S, W, comps, i_dist, i_AV, val, unc


@pytest.mark.parametrize("kind", ["track", "iso"])
def test_model_grid_part_is_the_twin_bit_for_bit(kind):
    cols, ax3, bc, ax4 = tw.tables(kind, 3)
    zero = np.zeros_like(bc)
    S, W, T = 40, 1, 1
    x, lp = tw.chain(kind, S, W, T, 1)
    x = x.copy()
    x[:, 3] = 10.0
    comps, i_dist, i_AV = tw.comps_for(1)
    val = np.tile(np.array([1.0, 2.0, 3.0, 5000.0, 4.0, 0.1, 90.0]), (S, 1))
    unc = np.tile(np.array([0.5, 0.5, 0.5, 70.0, 0.3, 0.2, 3.0]), (S, 1))
    tab = (cols, ax3, zero, ax4)
    got = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    mbol = want["model"][0, :, :, 3]                                            # [T, R]
    on_bc = ~np.isnan(want["mags"][:, 0])
    assert on_bc.sum() > 10
    assert tw.same_bits(got["mags"][:, 0][on_bc] + 0.0, mbol[on_bc] + 0.0)
    good = want["good"][0]
    assert good.sum() > 10 and (~good).sum() > 0
    assert tw.same_bits(got["term_chi2"][good], want["z"][0][good])             # one sample: the mean is z / 1
    np.testing.assert_array_equal(got["n_bad"], (~good).astype(np.int32))
    assert np.isnan(got["ppc"][~good]).all()


@pytest.mark.parametrize("kind", ["track", "iso"])
@pytest.mark.parametrize("B,Cn", [(1, 1), (3, 2), (8, 3), (9, 1), (9, 2)])
def test_host_entry_against_twin_and_oracle(kind, B, Cn, capsys):
    tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case(kind, (5, 26, 4), B, Cn)
    got = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    ok_m, dev_m = tw.mags_close(got["mags"], tw.oracle_mags(kind, x, comps, i_dist, i_AV, B))
    ok_t, dev_t = tw.rel_close(got["term_chi2"], want["term_chi2"])
    ok_p, dev_p = tw.rel_close(got["ppc"], want["ppc"])
    with capsys.disabled():
        print("\nhost, %s B=%d C=%d: mags %.2e, term_chi2 %.2e, ppc %.2e" % (kind, B, Cn, dev_m, dev_t, dev_p))
    assert ok_m and ok_t and ok_p
    np.testing.assert_array_equal(got["n_bad"], want["n_bad"])
    np.testing.assert_array_equal(got["map_index"], want["map_index"])
    np.testing.assert_array_equal(got["mag_nan"], want["mag_nan"])
    assert tw.same_bits(got["map_pars"], want["map_pars"])
    assert want["n_bad"].sum() > 0 and np.isfinite(want["ppc"]).any()


@pytest.mark.parametrize("B", tw.WIDE_BS)
def test_host_entry_with_three_and_four_band_chunks(B):
    for kind, Cn in (("track", 1), ("iso", 2)):
        tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case(kind, (3, 10, 7), B, Cn)
        got = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
        want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
        assert tw.mags_close(got["mags"], want["mags"])[0]
        assert tw.rel_close(got["term_chi2"], want["term_chi2"])[0] and tw.rel_close(got["ppc"], want["ppc"])[0]
        for k in ("n_bad", "map_index", "mag_nan"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        sel = list(range(9)) + list(range(B, B + 4))              # the first nine bands alone: the same bits, chunk by chunk
        nine = tw.host(tw.tables(kind, 9), x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV,
                       np.ascontiguousarray(val[:, sel]), np.ascontiguousarray(unc[:, sel]))
        assert tw.same_bits(got["mags"][:, :9], nine["mags"]) and tw.same_bits(got["term_chi2"][:, :9], nine["term_chi2"][:, :9])


def test_layouts_and_a_sub_range_give_the_same_bits():
    tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case("iso", (3, 10, 7), 3, 2)
    full = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1))
    rm = tw.host(tab, rows, lp, tw.ROW_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    sub = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc, ens_begin=1, n_out=2)
    for k in ("mags", "term_chi2", "ppc", "n_bad", "map_index", "map_pars", "mag_nan"):
        assert tw.same_bits(rm[k], full[k]), k
        assert tw.same_bits(sub[k], full[k][:, :, W:] if k == "mags" else full[k][1:]), k
    # a null lnprob writes no MAP; null outputs are skipped
    no = tw.host(tab, x, None, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc, want=("ppc", "map_index", "map_pars"))
    assert (no["map_index"] == -7).all() and (no["map_pars"] == -7).all() and (no["mags"] == -7).all()
    assert tw.same_bits(no["ppc"], full["ppc"])


def test_bad_arguments_are_refused_with_a_message():
    tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case("track", (3, 10, 7), 3, 1)
    cols, ax3, bc, ax4 = tab
    args = dict(tab=tab, x=x, lp=lp, layout=tw.PARAM_MAJOR, S=S, W=W, comps=comps, i_dist=i_dist, i_AV=i_AV, obs_val=val,
                obs_unc=unc)
    lib = pc.lib()

    def refused(**kw):
        rc = tw.host(**dict(args, **kw), rc_only=True)
        msg = lib.iso_predict_last_error().decode()
        assert rc == pc.ERR_INVALID and msg.startswith("iso_predict_chain_host: ") and len(msg) > 30, (kw, rc, msg)
        return msg

    assert tw.host(**args, rc_only=True) == 0
    assert "table" in refused(tab=(None, ax3, bc, ax4))
    assert "table" in refused(tab=(cols, ax3, None, ax4))
    wide = np.zeros(bc.shape[:4] + (33,))
    assert "B must" in refused(tab=(cols, ax3, wide, ax4), obs_val=np.zeros((S, 37)), obs_unc=np.ones((S, 37)))
    assert "B must" in refused(tab=(cols, ax3, np.zeros(bc.shape[:4] + (0,)), ax4))
    assert "C must" in refused(comps=[(1, 2, 0)] * 4)
    assert "component" in refused(comps=[(1, 2, 5)])
    assert "i_dist" in refused(i_dist=5)
    assert "i_dist" in refused(i_dist=-1)
    assert "i_AV" in refused(i_AV=5)
    assert "range" in refused(ens_begin=2, n_out=2)
    assert "range" in refused(ens_begin=0, n_out=0)
    assert "layout" in refused(layout=2)
