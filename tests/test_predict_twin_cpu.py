"""The numpy twin of include/isochrones_amd_predict.h against the C oracle (``OracleIC.interp_mag`` per component plus the
addmags formula) on small synthetic track and isochrone tables with 3 bands; no GPU needed.

Tolerance: the project's 1e-9, |a - b| <= 1e-9 (1 + |b|), NaN positions identical.  Twin and oracle run the same float64
operations; they can differ in the last bits of log10 and pow (numpy's against libm's)."""
import numpy as np
import pytest

from tests import _predict_twin as tw


@pytest.mark.parametrize("kind", ["track", "iso"])
@pytest.mark.parametrize("Cn", [1, 2, 3])
def test_twin_magnitudes_match_the_oracle(kind, Cn, capsys):
    S, W, T = 5, 26, 4
    B = 3
    x, lp = tw.chain(kind, S, W, T, Cn)
    comps, i_dist, i_AV = tw.comps_for(Cn)
    val, unc = tw.observations(kind, S, B)
    got = tw.predict(tw.tables(kind, B), x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    want = tw.oracle_mags(kind, x, comps, i_dist, i_AV, B)
    ok, dev = tw.mags_close(got["mags"], want)
    with capsys.disabled():
        print("\ntwin against the oracle, %s, C = %d: largest deviation %.2e" % (kind, Cn, dev))
    assert ok
    assert np.isfinite(want).mean() > 0.3 and np.isnan(want).mean() > 0.02       # inside the tables and off them


def test_twin_means_maps_ranges_and_layouts():
    kind, (S, W, T), B, Cn = "iso", (3, 10, 7), 3, 2
    x, lp = tw.chain(kind, S, W, T, Cn)
    comps, i_dist, i_AV = tw.comps_for(Cn)
    val, unc = tw.observations(kind, S, B)
    tab = tw.tables(kind, B)
    full = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    assert full["n_bad"].sum() > 0 and np.isfinite(full["ppc"]).all()
    e = 1
    z, good = full["z"][:, e * W:(e + 1) * W], full["good"][:, e * W:(e + 1) * W]
    present = ~np.isnan(val[e])
    np.testing.assert_allclose(full["term_chi2"][e, present], z[good][:, present].mean(axis=0), rtol=1e-12)
    assert np.isnan(full["term_chi2"][e, ~present]).all()
    np.testing.assert_allclose(full["ppc"][e], full["term_chi2"][e, present].sum() / present.sum(), rtol=1e-12)
    s = int(full["map_index"][e])
    assert lp[s // W, e * W + s % W] == np.nanmax(lp[:, e * W:(e + 1) * W])
    np.testing.assert_array_equal(full["map_pars"][e], x[s // W, :, e * W + s % W])
    rows = np.ascontiguousarray(x.transpose(0, 2, 1))
    other = tw.predict(tab, rows, lp, tw.ROW_MAJOR, S, W, comps, i_dist, i_AV, val, unc, ens_begin=1, n_ens_out=2)
    for k in ("term_chi2", "ppc", "n_bad", "map_index", "map_pars"):
        assert tw.same_bits(other[k], full[k][1:]), k
    assert tw.same_bits(other["mags"], full["mags"][:, :, W:])
