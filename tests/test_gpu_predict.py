"""iso_predict_chain on the GPU against iso_predict_chain_host, the numpy twin and the C oracle; bit identity of a star's
outputs alone, in a batch, in a range and from either layout; more stars than the grid has workgroups; edge cases the twin
alone fixes; the Python surface.

Tolerances (the issue's): magnitudes within 1e-9 (1 + |b|) of the oracle, term_chi2 and ppc within rtol 1e-9 of the
long-double twin, n_bad / map_index / map_pars exact."""
import numpy as np
import pytest

from tests import _predict_twin as tw

pytestmark = pytest.mark.gpu


def _case(kind, shape, B, Cn):
    S, W, T = shape
    x, lp = tw.chain(kind, S, W, T, Cn)
    comps, i_dist, i_AV = tw.comps_for(Cn)
    val, unc = tw.observations(kind, S, B)
    return tw.tables(kind, B), x, lp, S, W, comps, i_dist, i_AV, val, unc


@pytest.mark.parametrize("kind", ["track", "iso"])
@pytest.mark.parametrize("shape", tw.SHAPES)
def test_kernel_against_host_twin_and_oracle(kind, shape, capsys):
    worst = dict(mags=0.0, term=0.0, ppc=0.0)
    for B in (1, 3, 8, 9):
        for Cn in (1, 2, 3):
            tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case(kind, shape, B, Cn)
            got = tw.device(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
            hst = tw.host(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
            want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
            ok_m, dm = tw.mags_close(got["mags"], tw.oracle_mags(kind, x, comps, i_dist, i_AV, B))
            ok_h, _ = tw.mags_close(got["mags"], hst["mags"])
            ok_t, dt = tw.rel_close(got["term_chi2"], want["term_chi2"])
            ok_p, dp = tw.rel_close(got["ppc"], want["ppc"])
            worst = dict(mags=max(worst["mags"], dm), term=max(worst["term"], dt), ppc=max(worst["ppc"], dp))
            assert ok_m and ok_h and ok_t and ok_p, (B, Cn, dm, dt, dp)
            for k in ("n_bad", "map_index", "mag_nan"):
                np.testing.assert_array_equal(got[k], want[k], err_msg="%s B=%d C=%d" % (k, B, Cn))
                np.testing.assert_array_equal(got[k], hst[k])
            assert tw.same_bits(got["map_pars"], want["map_pars"])
    with capsys.disabled():
        print("\nkernel %s %s: largest deviation mags %.2e (oracle), term_chi2 %.2e, ppc %.2e (long-double twin)"
              % (kind, shape, worst["mags"], worst["term"], worst["ppc"]))


@pytest.mark.parametrize("B", tw.WIDE_BS)
def test_three_and_four_band_chunks_and_the_large_lds_launch(B, capsys):
    """17, 19 and 32 bands: three and four chunks of 8, a last chunk of one band, and (from 19 bands on) the launch that has
    to raise the kernel's dynamic LDS limit.  The same tolerances; the table's bands beyond nine are shifted copies."""
    for kind, Cn in (("track", 1), ("iso", 2)):
        tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case(kind, (3, 10, 7), B, Cn)
        got = tw.device(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
        want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
        ok_m, dm = tw.mags_close(got["mags"], want["mags"])
        ok_t, dt = tw.rel_close(got["term_chi2"], want["term_chi2"])
        ok_p, dp = tw.rel_close(got["ppc"], want["ppc"])
        with capsys.disabled():
            print("\nkernel %s B=%d C=%d: mags %.2e, term_chi2 %.2e, ppc %.2e" % (kind, B, Cn, dm, dt, dp))
        assert ok_m and ok_t and ok_p
        for k in ("n_bad", "map_index", "mag_nan"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert tw.same_bits(got["map_pars"], want["map_pars"])


@pytest.mark.parametrize("shape", [(3, 10, 7), (5, 26, 4)])
def test_a_star_has_the_same_bits_alone_in_a_batch_in_a_range_and_from_either_layout(shape):
    tab, x, lp, S, W, comps, i_dist, i_AV, val, unc = _case("iso", shape, 9, 2)
    full = tw.device(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1))
    rm = tw.device(tab, rows, lp, tw.ROW_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    e = S - 2
    rng = tw.device(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc, ens_begin=e, n_out=2)
    sl = slice(e * W, (e + 1) * W)
    alone = tw.device(tab, np.ascontiguousarray(x[:, :, sl]), np.ascontiguousarray(lp[:, sl]), tw.PARAM_MAJOR, 1, W, comps,
                      i_dist, i_AV, val[e:e + 1], unc[e:e + 1])
    for k in ("mags", "term_chi2", "ppc", "n_bad", "map_index", "map_pars", "mag_nan"):
        assert tw.same_bits(rm[k], full[k]), k
        one = full[k][:, :, sl] if k == "mags" else full[k][e:e + 1]
        assert tw.same_bits(rng[k][:, :, :W] if k == "mags" else rng[k][:1], one), k
        assert tw.same_bits(alone[k], one), k


def _check_against_host(got, hst, what):
    """every output of every star against the host entry, and no fill value left where the kernel has to write"""
    for k in got:
        assert not (got[k] == -7).any(), (what, k)
    assert tw.mags_close(got["mags"], hst["mags"])[0], what
    for k in ("term_chi2", "ppc"):
        ok, dev_ = tw.rel_close(got[k], hst[k])
        assert ok, (what, k, dev_)
    for k in ("n_bad", "map_index", "mag_nan"):
        np.testing.assert_array_equal(got[k], hst[k], err_msg="%s %s" % (what, k))
    assert tw.same_bits(got["map_pars"], hst["map_pars"]), what


def test_a_workgroup_takes_a_second_and_a_third_star():
    """S = 2 * ISO_PREDICT_MAX_BLOCKS + 1 stars of six samples (fewer than lanes): workgroup 0 takes the stars 0, 2 048 and
    4 096 in turn and reuses its LDS (the partial sums, the sample in flight, the bad and the NaN counts, the MAP tree).  What
    the first star leaves there would show in the second, the second's in the third: star 0 has every sample bad (n_bad = n,
    every mag_nan count full), star 2 048 is clean, star 4 096 lacks observations in some bands and has no finite lnprob
    (map_index = -1).  Then the same storage extended by five stars, read from star 3 on: the stars 3, 2 051 and 4 099
    carry the same three states."""
    from isochrones_amd import _predict_cabi as pc
    kind, B, Cn, W, T = "iso", 9, 2, 2, 3
    S = 2 * pc.MAX_BLOCKS + 1
    assert pc.MAX_BLOCKS == 2048 and W * T < pc.LANES
    tab = tw.tables(kind, B)
    _, ax3, _, _ = tab
    comps, i_dist, i_AV = tw.comps_for(Cn)
    x, lp = (v.copy() for v in tw.chain(kind, S + 5, W, T, Cn))
    val, unc = tw.observations(kind, S + 5, B)
    rng = np.random.default_rng(3)
    bad, clean, holes = (0, 3), (pc.MAX_BLOCKS, pc.MAX_BLOCKS + 3), (2 * pc.MAX_BLOCKS, 2 * pc.MAX_BLOCKS + 3)
    for s in bad + clean + holes:
        sl = slice(s * W, (s + 1) * W)
        x[:, 0:Cn, sl] = rng.uniform(250.0, 400.0, (T, Cn, W))                 # on both grids to begin with
        x[:, Cn, sl] = 0.5 * (ax3[0][0] + ax3[0][-1]) + rng.uniform(-0.05, 0.05, (T, W))
        x[:, Cn + 1, sl] = 0.5 * (ax3[1][0] + ax3[1][-1]) + rng.uniform(-0.05, 0.05, (T, W))
        x[:, i_dist, sl] = rng.uniform(150.0, 250.0, (T, W))
        x[:, i_AV, sl] = rng.uniform(0.1, 0.3, (T, W))
        val[s] = np.where(np.isnan(val[s]), 9.0, val[s])
    for s in bad:
        x[:, i_dist, s * W:(s + 1) * W] = np.nan
    for s in holes:
        val[s, [1, 4, B - 1, B + 2]] = np.nan
        lp[:, s * W:(s + 1) * W] = np.nan
    first = np.ascontiguousarray(x[:, :, :S * W]), np.ascontiguousarray(lp[:, :S * W])
    got = tw.device(tab, first[0], first[1], tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val[:S], unc[:S])
    hst = tw.host(tab, first[0], first[1], tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val[:S], unc[:S])
    _check_against_host(got, hst, "S = %d" % S)
    n = W * T
    assert got["n_bad"][bad[0]] == n and (got["mag_nan"][bad[0]] == n).all() and np.isnan(got["ppc"][bad[0]])
    assert got["n_bad"][clean[0]] == 0 and (got["mag_nan"][clean[0]] == 0).all() and np.isfinite(got["ppc"][clean[0]])
    assert np.isfinite(got["term_chi2"][clean[0]]).all() and 0 <= got["map_index"][clean[0]] < n
    assert got["map_index"][holes[0]] == -1 and np.isnan(got["map_pars"][holes[0]]).all() and got["n_bad"][holes[0]] == 0
    assert np.array_equal(np.isnan(got["term_chi2"][holes[0]]), np.isnan(val[holes[0]])) and np.isfinite(got["ppc"][holes[0]])
    # the stars around every change of star of workgroup 0, against the long-double twin
    stars = np.array([0, 1, pc.MAX_BLOCKS - 1, pc.MAX_BLOCKS, pc.MAX_BLOCKS + 1, 2 * pc.MAX_BLOCKS - 1, 2 * pc.MAX_BLOCKS])
    cols = (stars[:, None] * W + np.arange(W)).ravel()
    want = tw.predict(tab, np.ascontiguousarray(x[:, :, cols]), np.ascontiguousarray(lp[:, cols]), tw.PARAM_MAJOR, len(stars), W,
                      comps, i_dist, i_AV, val[stars], unc[stars])
    assert tw.mags_close(got["mags"][:, :, cols], want["mags"])[0]
    for k in ("term_chi2", "ppc"):
        ok, dev_ = tw.rel_close(got[k][stars], want[k])
        assert ok, (k, dev_)
    for k in ("n_bad", "map_index", "mag_nan"):
        np.testing.assert_array_equal(got[k][stars], want[k], err_msg=k)
    assert tw.same_bits(got["map_pars"][stars], want["map_pars"])
    # n_ens = S + 5, ens_begin = 3, n_ens_out = S
    rng_ = tw.device(tab, x, lp, tw.PARAM_MAJOR, S + 5, W, comps, i_dist, i_AV, val, unc, ens_begin=3, n_out=S)
    hst = tw.host(tab, x, lp, tw.PARAM_MAJOR, S + 5, W, comps, i_dist, i_AV, val, unc, ens_begin=3, n_out=S)
    _check_against_host(rng_, hst, "S = %d from star 3" % S)
    assert rng_["n_bad"][0] == n and rng_["n_bad"][pc.MAX_BLOCKS] == 0 and rng_["map_index"][2 * pc.MAX_BLOCKS] == -1
    for k in ("term_chi2", "ppc", "n_bad", "map_index", "map_pars", "mag_nan"):     # a star's bits do not depend on its workgroup
        assert tw.same_bits(rng_[k][:S - 3], got[k][3:]), k
    assert tw.same_bits(rng_["mags"][:, :, :(S - 3) * W], got["mags"][:, :, 3 * W:])


def test_edge_cases_fixed_by_the_twin():
    kind, B, Cn, S, W, T = "track", 3, 1, 6, 10, 7
    cols, ax3, bc, ax4 = tab = tw.tables(kind, B)
    comps, i_dist, i_AV = tw.comps_for(Cn)
    rng = np.random.default_rng(5)
    x = np.empty((T, 5, S * W))
    x[:, 0] = rng.uniform(300.0, 400.0, (T, S * W))                            # eep
    x[:, 1] = rng.uniform(-0.4, 0.2, (T, S * W))                               # feh (axis 0)
    x[:, 2] = rng.uniform(0.9, 1.2, (T, S * W))                                # mass (axis 1)
    x[:, 3] = rng.uniform(100.0, 300.0, (T, S * W))
    x[:, 4] = rng.uniform(0.0, 0.5, (T, S * W))
    base = tw.predict(tab, x, None, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, np.zeros((S, 7)), np.ones((S, 7)))
    assert base["n_bad"].sum() == 0                                            # every sample is on both grids to begin with
    x[3, 2, 1 * W + 4] = ax3[1][-1] + 1.0                                      # star 1: exactly one sample off the grid
    x[:, 0, 2 * W:3 * W] = ax3[2][-1] + 5.0                                    # star 2: every sample off the grid
    x[0, 4, 4 * W] = ax4[3][-1]                                                # star 4: AV on the last BC node ...
    val, unc = tw.observations(kind, S, B, seed=3)
    val[:] = np.where(np.isnan(val), 9.0, val)
    val[0, 1] = np.nan                                                         # star 0 lacks one band
    val[3, :] = np.nan                                                         # star 3 has no term at all
    lp = rng.normal(size=(T, S * W))
    lp[2, 0 * W + 3] = lp[2, 0 * W + 7] = lp[5, 0 * W + 1] = 50.0              # a tie: (t, w) = (2, 3) wins
    lp[1, 1 * W + 2] = np.nan                                                  # a NaN is skipped
    lp[:, 2 * W:3 * W] = np.nan                                                # all NaN: no MAP
    want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    got = tw.device(tab, x, lp, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    assert tw.rel_close(got["term_chi2"], want["term_chi2"])[0] and tw.rel_close(got["ppc"], want["ppc"])[0]
    np.testing.assert_array_equal(got["n_bad"], [0, 1, W * T, 0, 0, 0])
    np.testing.assert_array_equal(got["n_bad"], want["n_bad"])
    assert np.isnan(got["term_chi2"][0, 1]) and np.isfinite(got["ppc"][0])
    present = ~np.isnan(val[0])
    np.testing.assert_allclose(got["ppc"][0], got["term_chi2"][0, present].sum() / 6, rtol=1e-12)
    assert np.isnan(got["ppc"][2]) and np.isnan(got["ppc"][3]) and np.isnan(got["term_chi2"][3]).all()
    assert np.isfinite(got["ppc"][[1, 4, 5]]).all()
    np.testing.assert_array_equal(got["map_index"], want["map_index"])
    assert got["map_index"][0] == 2 * W + 3 and got["map_index"][2] == -1 and np.isnan(got["map_pars"][2]).all()
    assert tw.same_bits(got["map_pars"], want["map_pars"])
    assert np.isfinite(got["mags"][0, :, 4 * W]).all()                         # ... is on the grid (t = 1 in the last cell)
    ok, _ = tw.mags_close(got["mags"], want["mags"])
    assert ok
    # a Teff below the first BC node: the sample is off the BC grid, whatever the model grid says
    cold = (cols, ax3, bc, (ax4[0] + 1e5,) + ax4[1:])
    g2 = tw.device(cold, x, None, tw.PARAM_MAJOR, S, W, comps, i_dist, i_AV, val, unc)
    assert np.isnan(g2["mags"]).all() and (g2["n_bad"][[0, 1, 2, 4, 5]] == W * T).all() and g2["n_bad"][3] == 0
    assert (g2["map_index"] == -7).all() and (g2["map_pars"] == -7).all()      # lnprob null: the MAP outputs are not written


def test_surface_catalog_fit_and_single_model():
    import torch
    import isochrones_amd as ia
    from isochrones_amd import catalog as cat
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    c, _ = cat.synthetic_catalog(ic, 12, seed=2)
    kw = dict(nwalkers=32, nburn=20, niter=16, seed=3)
    out = cat.fit_catalog(c, ic, predictive=True, **kw)
    plain = cat.fit_catalog(c, ic, **kw)
    assert list(out.columns)[-1] == "ok" and "predictive_s" in out.attrs["timings"]["phases"]
    assert "predictive_s" not in plain.attrs["timings"]["phases"]
    shared = list(plain.columns)
    assert out[shared].values.tobytes() == plain.values.tobytes()
    rows, chain, lnp = cat.fit_stars_gpu(c, ic, np.arange(12), predictive=True, return_chains=True, **kw)
    names = cat.result_columns(cat._catalog_param_names(ic, 1), predictive=("V", "J", "K"))
    assert rows.shape[1] == len(names)
    x = np.ascontiguousarray(chain.permute(2, 3, 0, 1).reshape(16, 5, 12 * 32).cpu().numpy())
    lp = np.ascontiguousarray(lnp.permute(2, 0, 1).reshape(16, 12 * 32).cpu().numpy())
    from isochrones_amd import predictive as pv
    pcols, _ = cat.CatalogPosterior.build_columns(c, ic, N=1, indices=np.arange(12))
    val, unc = pv.pack_obs(pcols, ("V", "J", "K"), 12)
    m, b = ic.model_grid.interp, ic.bc_grid.interp
    tab = (np.ascontiguousarray(m.grid[..., list(ic._cols)]), tuple(np.asarray(a, dtype=np.float64) for a in m.index_columns),
           np.ascontiguousarray(b.grid[..., [int(i) for i in ic._band_cols(["V", "J", "K"])]]),
           tuple(np.asarray(a, dtype=np.float64) for a in b.index_columns))
    comps = [tuple(int(i) for i in ic.param_index_order[:3])]
    want = tw.predict(tab, x, lp, tw.PARAM_MAJOR, 12, 32, comps, 3, 4, val, unc)
    col = {n: rows[:, j] for j, n in enumerate(names)}
    ok = col["ok"] == 1
    assert ok.sum() >= 10
    assert tw.rel_close(col["ppc"][ok], want["ppc"][ok])[0]
    np.testing.assert_array_equal(col["ppc_nbad"][ok], want["n_bad"][ok])
    for j, t in enumerate(pv.term_names(("V", "J", "K"))):
        assert tw.rel_close(col["chi2_" + t][ok], want["term_chi2"][ok, j])[0], t
    for j, p in enumerate(cat._catalog_param_names(ic, 1)):
        assert tw.same_bits(col["map_" + p][ok], want["map_pars"][ok, j])
    for j, bnd in enumerate(("V", "J", "K")):
        q = np.percentile(want["mags"][:, j].reshape(16, 12, 32), [50, 16, 84], axis=(0, 2))       # [3, 12]
        for k, s in enumerate(("median", "p16", "p84")):
            np.testing.assert_allclose(col["%s_mag_%s" % (bnd, s)][ok], q[k][ok], rtol=0, atol=1e-9)
    # the kernel's own magnitude chain through the quantile kernel is numpy.percentile bit for bit; slicing changes no bit
    post = cat.CatalogPosterior.from_catalog(c, ic, N=1)
    from isochrones_amd.sampler import FusedEnsembleSampler
    smp = FusedEnsembleSampler(post, 32, seed=1)
    smp._chain, smp._lnprob = torch.as_tensor(x, device="cuda"), torch.as_tensor(lp, device="cuda")
    one = smp.predictive(ic, pcols, bands=("V", "J", "K"))
    per_ens = 16 * 3 * 32 * 8
    cut = smp.predictive(ic, pcols, bands=("V", "J", "K"), budget_bytes=5 * per_ens)
    for k in ("ppc", "term_chi2", "n_bad", "mag_quantiles", "map_pars", "map_index"):
        assert tw.same_bits(one[k].cpu().numpy(), cut[k].cpu().numpy()), k
    r = pv.predict_storage(smp._chain, smp._lnprob, 12, 32, ic, ("V", "J", "K"), pcols)
    mags = r.mags.cpu().numpy()
    q = np.moveaxis(np.percentile(mags.reshape(16, 3, 12, 32), [50, 16, 84], axis=(0, 3)), 0, -1).transpose(1, 0, 2)
    fin = ~np.isnan(q)
    assert tw.same_bits(one["mag_quantiles"].cpu().numpy()[fin], q[fin])
    smp.close()
    post.close()
    # a single model through fit_mcmc, and a binary on an isochrone table through addmags
    mod = ia.SingleStarModel(ic, Teff=(5770, 100), logg=(4.4, 0.1), V=(10.0, 0.05), J=(9.0, 0.05), parallax=(10.0, 0.1))
    mod.fit_mcmc(nwalkers=32, nburn=20, niter=16, seed=4)
    ppc, mp = mod.posterior_predictive, mod.map_pars
    assert np.isfinite(ppc) and ppc > 0 and mp.shape == (5,)
    assert np.isclose(mod.lnpost(mp), float(mod.sampler.lnprobability.max()))
    ages = ia.grids.mist_log_ages()[60::2]
    iso = ia.synthetic_isochrone(bands=("J", "K"), ages=ages, fehs=[-1.0, -0.5, 0.0, 0.5], eeps=np.arange(150.0, 700.0),
                                 eep_bounds=(150, 699), limits=dict(age=(ages[0], ages[-1]), feh=(-1.0, 0.5)))
    m2 = iso.interp_mag([380.0, 9.6, -0.1, 300.0, 0.1], ["J", "K"])[3]
    two = ia.BinaryStarModel(iso, J=(m2[0] - 0.4, 0.02), K=(m2[1] - 0.4, 0.02), parallax=(1000 / 300.0, 0.05))
    smp2 = two.fit_mcmc(nwalkers=40, nburn=30, niter=10, seed=2)
    assert np.isfinite(two.posterior_predictive) and two.map_pars.shape == (6,)
    obs = {k: two.kwargs[k] for k in ("J", "K", "parallax")}
    r = pv.chain_predictive(smp2.chain.contiguous(), smp2.lnprobability.contiguous(), iso, ("J", "K"), obs, N=2)
    d = two.derived_samples
    good = np.isfinite(d[["J_mag", "K_mag", "parallax"]].values).all(axis=1)            # the reference's mean skips the rest
    ref = sum(np.mean(((obs[k][0] - d[c].values) ** 2 / obs[k][1] ** 2)[good])
              for k, c in (("J", "J_mag"), ("K", "K_mag"), ("parallax", "parallax"))) / 3
    assert r.mags.shape == (40, 10, 2) and int(r.n_bad) == int((~good).sum()) and good.sum() > 200
    np.testing.assert_allclose(float(r.ppc), ref, rtol=1e-9)
    if isinstance(smp2, FusedEnsembleSampler):
        np.testing.assert_allclose(two.posterior_predictive, ref, rtol=1e-9)
    lpn = smp2.lnprobability.cpu().numpy()
    w, t = np.unravel_index(int(np.argmax(lpn)), lpn.shape)
    assert lpn[w, t] == lpn.T.ravel()[int(r.map_index)]
    np.testing.assert_array_equal(r.map_pars.cpu().numpy(), smp2.chain[w, t].cpu().numpy())
