"""star_posteriors, star_weights and star_bin_probabilities of a binned PopulationPosterior on the chains fit_catalog's fit
left on the device: an age histogram on evolution tracks (age is a derived column: the axis of the grid and a value column)
next to fixed mass and [Fe/H] densities, and [Fe/H] bins per age bin.  Finite rows for the unmasked stars; equal to the
host-entry route on the downloaded chain within 1e-11; the same bits under a budget_bytes that forces ten slices."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import catalog as cat, priors as P, reweight as rw

pytestmark = pytest.mark.gpu

AGE_EDGES = [5.0, 9.0, 9.7, 10.15]
FEH_EDGES = [-4.0, -0.3, 0.0, 0.5]
INTERIM = {"age": P.FlatPrior((5.0, 10.15)), "mass": P.PowerLawPrior(-2.35, (0.1, 10.0)), "feh": P.GaussianPrior(-0.1, 0.6)}
VALUES = ["age", "mass", "feh", "radius"]


@pytest.fixture(scope="module")
def fit():
    """A 64-star synthetic catalog fitted by fit_catalog; its fit function hands the stored chain over."""
    ic = ia.synthetic_track(bands=("V", "J", "K"))
    c, _ = cat.synthetic_catalog(ic, 64, seed=2)
    kept = []

    def keep_chain(*args, **kwargs):
        rows, chain, _ = cat.fit_stars_gpu(*args, return_chains=True, **kwargs)
        kept.append(chain)
        return rows

    res = cat.fit_catalog(c, ic, fit_fn=keep_chain, nwalkers=32, nburn=50, niter=50, seed=3)
    (chain,) = kept
    ok = res["ok"].to_numpy() != 0
    assert chain.is_cuda and chain.shape[:3] == (64, 32, 50) and ok.sum() >= 48
    names = tuple(cat._catalog_param_names(ic, 1))
    extra, _ = ia.chain_derived(chain, ic, ("age", "radius"))
    wide = np.concatenate([chain.cpu().numpy(), extra.cpu().numpy()], axis=3)
    return ic, chain, names, ok.astype(np.int32), wide


def _models():
    one = ia.PopulationModel(age=ia.Histogram(AGE_EDGES), mass=ia.Fixed(P.PowerLawPrior(-1.5, (0.1, 10.0))),
                             feh=ia.Fixed(P.GaussianPrior(0.0, 0.3)))
    two = ia.PopulationModel(feh=ia.Histogram(FEH_EDGES, given="age"), age=ia.Histogram(AGE_EDGES))
    return {"age": one, "feh given age": two}


@pytest.mark.parametrize("which", ["age", "feh given age"])
def test_binned_star_posteriors_on_a_catalog(fit, which):
    import torch
    ic, chain, names, mask, wide = fit
    model = _models()[which]
    interim = {c: INTERIM[c] for c in model.columns}
    S, W, T = 64, 32, 50
    live = np.flatnonzero(mask)
    rng = np.random.default_rng(4)
    theta = rng.uniform(-2.0, 2.0, (9, model.n_params))
    pp = ia.PopulationPosterior((chain, names), ic, model, interim=interim, mask=mask)
    assert model.binned and pp.derived_cols == ["age"] and not pp.host
    host = ia.PopulationPosterior((wide, names + ("age", "radius")), None, model, interim=interim, mask=mask)
    assert host.host

    df, want = pp.star_posteriors(theta, columns=VALUES), host.star_posteriors(theta, columns=VALUES)
    assert list(df.columns) == list(want.columns) and list(df.columns)[-3:] == ["ess", "n_bad", "n_out"]
    dead = np.flatnonzero(mask == 0)
    counts = ["n_bad", "n_out"]
    assert df.loc[dead, [c for c in df.columns if c not in counts]].isna().all().all() and (df.loc[dead, counts] == 0).all().all()
    assert np.isfinite(df.loc[live].to_numpy()).all() and (df.loc[live, "ess"] > 1).all()
    for c in df.columns:
        g, w = df[c].to_numpy()[live], want[c].to_numpy()[live]
        if c.endswith(("_median", "_p16", "_p84")) or c in counts:
            assert np.array_equal(g, w), c
        else:
            assert np.all(np.abs(g - w) <= 1e-11 * np.maximum(np.abs(w), 1.0)), (c, float(np.max(np.abs(g - w))))

    w, hw = pp.star_weights(theta), host.star_weights(theta)
    assert w.is_cuda and w.shape == (S, W * T)
    got = w.cpu().numpy()
    assert np.isnan(got[dead]).all() and np.all(np.abs(got[live].sum(axis=1) - 1.0) <= 1e-12)
    assert np.all(np.abs(got[live] - hw[live]) <= 1e-11 * hw[live])
    some = pp.star_weights(theta, stars=[int(live[5]), int(live[0])])
    assert torch.equal(some, w[[int(live[5]), int(live[0])]])

    cp, hcp = pp.star_bin_probabilities(theta), host.star_bin_probabilities(theta)
    shape = (S, 3) if which == "age" else (S, 3, 3)
    assert cp.is_cuda and tuple(cp.shape) == shape == hcp.shape
    got = cp.cpu().numpy()
    assert np.isnan(got[dead]).all() and np.isfinite(got[live]).all()
    assert np.all(np.abs(got[live].reshape(len(live), -1).sum(axis=1) - 1.0) <= 1e-12)
    assert np.all(np.abs(got[live] - hcp[live]) <= 1e-11 * hcp[live])

    # slices of seven stars: the model's derived column, radius and the weights are three doubles a sample
    cut = ia.PopulationPosterior((chain, names), ic, model, interim=interim, mask=mask, budget_bytes=7 * 3 * W * T * 8)
    assert [n for _, n in rw._slices(cut, 1)] == [7] * 9 + [1]
    assert cut.star_posteriors(theta, columns=VALUES).equals(df)
    assert torch.equal(torch.nan_to_num(cut.star_weights(theta)), torch.nan_to_num(w))
    assert torch.equal(torch.nan_to_num(cut.star_bin_probabilities(theta)), torch.nan_to_num(cp))
    # the default columns: the chain's parameters, then the model's derived column; n_out next to n_bad
    default = pp.star_posteriors(theta, as_tensors=True)
    assert [k for k in default if k.endswith("_mean")] == [n + "_mean" for n in names + ("age",)]
    assert default["age_median"].is_cuda and list(default)[-3:] == ["ess", "n_bad", "n_out"]
    assert np.array_equal(default["age_median"].cpu().numpy(), df["age_median"].to_numpy(), equal_nan=True)
