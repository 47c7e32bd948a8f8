"""PopulationPosterior.star_posteriors / star_weights without a device: a host numpy chain goes through
iso_reweight_stars_host.  The naming, the defaults, the masks, the refusals, budget slicing equal to one slice, and the
numbers against the long-double twin."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import priors as P, reweight as rw
from isochrones_amd.csrc.libraries import HIER as build_hier, REWEIGHT as build_reweight
from tests import _reweight_twin as tw

S, W, T = 7, 4, 9
NAMES = ("feh", "mass", "other")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build_hier.build()
    build_reweight.build()


def _chain(seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(-0.2, 0.15, (S, W, T)), np.exp(rng.normal(0.0, 0.4, (S, W, T))), rng.normal(5.0, 2.0, (S, W, T))],
                    axis=3)


def _post(chain=None, **kw):
    model = ia.PopulationModel(feh=ia.TruncatedGaussian((-4.0, 0.5)), mass=ia.PowerLaw((0.1, 10.0)))
    interim = {"feh": P.FlatPrior((-4.0, 0.5)), "mass": P.PowerLawPrior(-2.35, (0.1, 10.0))}
    return ia.PopulationPosterior((_chain() if chain is None else chain, NAMES), None, model, interim=interim, **kw)


THETA = np.array([[-0.1, 0.3, -2.0], [0.0, 0.25, -1.5], [-0.2, 0.4, -2.5]])


def test_names_defaults_and_exports():
    assert ia.reweight is rw and rw.stat_names((0.5, 0.16, 0.84, 0.025, 0.9)) == ["median", "p16", "p84", "q2.5", "q90"]
    post = _post()
    df = post.star_posteriors(THETA)
    cols = [c + "_" + s for c in NAMES for s in ("median", "p16", "p84", "mean", "sd")] + ["ess", "n_bad"]
    assert list(df.columns) == cols and len(df) == S
    assert np.isfinite(df.to_numpy()).all() and (df["n_bad"] == 0).all() and (df["ess"] > 1).all() and (df["ess"] <= W * T).all()
    assert (df["feh_p16"] <= df["feh_median"]).all() and (df["feh_median"] <= df["feh_p84"]).all()
    one = post.star_posteriors(THETA, columns="other", q=(0.025, 0.5))
    assert list(one.columns) == ["other_q2.5", "other_median", "other_mean", "other_sd", "ess", "n_bad"]
    assert np.array_equal(one["other_median"], df["other_median"]) and np.array_equal(one["ess"], df["ess"])
    t = post.star_posteriors(THETA, as_tensors=True)
    assert list(t) == cols and all(np.array_equal(t[c].numpy(), df[c].to_numpy()) for c in cols)


def test_numbers_are_the_twin_s():
    chain = _chain(3)
    post = _post(chain)
    df = post.star_posteriors(THETA, q=tw.PROBS3)
    x = np.stack([chain[:, :, :, d].transpose(0, 2, 1).reshape(S, T * W) for d in range(3)])       # m = t * W + w
    case = dict(x=x[:2], y=x, values=[("y", 0), ("y", 1), ("y", 2)], interim=post.interim, rows=post.model.pack(THETA),
                mask=None, probs=tw.PROBS3)
    want = tw.reweight(case, ln_norm=post.star_terms(THETA)[0])
    assert not want["near_tie"].any()
    for v, col in enumerate(NAMES):
        for k, stat in enumerate(("median", "p16", "p84")):
            assert np.array_equal(df["%s_%s" % (col, stat)], want["quant"][:, v, k]), (col, stat)
        assert np.max(np.abs(df[col + "_mean"] - want["mean"][:, v]) / want["scale"][:, v]) <= 1e-10
        assert np.max(np.abs(df[col + "_sd"] - want["sd"][:, v]) / want["scale"][:, v]) <= 1e-10
    assert np.max(np.abs(df["ess"] / want["ess"] - 1.0)) <= 1e-10
    w = post.star_weights(THETA)
    assert w.shape == (S, W * T) and np.max(np.abs(w.sum(axis=1) - 1.0)) <= 1e-13
    norm = want["weights"] / want["wsum"][:, None]
    assert np.max(np.abs(w - norm) / norm) <= 1e-10
    # shrinkage: a narrow population pulls every star's feh towards its mean
    narrow = post.star_posteriors(np.array([[-0.1, 0.05, -2.0]]), columns=["feh"])
    plain = np.median(x[0], axis=1)
    assert (np.abs(narrow["feh_median"] + 0.1) < np.abs(plain + 0.1)).all() and (narrow["feh_sd"] < 0.06).all()


def test_star_weights_selects_stars():
    post = _post()
    w = post.star_weights(THETA)
    assert np.array_equal(post.star_weights(THETA, stars=[5, 2]), w[[5, 2]])
    assert np.array_equal(post.star_weights(THETA, stars=3), w[3:4])
    assert np.array_equal(post.star_weights(THETA, stars=slice(2, 6)), w[2:6])
    for bad in ([], [S], [-1], slice(0, S, 2), slice(3, 3)):
        with pytest.raises(ValueError, match="stars must be"):
            post.star_weights(THETA, stars=bad)


def test_masks_and_dead_stars():
    chain = _chain()
    chain[4, :, :, 0] = 3.0                         # outside the interim prior of feh: every sample of star 4 is bad
    chain[6, 1, 2, 1] = np.nan
    mask = np.ones(S, int)
    mask[1] = 0
    post = _post(chain, mask=mask)
    df = post.star_posteriors(THETA)
    stats = [c for c in df.columns if c != "n_bad"]
    assert df.loc[1, stats].isna().all() and df.loc[1, "n_bad"] == 0
    assert df.loc[4, "n_bad"] == W * T and df.loc[4, "ess"] == 0 and df.loc[4, [c for c in stats if c != "ess"]].isna().all()
    assert df.loc[6, "n_bad"] == 1 and np.isfinite(df.loc[[0, 2, 3, 5, 6], stats].to_numpy()).all()
    w = post.star_weights(THETA)
    assert np.isnan(w[[1, 4]]).all() and np.isfinite(w[[0, 2, 3, 5, 6]]).all() and w[6, 2 * W + 1] == 0.0
    same = _post(chain).star_posteriors(THETA)
    keep = [0, 2, 3, 4, 5, 6]
    assert same.loc[keep].equals(df.loc[keep])


def test_budget_slices_equal_one_slice():
    whole = _post()
    per_star = W * T * 8
    sliced = _post(budget_bytes=3 * per_star)
    assert [n for _, n in rw._slices(sliced, 0)] == [3, 3, 1] and rw._slices(whole, 0) == [(0, S)]
    assert rw._slices(sliced, 2) == [(s, 1) for s in range(S)]                 # the weights and two derived columns
    a, b = whole.star_posteriors(THETA), sliced.star_posteriors(THETA)
    assert a.equals(b)
    assert np.array_equal(whole.star_weights(THETA), sliced.star_weights(THETA))
    assert np.array_equal(whole.star_weights(THETA, stars=[6, 1]), sliced.star_weights(THETA, stars=[6, 1]))
    with pytest.raises(ValueError, match="more than budget_bytes"):
        rw._slices(_post(budget_bytes=per_star), 1)                            # one star's weights and one derived column


def test_more_than_eight_columns_go_in_groups():
    rng = np.random.default_rng(5)
    names = tuple("c%d" % i for i in range(11))
    chain = rng.normal(0.0, 1.0, (3, W, T, 11))
    model = ia.PopulationModel(c0=ia.TruncatedGaussian((-8.0, 8.0)))
    post = ia.PopulationPosterior((chain, names), None, model, interim={"c0": P.FlatPrior((-8.0, 8.0))})
    th = np.array([[0.2, 0.7], [0.0, 1.1]])
    df = post.star_posteriors(th)
    assert len(df.columns) == 11 * 5 + 2 and np.isfinite(df.to_numpy()).all()
    for col in ("c3", "c9"):
        one = post.star_posteriors(th, columns=[col])
        assert all(np.array_equal(one[c], df[c]) for c in one.columns)


def test_refusals_and_theta_default():
    post = _post()
    with pytest.raises(ValueError, match="run fit_mcmc first"):
        post.star_posteriors()
    with pytest.raises(ValueError, match="run fit_mcmc first"):
        post.star_weights()
    with pytest.raises(ValueError, match="neither a parameter of the chain"):
        post.star_posteriors(THETA, columns=["radius"])
    with pytest.raises(ValueError, match="1 to 8 probabilities"):
        post.star_posteriors(THETA, q=np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match="1 to 8 probabilities"):
        post.star_posteriors(THETA, q=())
    with pytest.raises(ValueError, match=r"inside \(0, 1\)"):
        post.star_posteriors(THETA, q=(0.5, 1.0))
    with pytest.raises(ValueError, match="repeats"):
        post.star_posteriors(THETA, q=(0.5, 0.5))
    with pytest.raises(ValueError, match="theta must be"):
        post.star_posteriors(np.zeros((2, 2)))
    # the default rows: at most 64, spread evenly over the fitted samples, the first and the last among them
    post.fit_mcmc(nwalkers=8, nburn=3, niter=12, seed=1)
    flat = post.sampler.flatchain.cpu().numpy()
    th = rw.default_theta(post)
    assert th.shape == (64, 3) and np.array_equal(th[0], flat[0]) and np.array_equal(th[-1], flat[-1])
    assert all((row == flat).all(axis=1).any() for row in th)
    df = post.star_posteriors()
    assert df.equals(post.star_posteriors(th)) and np.isfinite(df["feh_median"]).all()
    post.fit_mcmc(nwalkers=8, nburn=2, niter=3, seed=1)
    assert rw.default_theta(post).shape == (24, 3)
