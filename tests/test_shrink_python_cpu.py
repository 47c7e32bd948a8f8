"""PopulationPosterior.star_posteriors, star_weights and star_bin_probabilities on a binned model, on the host route (a numpy
chain goes through the host entries of libiso_binned.so, libiso_shrink.so and libiso_reweight.so), no GPU needed: the
frame's columns, the shapes, the errors, budget slices, more than eight value columns, and the closed form of a Gaussian
likelihood under a fixed histogram."""
import numpy as np
import pytest
from scipy.stats import norm, truncnorm

import isochrones_amd as ia
from isochrones_amd import priors as P, reweight as rw
from isochrones_amd.csrc.libraries import BINNED, HIER, RELATION, REWEIGHT, SHRINK


@pytest.fixture(scope="module", autouse=True)
def built():
    for spec in (HIER, BINNED, REWEIGHT, RELATION, SHRINK):
        spec.build()


def _chain(x, W, T):
    """[Q, S, M] (m = t * W + w) -> [S, W, T, Q]"""
    Q, S, _ = x.shape
    return np.ascontiguousarray(x.reshape(Q, S, T, W).transpose(1, 3, 2, 0))


def _logits(p):
    p = np.asarray(p, dtype=np.float64)
    return np.log(p[..., 1:] / p[..., :1])


# -- the closed form --------------------------------------------------------------------------------------------------
LO, HI, SIGMA = 0.0, 6.0, 1.0
EDGES = np.array([0.0, 0.8, 1.7, 3.0, 3.6, 4.9, 6.0])              # six bins of unequal width (mean width 1.0 = SIGMA)
PROBS = np.array([0.05, 0.30, 0.10, 0.25, 0.22, 0.08])             # and unequal heights


@pytest.fixture(scope="module")
def closed():
    """200 stars, one column, a flat interim prior on [LO, HI]: a star's chain is N(x_obs, SIGMA) truncated to the range,
    so under the fixed histogram h its posterior is h(x) N(x; x_obs, SIGMA), whose cell masses and mean are sums of Phi and
    phi at the edges."""
    rng = np.random.default_rng(2)
    S, W, T = 200, 32, 64
    xobs = rng.uniform(LO + 0.3, HI - 0.3, S)
    a, b = (LO - xobs) / SIGMA, (HI - xobs) / SIGMA
    x = truncnorm.rvs(a[:, None], b[:, None], loc=xobs[:, None], scale=SIGMA, size=(S, W * T), random_state=rng)
    model = ia.PopulationModel(age=ia.Histogram(EDGES))
    pp = ia.PopulationPosterior((_chain(x[None], W, T), ("age",)), None, model, interim={"age": P.FlatPrior((LO, HI))})
    theta = _logits(PROBS)[None]
    h = PROBS / np.diff(EDGES)
    cdf, pdf = norm.cdf((EDGES[None] - xobs[:, None]) / SIGMA), norm.pdf((EDGES[None] - xobs[:, None]) / SIGMA)
    mass = h[None] * np.diff(cdf, axis=1)                           # h_b [Phi((e_{b+1} - x_obs) / s) - Phi((e_b - x_obs) / s)]
    first = h[None] * (xobs[:, None] * np.diff(cdf, axis=1) - SIGMA * np.diff(pdf, axis=1))     # h_b int_b x N(x; x_obs, s) dx
    return pp, theta, x, mass / mass.sum(axis=1, keepdims=True), first.sum(axis=1) / mass.sum(axis=1)


def test_the_frame_the_weights_and_the_shapes(closed):
    pp, theta, x, _, _ = closed
    df = pp.star_posteriors(theta)
    assert list(df.columns) == ["age_median", "age_p16", "age_p84", "age_mean", "age_sd", "ess", "n_bad", "n_out"]
    assert len(df) == pp.S and np.isfinite(df.to_numpy()).all() and (df["n_bad"] == 0).all() and (df["n_out"] == 0).all()
    assert (df["age_p16"] < df["age_median"]).all() and (df["age_median"] < df["age_p84"]).all()
    assert (df["ess"] > 100).all() and (df["ess"] <= pp.W * pp.T).all()
    w = pp.star_weights(theta)
    assert w.shape == (pp.S, pp.W * pp.T) and np.all(np.abs(w.sum(axis=1) - 1.0) <= 1e-12) and (w >= 0).all()
    mean = (w * x).sum(axis=1)
    assert np.all(np.abs(mean - df["age_mean"].to_numpy()) <= 1e-11 * np.abs(mean))
    some = pp.star_weights(theta, stars=[7, 3])
    assert some.shape == (2, pp.W * pp.T) and np.array_equal(some[0], w[7]) and np.array_equal(some[1], w[3])
    assert np.array_equal(pp.star_weights(theta, stars=slice(5, 9)), w[5:9])
    cp = pp.star_bin_probabilities(theta)
    assert cp.shape == (pp.S, 6) and np.all(np.abs(cp.sum(axis=1) - 1.0) <= 1e-12) and (cp >= 0).all()
    # the cell probabilities are the normalised weights summed per cell
    cell = np.searchsorted(EDGES, x, side="right") - 1
    for s in (0, 17, 199):
        assert np.allclose(np.bincount(cell[s], w[s], minlength=6), cp[s], rtol=0, atol=1e-12)
    t = pp.star_posteriors(theta, q=(0.5, 0.025), as_tensors=True)
    assert set(t) == {"age_median", "age_q2.5", "age_mean", "age_sd", "ess", "n_bad", "n_out"}
    assert t["age_mean"].numpy().tobytes() == df["age_mean"].to_numpy().tobytes()


def test_closed_form(closed):
    """Every star's weighted mean within 5 of its standard errors (weighted sd / sqrt(ess)) of the analytic mean, every cell
    probability within 5 binomial standard errors at ess of the analytic one; no star and no cell left out."""
    pp, theta, _, want_p, want_mean = closed
    df = pp.star_posteriors(theta)
    ess = df["ess"].to_numpy()
    r_mean = np.abs(df["age_mean"].to_numpy() - want_mean) / (df["age_sd"].to_numpy() / np.sqrt(ess))
    cp = pp.star_bin_probabilities(theta)
    r_cell = np.abs(cp - want_p) / np.sqrt(want_p * (1.0 - want_p) / ess[:, None])
    print("closed form: largest |d mean| / se = %.2f, largest |d p| / se = %.2f, smallest ess = %.0f"
          % (r_mean.max(), r_cell.max(), ess.min()))
    assert r_mean.shape == (200,) and r_cell.shape == (200, 6) and np.isfinite(r_mean).all() and np.isfinite(r_cell).all()
    assert (r_mean <= 5.0).all() and (r_cell <= 5.0).all()
    # more rows of the same histogram change nothing but rounding: the rows are equally weighted draws
    again = pp.star_posteriors(np.repeat(theta, 3, axis=0))
    assert np.allclose(again["age_mean"], df["age_mean"], rtol=1e-12, atol=0) and np.allclose(again["ess"], df["ess"], rtol=1e-11)


def test_two_axes_slices_groups_and_masks():
    rng = np.random.default_rng(5)
    S, W, T = 9, 8, 25
    age = rng.uniform(7.9, 10.2, (S, W * T))
    feh = rng.uniform(-1.1, 0.6, (S, W * T))
    mass = rng.uniform(0.5, 2.0, (S, W * T))
    extra = rng.normal(size=(8, S, W * T))
    names = ("age", "feh", "mass") + tuple("z%d" % i for i in range(8))
    chain = _chain(np.concatenate([np.stack([age, feh, mass]), extra]), W, T)
    e0, e1 = [8.0, 9.0, 9.5, 10.0], [-1.0, -0.5, 0.0, 0.25, 0.5]
    model = ia.PopulationModel(feh=ia.Histogram(e1, given="age"), mass=ia.Fixed(P.ChabrierPrior()), age=ia.Histogram(e0))
    interim = {"age": P.FlatPrior((7.5, 10.5)), "feh": P.GaussianPrior(0.0, 0.6), "mass": P.FlatPrior((0.1, 10.0))}
    mask = np.ones(S, np.int32)
    mask[4] = 0
    pp = ia.PopulationPosterior((chain, names), None, model, interim=interim, mask=mask)
    theta = rng.normal(0.0, 0.7, (5, model.n_params))
    df = pp.star_posteriors(theta)                                  # eleven value columns: two summary groups
    assert len(df.columns) == 11 * 5 + 3 and np.isnan(df.iloc[4].drop(["n_bad", "n_out"])).all()
    assert np.isfinite(df.drop(index=4).to_numpy()).all() and (df["n_out"].drop(index=4) > 0).all() and df["n_out"][4] == 0
    cp = pp.star_bin_probabilities(theta)
    assert cp.shape == (S, 3, 4) and np.isnan(cp[4]).all() and np.allclose(np.delete(cp, 4, 0).sum(axis=(1, 2)), 1.0, atol=1e-12)
    w = pp.star_weights(theta)
    assert np.isnan(w[4]).all() and np.allclose(np.delete(w, 4, 0).sum(axis=1), 1.0, atol=1e-12)
    # the cell of the grid is (age bin, feh bin) whatever the order of the model's columns
    k0 = np.searchsorted(e0, age, side="right") - 1
    k1 = np.searchsorted(e1, feh, side="right") - 1
    inside = (age >= e0[0]) & (age <= e0[-1]) & (feh >= e1[0]) & (feh <= e1[-1])
    got = np.zeros((3, 4))
    np.add.at(got, (k0[0][inside[0]], k1[0][inside[0]]), w[0][inside[0]])
    assert np.allclose(got, cp[0], rtol=0, atol=1e-12) and (w[0][~inside[0]] == 0).all()
    # a budget of two stars a slice: the same bits
    small = ia.PopulationPosterior((chain, names), None, model, interim=interim, mask=mask, budget_bytes=2 * W * T * 8)
    assert len(rw._slices(small, 0)) == 5
    assert small.star_posteriors(theta).to_numpy().tobytes() == df.to_numpy().tobytes()
    assert small.star_weights(theta).tobytes() == w.tobytes()
    # one group alone is the same columns
    one = pp.star_posteriors(theta, columns=["z7", "age"])
    assert one["z7_mean"].to_numpy().tobytes() == df["z7_mean"].to_numpy().tobytes()
    assert one["age_p84"].to_numpy().tobytes() == df["age_p84"].to_numpy().tobytes()


def test_errors(closed):
    pp, theta, x, _, _ = closed
    chain = pp.storage.reshape(pp.T, 1, pp.S, pp.W).transpose(2, 3, 0, 1)[:5]
    plain = ia.PopulationPosterior((chain, ("age",)), None, ia.PopulationModel(age=ia.TruncatedGaussian((LO, HI))),
                                   interim={"age": P.FlatPrior((LO, HI))})
    with pytest.raises(ValueError, match="Histogram"):
        plain.star_bin_probabilities(np.array([[3.0, 1.0]]))
    assert np.isfinite(plain.star_posteriors(np.array([[3.0, 1.0]])).to_numpy()).all()
    assert "n_out" not in plain.star_posteriors(np.array([[3.0, 1.0]])).columns         # an unbinned model's frame is as it was
    with pytest.raises(ValueError, match="fit_mcmc"):
        pp.star_bin_probabilities()
    with pytest.raises(ValueError, match="fit_mcmc"):
        pp.star_posteriors()
    with pytest.raises(ValueError, match=r"theta must be \[H, 5\]"):
        pp.star_posteriors(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="1 to 8 probabilities"):
        pp.star_posteriors(theta, q=np.linspace(0.1, 0.9, 9))
    # a coupled model still raises its error
    two = np.concatenate([chain, chain], axis=3)
    linked = ia.PopulationModel(x=ia.TruncatedGaussian((LO, HI)), y=ia.LinearGaussian("x", (-4.0, 8.0), (-1.0, 1.0)))
    cp = ia.PopulationPosterior((two, ("x", "y")), None, linked, interim={"x": P.FlatPrior((LO, HI)), "y": P.FlatPrior((LO, HI))})
    row = np.zeros((1, linked.n_params))
    with pytest.raises(ValueError, match="uncoupled.*y on x"):
        cp.star_posteriors(row)
    with pytest.raises(ValueError, match="uncoupled.*y on x"):
        cp.star_weights(row)
    with pytest.raises(ValueError, match="Histogram"):
        cp.star_bin_probabilities(row)


def test_default_theta_after_fit_mcmc(closed):
    pp = closed[0]
    chain = pp.storage.reshape(pp.T, 1, pp.S, pp.W).transpose(2, 3, 0, 1)[:20]
    small = ia.PopulationPosterior((chain, ("age",)), None, pp.model, interim={"age": P.FlatPrior((LO, HI))})
    small.fit_mcmc(nwalkers=12, nburn=3, niter=3, seed=1)
    rows = rw.default_theta(small)
    cp = small.star_bin_probabilities()
    assert cp.shape == (20, 6) and cp.tobytes() == small.star_bin_probabilities(rows).tobytes()
    assert small.star_posteriors().to_numpy().tobytes() == small.star_posteriors(rows).to_numpy().tobytes()
