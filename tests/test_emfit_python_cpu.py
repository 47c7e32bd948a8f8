"""PopulationPosterior.em_masses and bootstrap on the host route (a numpy chain goes through the host entries of
libiso_binned.so, libiso_binfit.so and libiso_emfit.so), no GPU needed: one step against N / sum N of the existing
cell_counts, with and without an injection set; the Poisson bootstrap of point-like chains against the multinomial's
standard deviation; the noisy six-bin catalog of DESIGN.md section 24 at a seed whose maximum lies on the boundary of the
simplex; the replicates' theta rows as hyper rows; the refusals."""
import numpy as np
import pytest
from scipy.stats import truncnorm

import isochrones_amd as ia
from isochrones_amd import _emfit_cabi as ec, emfit, priors as P
from isochrones_amd.csrc.libraries import BINFIT, BINNED, EMFIT, HIER, REWEIGHT, SELECT, SHRINK


@pytest.fixture(scope="module", autouse=True)
def built():
    for spec in (HIER, SELECT, BINNED, REWEIGHT, SHRINK, BINFIT, EMFIT):
        spec.build()


def _chain(x, W, T):
    """[Q, S, M] (m = t * W + w) -> [S, W, T, Q]"""
    Q, S, _ = x.shape
    return np.ascontiguousarray(x.reshape(Q, S, T, W).transpose(1, 3, 2, 0))


E0, E1 = np.array([8.0, 8.7, 9.2, 9.6, 10.0]), np.array([-1.0, -0.4, 0.1, 0.5])


def _posterior(kind, injections=False, S=40, W=8, T=12, seed=0):
    """The posteriors of tests/test_binfit_python_cpu.py: samples spread over a few bins, one masked star, and with
    ``injections`` a set with a detection probability that falls with age."""
    rng = np.random.default_rng(seed)
    M = W * T
    centre = rng.uniform(8.2, 9.8, (S, 1))
    age = centre + rng.normal(0.0, 0.35, (S, M))
    second = rng.uniform(0.2, 3.0, (S, M)) if kind == "one" else rng.uniform(-0.8, 0.3, (S, 1)) + rng.normal(0.0, 0.3, (S, M))
    names = ("age", "mass") if kind == "one" else ("age", "feh")
    interim = {"age": P.FlatPrior((5.0, 10.5)), names[1]: P.ChabrierPrior() if kind == "one" else P.GaussianPrior(-0.2, 0.8)}
    mask = np.ones(S, np.int32)
    mask[3] = 0
    inj = None
    if injections:
        J = 4000
        draw = {"age": P.FlatPrior((7.5, 10.5)),
                names[1]: P.PowerLawPrior(-1.5, (0.1, 10.0)) if kind == "one" else P.GaussianPrior(-0.2, 0.6, bounds=(-2.0, 1.0))}
        cols = {k: np.ascontiguousarray(p.sample(J, rng), dtype=np.float64) for k, p in draw.items()}
        lnd = np.where(rng.random(J) < 0.3, -np.inf, -rng.exponential(1.0, J)) - 0.3 * (cols["age"] - 7.5)
        inj = ia.InjectionSet(cols, draw, lnd)
    if kind == "one":
        model = ia.PopulationModel(age=ia.Histogram(E0), mass=ia.Fixed(P.ChabrierPrior()))
    else:
        model = ia.PopulationModel(age=ia.Histogram(E0), feh=ia.Histogram(E1, given="age" if kind == "given" else None))
    return ia.PopulationPosterior((_chain(np.stack([age, second]), W, T), names), None, model, interim=interim, mask=mask,
                                  injections=inj)


@pytest.mark.parametrize("kind, injections", [("one", False), ("given", False), ("one", True), ("given", True)])
def test_one_step_is_the_normalised_cell_counts(kind, injections):
    """The parent's code is the reference: one step of em_masses from theta0's masses equals N / sum N of cell_counts at
    theta0's heights within 1e-11.  With an injection set the start is h a / alpha and the heights g / a are the same h up to
    a factor, so the counts are the same ones."""
    pp = _posterior(kind, injections)
    rng = np.random.default_rng(3)
    theta = rng.normal(0.0, 0.8, (3, pp.model.n_params))
    g0 = np.stack([emfit.start_masses(pp, th) for th in theta])
    assert np.all(np.abs(g0.sum(axis=1) - 1.0) <= 1e-14)
    g, objective, n_iter, status, n_live = pp.em_masses(g0=g0, max_iter=1, tol=-np.inf)
    N, live = pp.cell_counts(theta)
    err = float(np.max(np.abs(g - N / N.sum(axis=1, keepdims=True))))
    print("%s, injections %s: one step against N / sum N of cell_counts %.2e (limit 1e-11)" % (kind, injections, err))
    assert g.shape == N.shape and err <= 1e-11
    assert np.array_equal(n_live, live) and (n_iter == 1).all() and (status == ec.MAX_ITER).all() and np.isfinite(objective).all()
    # the default start is the uniform masses of maximize's default theta0, and weights of one change nothing
    d = pp.em_masses(max_iter=1, tol=-np.inf)
    N0, _ = pp.cell_counts(np.zeros((1, pp.model.n_params)))
    assert d[0].shape == (1, pp.model.n_cells) and np.all(np.abs(d[0][0] - N0[0] / N0[0].sum()) <= 1e-11)
    ones = pp.em_masses(weights=np.ones((2, pp.S)), max_iter=1, tol=-np.inf)
    assert ones[0][0].tobytes() == ones[0][1].tobytes() == d[0][0].tobytes()
    # the run stops on its own and the objective is the weighted log likelihood up to a constant: it has risen
    full = pp.em_masses(g0=g0)
    assert (full[3] != ec.RUNNING).all() and (full[1] >= objective).all()


# -- point-like chains ------------------------------------------------------------------------------------------------
PE = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
COUNTS = np.array([60, 190, 100, 150])
BOOT_SEED = 0                                                       # fixed once on the host entry (see the test)


def _point_like(counts, W=4, T=5, seed=1, edges=PE):
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(len(counts)), counts)
    x = edges[cells][:, None] + rng.uniform(0.05, 0.95, (cells.size, W * T)) * np.diff(edges)[cells][:, None]
    model = ia.PopulationModel(x=ia.Histogram(edges))
    return ia.PopulationPosterior((_chain(x[None], W, T), ("x",)), None, model, interim={"x": P.FlatPrior((-1.0, 5.0))})


@pytest.mark.parametrize("weights", ["poisson", "bayesian"])
def test_point_like_chains_give_the_multinomial_and_its_errors(weights):
    """500 stars, each inside one of 4 bins: the unweighted fit is counts / S, and a bootstrap replicate's masses are the
    weighted counts over the weights' sum, whose standard deviation is the multinomial's sqrt(p (1 - p) / S) to first order
    in 1 / S (Poisson(1) counts and exponential weights both have variance 1).  The standard deviation over R = 400
    replicates has the standard error sd / sqrt(2 (R - 1)); the bound is 5 of them.  The seed was fixed once to one the host
    entry passes (largest pull 1.51 for the Poisson weights)."""
    S, R = int(COUNTS.sum()), 400
    p = COUNTS / S
    pp = _point_like(COUNTS)
    bs = pp.bootstrap(n_boot=R, seed=BOOT_SEED, weights=weights)
    assert isinstance(bs, ia.BinnedBootstrap) and bs.masses.shape == (R + 1, 4) and bs.n_boot == R
    assert np.all(np.abs(bs.point_masses - p) <= 1e-12) and np.array_equal(bs.point_masses, bs.masses[0])
    assert np.all(np.abs(bs.point_density - p / np.diff(PE)) <= 1e-12)
    assert (bs.status == ec.CONVERGED).all() and (bs.n_iter == 2).all() and (bs.n_live[0] == S)
    want = np.sqrt(p * (1 - p) / S)
    pull = (bs.mass_sd - want) / (want / np.sqrt(2 * (R - 1)))
    print("%s bootstrap of point-like chains: mass_sd %s against %s, pulls %s" % (weights, bs.mass_sd, want, np.round(pull, 2)))
    assert np.all(np.abs(pull) <= 5.0)
    assert np.all(np.abs(bs.mass_mean - p) <= 5.0 * want / np.sqrt(R))
    assert bs.mass_q.shape == (3, 4) and np.all(np.diff(bs.mass_q, axis=0) > 0) and np.all(np.abs(bs.mass_q[1] - p) <= want)
    # a replicate is the weighted counts over the weights' sum, and the weights are the library's
    w = emfit.star_weights(weights, BOOT_SEED, 1, 3, S)
    cells = np.repeat(np.arange(4), COUNTS)
    for r in range(3):
        wc = np.bincount(cells, weights=w[r], minlength=4)
        assert np.all(np.abs(bs.masses[1 + r] - wc / wc.sum()) <= 1e-12)
    # the same weights given as an array are the same replicates
    again = pp.bootstrap(weights=emfit.star_weights(weights, BOOT_SEED, 1, 7, S))
    assert again.n_boot == 7 and again.weights == "given" and again.masses.tobytes() == bs.masses[:8].tobytes()
    df = bs.frame()
    assert list(df.columns) == ["k0", "x_lo", "x_hi", "mass", "mass_mean", "mass_sd", "mass_q16", "mass_q50", "mass_q84", "density"]
    assert len(df) == 4 and np.array_equal(df["mass"], bs.point_masses) and np.array_equal(df["x_hi"], PE[1:])


def test_the_slices_of_a_small_budget_give_the_same_replicates():
    S = int(COUNTS.sum())
    pp = _point_like(COUNTS)
    whole = pp.bootstrap(n_boot=40, seed=3)
    pp.budget = 7 * S * 8                                               # seven replicates' weights a slice
    sliced = pp.bootstrap(n_boot=40, seed=3)
    for k in ("masses", "theta", "n_iter", "status", "objective", "n_live"):
        assert getattr(sliced, k).tobytes() == getattr(whole, k).tobytes(), k


def test_a_bootstrap_from_a_start_with_a_subnormal_cell_has_finite_masses():
    """Point-like chains with one star alone in the first bin, and replicates that share one start row whose first cell has
    the subnormal mass 1e-310 (what an earlier fit leaves of a cell it has emptied): w / s1 of that star is beyond float64,
    and its products are taken again relative to their largest (include/isochrones_amd_emfit.h).  Every replicate has
    finite masses, counts that star where its weight is above 0, and ends at the weighted counts over the weights' sum."""
    counts = np.array([1, 20, 15, 14])
    S, R = int(counts.sum()), 12
    pp = _point_like(counts)
    w = emfit.star_weights("poisson", 5, 1, R, S)
    w[0] = 1.0
    assert (w[:, 0] > 0).any() and (w[:, 0] == 0).any()
    g, objective, n_iter, status, n_live = pp.em_masses(weights=w, g0=np.array([1e-310, 0.4, 0.3, 0.3]))
    assert np.isfinite(g).all() and np.isfinite(objective).all() and (status == ec.CONVERGED).all()
    assert np.array_equal(n_live, (w > 0).sum(axis=1))
    cells = np.repeat(np.arange(4), counts)
    for r in range(R):
        wc = np.bincount(cells, weights=w[r], minlength=4)
        assert np.all(np.abs(g[r] - wc / wc.sum()) <= 1e-12), r


# -- the noisy catalog of section 24 at a seed whose maximum is on the boundary ---------------------------------------
LO, HI, SIGMA = 0.0, 6.0, 1.0
EDGES = np.array([0.0, 0.8, 1.7, 3.0, 3.6, 4.9, 6.0])
PROBS = np.array([0.05, 0.30, 0.10, 0.25, 0.22, 0.08])
SEED = 0                # chosen: one of the thirteen seeds of 0 .. 15 whose maximum gives a cell no mass (section 24)


def _noisy(seed, S=200, W=32, T=64):
    rng = np.random.default_rng(seed)
    cell = rng.choice(6, S, p=PROBS)
    true = EDGES[cell] + rng.random(S) * np.diff(EDGES)[cell]
    xobs = true + rng.normal(0.0, SIGMA, S)
    a, b = (LO - xobs) / SIGMA, (HI - xobs) / SIGMA
    x = truncnorm.rvs(a[:, None], b[:, None], loc=xobs[:, None], scale=SIGMA, size=(S, W * T), random_state=rng)
    model = ia.PopulationModel(age=ia.Histogram(EDGES))
    return ia.PopulationPosterior((_chain(x[None], W, T), ("age",)), None, model, interim={"age": P.FlatPrior((LO, HI))})


def test_a_maximum_on_the_boundary_has_bootstrap_errors():
    """Section 24's 200 noisy stars at a seed (chosen) where the maximum-likelihood histogram gives the fourth cell no mass:
    maximize reports the logit on its bound, its Laplace covariance is NaN there, and the delta-method mass_sd of that cell
    is no error bar (the true mass 0.25 lies thousands of them away).  The bootstrap's mass_sd is finite for every cell
    and every true mass lies within 5 of them (largest pull 2.97)."""
    pp = _noisy(SEED)
    fit = pp.maximize()
    assert fit.on_bound == ("age.a3",) and np.isnan(fit.cov).any()
    with np.errstate(divide="ignore"):
        assert np.abs((fit.masses - PROBS) / fit.mass_sd).max() > 5.0
    bs = pp.bootstrap(n_boot=200, seed=0)
    pull = (bs.point_masses - PROBS) / bs.mass_sd
    print("noisy catalog on the boundary: masses %s, bootstrap mass_sd %s, largest pull %.2f, statuses %s, steps up to %d"
          % (np.round(bs.point_masses, 3), np.round(bs.mass_sd, 3), np.abs(pull).max(), np.bincount(bs.status, minlength=4),
             bs.n_iter.max()))
    assert np.isfinite(bs.mass_sd).all() and (bs.mass_sd > 0).all() and np.all(np.abs(pull) <= 5.0)
    assert bs.point_masses[3] < 1e-3 and np.all(np.abs(bs.point_masses - fit.masses) <= 1e-3)
    assert (bs.status != ec.EMPTY).all() and (bs.status != ec.RUNNING).all()
    assert np.all(bs.mass_q[0] <= bs.mass_q[1]) and np.all(bs.mass_q[1] <= bs.mass_q[2])
    # a replicate's theta is a hyper row: the stars' bin probabilities under it
    for r in (0, 1, 200):
        cp = pp.star_bin_probabilities(bs.theta[r:r + 1]).reshape(pp.S, 6)
        assert np.isfinite(cp).all() and np.all(np.abs(cp.sum(axis=1) - 1.0) <= 1e-12)
    assert np.isfinite(pp.lnlike(bs.theta)).all() and bs.theta.shape == (201, 5)
    assert np.all(bs.theta >= pp.model.ranges[:, 0]) and np.all(bs.theta <= pp.model.ranges[:, 1])
    assert pp.lnlike(bs.theta[:1])[0] >= fit.lnlike - 1e-6


# -- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    for injections in (False, True):
        pp = _posterior("indep", injections=injections)
        for call in (pp.bootstrap, pp.em_masses):
            with pytest.raises(ValueError, match="independent"):
                call()
    rng = np.random.default_rng(0)
    x = rng.uniform(0.5, 2.0, (1, 3, 20))
    plain = ia.PopulationPosterior((_chain(x, 4, 5), ("mass",)), None, ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0))),
                                   interim={"mass": P.FlatPrior((0.1, 10.0))})
    for call in (plain.bootstrap, plain.em_masses):
        with pytest.raises(ValueError, match="Histogram"):
            call()
    pp = _point_like(np.array([4, 4, 4, 4]))
    for n in (1, 0, -3):
        with pytest.raises(ValueError, match="n_boot"):
            pp.bootstrap(n_boot=n)
    with pytest.raises(ValueError, match="n_boot"):
        pp.bootstrap(weights=np.ones((1, 16)))
    with pytest.raises(ValueError, match="poisson"):
        pp.bootstrap(weights="jackknife")
    with pytest.raises(ValueError, match="weights must be"):
        pp.bootstrap(weights=np.ones((5, 15)))
    with pytest.raises(ValueError, match="not negative"):
        pp.bootstrap(weights=-np.ones((5, 16)))
    with pytest.raises(ValueError, match="theta0"):
        pp.bootstrap(theta0=np.zeros(2))
    with pytest.raises(ValueError, match="weights must be"):
        pp.em_masses(weights=np.ones(16))
    with pytest.raises(ValueError, match="not negative"):
        pp.em_masses(weights=np.full((2, 16), np.nan))
    with pytest.raises(ValueError, match="g0"):
        pp.em_masses(g0=np.array([0.5, 0.5, -0.1, 0.1]))
    with pytest.raises(ValueError, match="g0"):
        pp.em_masses(g0=np.zeros(4))
    with pytest.raises(ValueError, match="cells"):
        pp.em_masses(g0=np.ones(3))
    # a cell with expected stars that no detected injection covers: maximize's refusal
    xi = (np.arange(400) + 0.5) / 100.0
    lnd = np.zeros(400)
    lnd[200:300] = -np.inf
    counts = np.array([4, 4, 4, 4])
    rng = np.random.default_rng(1)
    cells = np.repeat(np.arange(4), counts)
    xs = PE[cells][:, None] + rng.uniform(0.05, 0.95, (16, 20))
    hole = ia.PopulationPosterior((_chain(xs[None], 4, 5), ("x",)), None, ia.PopulationModel(x=ia.Histogram(PE)),
                                  interim={"x": P.FlatPrior((-1.0, 5.0))},
                                  injections=ia.InjectionSet({"x": xi}, {"x": P.FlatPrior((0.0, 4.0))}, lnd))
    for call in (hole.bootstrap, hole.em_masses, hole.maximize):
        with pytest.raises(ValueError, match="no detected injection"):
            call()
    assert ia.BinnedBootstrap is emfit.BinnedBootstrap and ia.emfit is emfit
