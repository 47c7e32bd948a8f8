"""PopulationPosterior.cell_counts, grad, hessian and maximize on the host route (a numpy chain goes through the host entries
of libiso_binned.so and libiso_binfit.so), no GPU needed: the derivatives against the long-double twin and against central
differences of the existing lnlike, for one axis, given= and two independent axes, with and without an injection set; EM on
point-like chains (the multinomial closed form), with a known detection fraction per cell, and on a noisy catalog drawn
from a known histogram; the bounds, the refusals."""
import numpy as np
import pytest
from scipy.stats import truncnorm

import isochrones_amd as ia
from isochrones_amd import priors as P
from isochrones_amd.csrc.libraries import BINFIT, BINNED, HIER, REWEIGHT, SHRINK
from tests import _binfit_twin as ft


@pytest.fixture(scope="module", autouse=True)
def built():
    for spec in (HIER, BINNED, REWEIGHT, SHRINK, BINFIT):
        spec.build()


def _chain(x, W, T):
    """[Q, S, M] (m = t * W + w) -> [S, W, T, Q]"""
    Q, S, _ = x.shape
    return np.ascontiguousarray(x.reshape(Q, S, T, W).transpose(1, 3, 2, 0))


E0, E1 = np.array([8.0, 8.7, 9.2, 9.6, 10.0]), np.array([-1.0, -0.4, 0.1, 0.5])
SHAPES = {"one": ("one", 4), "given": ("given", 4, 3), "indep": ("indep", 4, 3)}


def _model(kind):
    if kind == "one":
        return ia.PopulationModel(age=ia.Histogram(E0), mass=ia.Fixed(P.ChabrierPrior()))
    return ia.PopulationModel(age=ia.Histogram(E0), feh=ia.Histogram(E1, given="age" if kind == "given" else None))


def _posterior(kind, injections=False, S=40, W=8, T=12, seed=0):
    rng = np.random.default_rng(seed)
    M = W * T
    centre = rng.uniform(8.2, 9.8, (S, 1))
    age = centre + rng.normal(0.0, 0.35, (S, M))                      # a star's samples spread over a few bins, some outside
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
    model = _model(kind)
    pp = ia.PopulationPosterior((_chain(np.stack([age, second]), W, T), names), None, model, interim=interim, mask=mask,
                                injections=inj)
    return pp


def _lnvol(model):
    widths = [np.diff(model.families[q].edges) for q in model.axes]
    vol = widths[0] if len(widths) == 1 else widths[0][:, None] * widths[1][None, :]
    return np.log(vol).reshape(-1)


@pytest.mark.parametrize("kind, injections", [("one", False), ("given", False), ("indep", False), ("one", True), ("given", True),
                                               ("indep", True)])
def test_derivatives_against_the_twin_and_against_differences_of_lnlike(kind, injections):
    pp = _posterior(kind, injections)
    model = pp.model
    P_, B, _ = ft.blocks(SHAPES[kind])
    assert model.n_params == P_ and model.n_cells == B
    rng = np.random.default_rng(7)
    theta = rng.normal(0.0, 0.8, (3, P_))
    A = pp.bin_tables()[0]
    a_sel = pp.selection.tables[0].reshape(-1) if injections else None
    g, hs = pp.grad(theta), pp.hessian(theta)
    assert g.shape == (3, P_) and hs.shape == (3, P_, P_)
    for h in range(3):
        wg, wh = ft.derivatives(SHAPES[kind], theta[h], _lnvol(model), A, pp.mask, a_sel)
        eg = float(np.max(np.abs(g[h] - wg))) / max(1.0, float(np.max(np.abs(wg))))
        eh = float(np.max(np.abs(hs[h] - wh))) / max(1.0, float(np.max(np.abs(wh))))
        print("%s row %d: grad against the twin %.2e, hessian %.2e (relative to the largest entry)" % (kind, h, eg, eh))
        assert eg <= 1e-9 and eh <= 1e-9
        # the existing path: central differences of pp.lnlike, step 1e-5, tolerance 1e-6 max(1, max |g|)
        num = ft.central_gradient(lambda th: pp.lnlike(th[None, :])[0], theta[h])
        err = float(np.max(np.abs(num - g[h])))
        print("    against differences of lnlike: %.2e, max |g| = %.3g" % (err, np.max(np.abs(g[h]))))
        assert err <= 1e-6 * max(1.0, float(np.max(np.abs(g[h]))))
    # the counts: for one row the star-sum of star_bin_probabilities, and the two identities
    N, Cm, live = pp.cell_counts(theta, pairs=True)
    assert N.shape == (3, B) and Cm.shape == (3, B, B) and live.shape == (3,) and (live <= pp.n_unmasked).all()
    cp = pp.star_bin_probabilities(theta[1:2]).reshape(pp.S, B)
    alive = np.isfinite(cp).all(axis=1)
    assert alive.sum() == live[1] and np.all(np.abs(cp[alive].sum(axis=0) - N[1]) <= 1e-11 * max(1, live[1]))
    assert np.all(np.abs(N.sum(axis=1) - live) <= 1e-11 * live) and np.all(np.abs(Cm.sum(axis=2) - N) <= 1e-11 * live[:, None])
    N2, live2 = pp.cell_counts(theta)
    assert N2.tobytes() == N.tobytes() and np.array_equal(live2, live)
    # where theta lies: a tensor in, tensors out
    import torch
    tg = pp.grad(torch.from_numpy(theta))
    assert isinstance(tg, torch.Tensor) and tg.numpy().tobytes() == g.tobytes()
    tn = pp.cell_counts(torch.from_numpy(theta))
    assert isinstance(tn[0], torch.Tensor) and tn[0].numpy().tobytes() == N.tobytes() and tn[1].dtype == torch.int32


# -- point-like chains ------------------------------------------------------------------------------------------------
PE = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])


def _point_like(counts, injections=None, W=4, T=5, seed=1, edges=PE):
    """Every star's samples inside one cell of ``edges``, ``counts[b]`` stars in cell b, a flat interim prior."""
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(len(counts)), counts)
    x = edges[cells][:, None] + rng.uniform(0.05, 0.95, (cells.size, W * T)) * np.diff(edges)[cells][:, None]
    model = ia.PopulationModel(x=ia.Histogram(edges))
    return ia.PopulationPosterior((_chain(x[None], W, T), ("x",)), None, model, interim={"x": P.FlatPrior((-1.0, 7.0))},
                                  injections=injections)


def test_point_like_chains_give_the_multinomial():
    counts = np.array([5, 11, 2, 9, 17, 6])
    S = counts.sum()
    pp = _point_like(counts)
    one = pp.maximize(max_iter=1)
    assert one.n_iter == 1 and one.masses.shape == (6,) and one.on_bound == ()
    # one step: the result goes through log and exp, so 1e-12 and not 0
    assert np.all(np.abs(one.masses - counts / S) <= 1e-12)
    fit = pp.maximize()
    assert fit.converged and fit.n_iter == 2 and np.all(np.abs(fit.masses - counts / S) <= 1e-12)
    assert np.all(np.diff(fit.trace) >= -1e-9 * max(1.0, abs(fit.lnlike))) and fit.trace.size == 3
    assert abs(fit.lnlike - pp.lnlike(fit.theta[None])[0]) == 0.0
    assert np.all(np.abs(fit.density - counts / S / np.diff(PE)) <= 1e-12) and np.all(np.abs(fit.expected - counts) <= 1e-11 * S)
    # the Laplace covariance of the logits pushed to the masses is the multinomial's
    pi = counts / S
    multinomial = (np.diag(pi) - np.outer(pi, pi)) / S
    J = (np.diag(pi) - np.outer(pi, pi))[:, 1:]
    assert np.all(np.abs(J @ fit.cov @ J.T - multinomial) <= 1e-8)
    assert np.all(np.abs(fit.mass_sd - np.sqrt(np.diag(multinomial))) <= 1e-8)
    assert np.all(np.abs(fit.cov - np.linalg.inv(-pp.hessian(fit.theta[None])[0])) <= 1e-9 * np.abs(fit.cov).max())
    df = fit.frame()
    assert list(df.columns) == ["k0", "x_lo", "x_hi", "mass", "mass_sd", "density", "expected"] and len(df) == 6
    assert np.array_equal(df["x_lo"], PE[:-1]) and np.array_equal(df["x_hi"], PE[1:]) and np.array_equal(df["mass"], fit.masses)
    # another start ends in the same place
    far = pp.maximize(theta0=np.array([2.0, -3.0, 1.0, 0.0, -1.0]))
    assert far.converged and np.all(np.abs(far.masses - counts / S) <= 1e-12)
    assert isinstance(fit, ia.BinnedFit)


@pytest.mark.parametrize("edges", [PE, np.array([0.0, 0.5, 2.0, 3.0, 3.5, 5.0, 6.0])])
def test_a_known_detection_fraction_per_cell(edges):
    """100 injections per unit of x, evenly spaced, detected with probability d_b in cell b: the injection table is
    proportional to width_b d_b, the density of the detected stars' population to counts_b / (width_b d_b), and so the
    maximum-likelihood masses to counts / d_b whatever the widths (with unequal widths this holds only if the M-step
    carries the cell volumes)."""
    counts = np.array([8, 12, 4, 20, 10, 6])
    d = np.array([1.0, 0.8, 0.5, 0.9, 0.25, 0.6])
    xi = (np.arange(600) + 0.5) / 100.0
    per_cell = np.round(100 * np.diff(edges)).astype(int)
    assert np.array_equal(np.histogram(xi, edges)[0], per_cell)
    inj = ia.InjectionSet({"x": xi}, {"x": P.FlatPrior((0.0, 6.0))}, np.log(np.repeat(d, per_cell)))
    pp = _point_like(counts, inj, edges=edges)
    want = counts / d / (counts / d).sum()
    one = pp.maximize(max_iter=1)
    assert np.all(np.abs(one.masses - want) <= 1e-12)
    fit = pp.maximize()
    assert fit.converged and fit.n_iter <= 3 and np.all(np.abs(fit.masses - want) <= 1e-12)
    assert np.all(np.abs(fit.density - want / np.diff(edges)) <= 1e-12)
    assert np.all(np.diff(fit.trace) >= -1e-9 * max(1.0, abs(fit.lnlike)))
    assert np.all(np.abs(pp.grad(fit.theta[None])) <= 1e-9 * counts.sum())          # a stationary point of the selected lnlike
    assert np.isfinite(fit.cov).all() and (fit.mass_sd > 0).all()


def test_an_empty_cell_is_reported_on_its_bound():
    counts = np.array([7, 9, 0, 5, 3, 6])
    pp = _point_like(counts)
    fit = pp.maximize()
    assert fit.on_bound == ("x.a2",) and fit.theta[1] == -10.0 and fit.converged
    k = 1                                                              # the logit a2
    assert np.isnan(fit.cov[k]).all() and np.isnan(fit.cov[:, k]).all()
    rest = [0, 2, 3, 4]
    assert np.isfinite(fit.cov[np.ix_(rest, rest)]).all() and np.isfinite(fit.mass_sd).all()
    assert fit.masses[2] < 1e-4 and np.all(np.abs(np.delete(fit.masses, 2) - np.delete(counts, 2) / counts.sum()) <= 1e-4)


def test_a_floored_bin_is_on_its_bound_to_the_last_bit():
    """The M-step's logits of random six-bin masses with an empty bin: a bin floored at exp(lo) of bin 0 has the logit lo
    itself, and when bin 0 is floored at exp(-hi) of the heaviest bin that bin's logit is hi itself, so that the comparison
    with the bounds lists it in on_bound (computed from the floored mass it lands an ulp inside in about 1 % of the cases)."""
    from isochrones_amd.binfit import _logits
    rng = np.random.default_rng(0)
    lo, hi = -10.0, 10.0
    for _ in range(20000):
        pi = rng.dirichlet(np.ones(6))
        k = int(rng.integers(0, 6))
        pi[k] = 0.0
        pi /= pi.sum()
        a = _logits(pi, lo, hi)
        assert a.shape == (5,) and (a >= lo).all() and (a <= hi + 1e-14).all()
        if k > 0:
            assert a[k - 1] == lo
        else:
            assert a[int(np.argmax(pi)) - 1] == hi and (np.delete(a, int(np.argmax(pi)) - 1) < hi).all()
    # nothing floored: the plain log ratios
    pi = np.array([0.2, 0.5, 0.3])
    assert np.array_equal(_logits(pi, lo, hi), np.log(pi[1:]) - np.log(pi[0]))


# -- a noisy catalog from a known histogram ---------------------------------------------------------------------------
LO, HI, SIGMA = 0.0, 6.0, 1.0
EDGES = np.array([0.0, 0.8, 1.7, 3.0, 3.6, 4.9, 6.0])                # tests/test_shrink_python_cpu.py's six bins
PROBS = np.array([0.05, 0.30, 0.10, 0.25, 0.22, 0.08])
SEED = 5                                                             # one whose maximum is interior (DESIGN.md section 24 has the others)


def test_a_noisy_catalog_recovers_its_histogram():
    """200 stars drawn from the histogram PROBS on EDGES, observed with N(0, SIGMA) noise; a star's chain is N(x_obs, SIGMA)
    truncated to [LO, HI] under a flat interim prior.  The trace never falls (slack 1e-9 max(1, |L|) for rounding) and every
    mass lies within 5 mass_sd of the truth."""
    rng = np.random.default_rng(SEED)
    S, W, T = 200, 32, 64
    cell = rng.choice(6, S, p=PROBS)
    true = EDGES[cell] + rng.random(S) * np.diff(EDGES)[cell]
    xobs = true + rng.normal(0.0, SIGMA, S)
    a, b = (LO - xobs) / SIGMA, (HI - xobs) / SIGMA
    x = truncnorm.rvs(a[:, None], b[:, None], loc=xobs[:, None], scale=SIGMA, size=(S, W * T), random_state=rng)
    model = ia.PopulationModel(age=ia.Histogram(EDGES))
    pp = ia.PopulationPosterior((_chain(x[None], W, T), ("age",)), None, model, interim={"age": P.FlatPrior((LO, HI))})
    fit = pp.maximize()
    slack = 1e-9 * max(1.0, abs(fit.lnlike))
    pull = (fit.masses - PROBS) / fit.mass_sd
    print("noisy catalog: %d EM steps, converged %s, lnlike %.4f, masses %s, mass_sd %s, largest pull %.2f"
          % (fit.n_iter, fit.converged, fit.lnlike, np.round(fit.masses, 3), np.round(fit.mass_sd, 3), np.abs(pull).max()))
    assert np.all(np.diff(fit.trace) >= -slack) and fit.trace.size == fit.n_iter + 1
    assert fit.on_bound == () and np.isfinite(fit.mass_sd).all() and abs(fit.masses.sum() - 1.0) <= 1e-12
    assert np.all(np.abs(pull) <= 5.0)
    assert fit.lnlike >= pp.lnlike(np.log(PROBS[1:] / PROBS[0])[None])[0]         # no worse than the truth itself


# -- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    pp = _posterior("indep", injections=True)
    with pytest.raises(ValueError, match="closed-form"):
        pp.maximize()
    assert np.isfinite(pp.grad(np.zeros((1, pp.model.n_params)))).all()          # the derivatives are not refused
    # a cell with expected stars that no detected injection covers
    counts = np.array([4, 4, 4, 4, 4, 4])
    xi = (np.arange(600) + 0.5) / 100.0
    lnd = np.zeros(600)
    lnd[200:300] = -np.inf
    with pytest.raises(ValueError, match="no detected injection"):
        _point_like(counts, ia.InjectionSet({"x": xi}, {"x": P.FlatPrior((0.0, 6.0))}, lnd)).maximize()
    with pytest.raises(ValueError, match="theta0"):
        _point_like(counts).maximize(theta0=np.zeros(3))
    # a model without a Histogram
    rng = np.random.default_rng(0)
    x = rng.uniform(0.5, 2.0, (1, 3, 20))
    plain = ia.PopulationPosterior((_chain(x, 4, 5), ("mass",)), None, ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0))),
                                   interim={"mass": P.FlatPrior((0.1, 10.0))})
    for call in (lambda: plain.cell_counts(np.zeros((1, 1))), lambda: plain.grad(np.zeros((1, 1))),
                 lambda: plain.hessian(np.zeros((1, 1))), lambda: plain.maximize()):
        with pytest.raises(ValueError, match="Histogram"):
            call()
