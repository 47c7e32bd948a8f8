"""StarClusterModel on the device (libiso_cluster.so): the reference's own numbers (tests/golden/cluster/) in every calling
form, the numpy restatement (tests/_cluster_ref.py) at shapes too large for fixtures, the long-double reference
(tests/_cluster_hp.py) over columns from the CPU oracle at 32 bands, 8 properties and the notebook shape, bitwise row
independence, and fits."""
import numpy as np
import pandas as pd
import pytest

import isochrones_amd as ia

from . import _cluster_hp as H
from . import _cluster_ref as R
from . import _fixtures as fx

pytestmark = pytest.mark.gpu

TRUTH_NB = [8.84, -0.2, 500.0, 0.03, -3.0, 0.3, 0.3]      # the Overview notebook's parameters


def _close(got, want, what, tol=1e-9):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, got, want)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (what, got, want)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= tol * (1 + np.abs(want[fin]))), (what, err.max() if err.size else 0)


@pytest.mark.parametrize("case", R.CASES)
def test_goldens_in_every_calling_form(case):
    import torch
    fx = R.load(case)
    ic = R.make_ic(fx)
    defined = ~fx["undefined"]
    for q in np.unique(fx["minq"]):
        rows = np.flatnonzero((fx["minq"] == q) & defined)
        mod = R.make_model(fx, q, ic=ic)
        x = fx["pars"][rows]
        for which in ("lnprior", "lnlike", "lnpost"):
            want = fx[which][rows]
            fn = getattr(mod, which)
            _close(fn(x), want, (case, which, "numpy"))
            t = fn(torch.as_tensor(x, device="cuda"))
            assert t.is_cuda
            _close(t.cpu().numpy(), want, (case, which, "tensor"))
            _close([fn(r) for r in x], want, (case, which, "scalar"))
        like, per_star = mod.lnlike_stars(x)
        with np.errstate(divide="ignore", invalid="ignore"):
            _close(per_star, np.log(fx["like_tot"][rows]), (case, "ln like_s"))


def _stars(ic, rng, n, age, feh, dist, AV, bands, eep_range, binary_fraction=0.3):
    pri = rng.uniform(*eep_range, n)
    sec = pri - rng.uniform(1.0, 0.5 * (eep_range[1] - eep_range[0]), n)
    binary = rng.random(n) < binary_fraction
    o = np.ones(n)
    _, _, _, mp = ic.interp_mag([pri, age * o, feh * o, dist * o, AV * o], list(bands))
    _, _, _, ms = ic.interp_mag([sec, age * o, feh * o, dist * o, AV * o], list(bands))
    tot = np.where(binary[:, None] & np.isfinite(ms), -2.5 * np.log10(10 ** (-0.4 * mp) + 10 ** (-0.4 * ms)), mp)
    df = pd.DataFrame()
    for i, b in enumerate(bands):
        df[b + "_mag"] = tot[:, i] + 0.02 * rng.standard_normal(n)
        df[b + "_mag_unc"] = 0.02
    df["parallax"] = 1000.0 / dist + 0.1 * rng.standard_normal(n)
    df["parallax_unc"] = 0.1
    assert np.isfinite(tot).all()
    return df


def _restated(mod, p):
    """ln like_s of the numpy restatement, the per-EEP columns taken from the device interpolators."""
    ic = mod.ic
    lo, hi = mod.bounds("eep")
    E = np.arange(lo, hi + 1).astype(float)
    o = np.ones(E.size)
    vals = np.asarray(ic.interp_value([E, p[0] * o, p[1] * o], ["initial_mass", "dm_deep"]), dtype=float).reshape(E.size, 2)
    ok = np.isfinite(vals[:, 0])
    E, vals, o = E[ok], vals[ok], o[ok]
    if E.size:
        _, _, _, mags = ic.interp_mag([E, p[0] * o, p[1] * o, p[2] * o, p[3] * o], list(mod.bands))
        mags = np.asarray(mags, dtype=float).reshape(E.size, len(mod.bands))
    else:
        mags = np.zeros((0, len(mod.bands)))
    m = [mod.stars.measurements[b] for b in mod.bands]
    pm = [mod.stars.measurements[q] for q in mod.props]
    ns = len(mod.stars)
    prop_model = np.column_stack([np.full(E.size, 1000.0 / p[2]) if q == "parallax" else
                                  np.asarray(ic.interp_value([E, p[0] * o, p[1] * o], [q]), dtype=float).reshape(-1)
                                  for q in mod.props]) if mod.props else np.zeros((E.size, 0))
    like = R.like_per_star(E, vals[:, 0], np.log(np.abs(vals[:, 1])), mags, prop_model,
                           np.column_stack([a for a, _ in m]), np.column_stack([u for _, u in m]),
                           np.column_stack([a for a, _ in pm]) if pm else np.zeros((ns, 0)),
                           np.column_stack([u for _, u in pm]) if pm else np.zeros((ns, 0)),
                           p[4], p[5], p[6], *mod.bounds("mass"), mod.minq)
    return like


def _check_restated(mod, rows):
    lnl, per_star = mod.lnlike_stars(np.asarray(rows, dtype=float))
    for i, p in enumerate(rows):
        like = _restated(mod, p)
        with np.errstate(divide="ignore"):
            _close(per_star[i], np.log(like), ("ln like_s", i))
        _close([lnl[i]], [R.lnlike_from_likes(like)], ("lnlike", i))
    return lnl


def _notebook_model(n_stars=50, seed=3, minq=0.5, **kw):
    ic = ia.synthetic_isochrone(bands=("g", "r", "i"))
    cat = ia.simulate_cluster(n_stars, *TRUTH_NB, bands="gri", ic=ic, seed=seed)
    df = cat.df[np.isfinite(cat.df[["g_mag", "r_mag", "i_mag"]].to_numpy()).all(axis=1)]
    return ia.StarClusterModel(ic, df, bands=["g", "r", "i"], props=["parallax"], eep_bounds=(200, 700), minq=minq, **kw)


@pytest.fixture(scope="module")
def notebook():
    return _notebook_model()


def test_notebook_shape_against_the_restatement(notebook):
    rng = np.random.default_rng(5)
    rows = np.array(TRUTH_NB) + np.array([0.02, 0.03, 5.0, 0.01, 0.2, 0.05, 0.05]) * rng.standard_normal((4, 7))
    lnl = _check_restated(notebook, rows)
    assert np.isfinite(lnl).all()
    assert isinstance(notebook.lnpost(np.array(TRUTH_NB)), float)


@pytest.fixture(scope="module")
def small():
    fx = R.load("cluster_jhk")
    return fx, R.make_ic(fx)


def _small_model(small, n_stars, bands=("J", "H", "K"), seed=0, eep_bounds=(151, 196), binary_fraction=0.3,
                 eep_range=(160.0, 192.0), **kw):
    fx, ic = small
    df = _stars(ic, np.random.default_rng(seed), n_stars, 9.0, -0.1, 400.0, 0.1, bands, eep_range, binary_fraction)
    return ia.StarClusterModel(ic, df, bands=list(bands), props=["parallax"], eep_bounds=eep_bounds, **kw)


ROWS = np.array([[9.0, -0.1, 400.0, 0.1, -2.5, 0.3, 0.3], [9.03, -0.05, 410.0, 0.12, -2.0, 0.4, 0.2]])


@pytest.mark.parametrize("n_stars,bands", [(1, ("J", "H", "K")), (2000, ("J", "H", "K")), (12, ("K",)),
                                           (12, ("J", "H", "K", "G", "BP", "RP", "V"))])
def test_shapes_against_the_restatement(small, n_stars, bands):
    mod = _small_model(small, n_stars, bands)
    lnl = _check_restated(mod, ROWS)
    assert np.isfinite(lnl).all()


def test_twelve_bands_and_two_k_blocks_against_the_restatement():
    bands = ia.grids.DEFAULT_BANDS + ("V",)
    assert len(bands) == 12
    ic = ia.synthetic_isochrone(bands=bands, ages=np.array([8.5, 9.0, 9.5]), fehs=np.array([-0.5, 0.0, 0.5]),
                                eeps=np.arange(140.0, 240.0), limits=dict(mass=(0.1, 300.0)))
    df = _stars(ic, np.random.default_rng(9), 20, 9.0, -0.1, 400.0, 0.1, bands, (180.0, 230.0))
    mod = ia.StarClusterModel(ic, df, bands=list(bands), props=["parallax"], eep_bounds=(141, 238), minq=0.1)
    lnl = _check_restated(mod, ROWS)
    assert np.isfinite(lnl[0])


def test_binary_fraction_edges_and_empty_rows(small):
    rows = ROWS.copy()
    rows[:, 6] = 0.0                                                        # no binaries: ln fB = -inf selects the single term
    assert np.isfinite(_check_restated(_small_model(small, 12, binary_fraction=0.0), rows)).all()
    rows[:, 6] = 1.0                                                        # only binaries: ln(1 - fB) = -inf
    both = _small_model(small, 12, binary_fraction=1.0, eep_range=(174.0, 192.0))   # secondaries inside the EEP range
    assert np.isfinite(_check_restated(both, rows)).all()
    mod = _small_model(small, 12)
    off = np.array([[7.0, -0.1, 400.0, 0.1, -2.5, 0.3, 0.3]])                # off the table: no valid EEP
    assert mod.lnlike(off)[0] == -np.inf and mod.lnpost(off[0]) == -np.inf
    one = _small_model(small, 12, eep_bounds=(180, 180))
    assert one.lnlike(ROWS[0]) == -np.inf                                   # a single EEP: like_s = 0
    _check_restated(_small_model(small, 12, eep_bounds=(180, 181)), ROWS[:1])


def test_rows_are_bitwise_independent_of_the_batch(notebook):
    import torch
    rng = np.random.default_rng(11)
    rows = np.array(TRUTH_NB) + np.array([0.05, 0.1, 20.0, 0.02, 0.3, 0.1, 0.1]) * rng.standard_normal((1024, 7))
    full = notebook.lnpost(rows)
    assert np.isfinite(full).sum() > 500
    again = notebook.lnpost(rows)
    rev = notebook.lnpost(rows[::-1].copy())[::-1]
    forced = ia.StarClusterModel(notebook.ic, notebook.stars, eep_bounds=(200, 700), minq=0.5, chunk_rows=100)
    chunked = forced.lnpost(rows)
    t = notebook.lnpost(torch.as_tensor(rows, device="cuda")).cpu().numpy()
    for other in (again, rev, chunked, t):
        assert np.array_equal(full.view(np.int64), other.view(np.int64))
    for i in (0, 1, 500, 1023):
        assert np.array_equal(np.array([notebook.lnpost(rows[i])]).view(np.int64), full[i:i + 1].view(np.int64))


@pytest.fixture(scope="module")
def fit_model():
    truth = [9.0, 0.0, 500.0, 0.1, -2.5, 0.3, 0.3]
    ic = ia.synthetic_isochrone(bands=("J", "H", "K"))
    cat = ia.simulate_cluster(30, *truth, bands="JHK", mass_range=(0.4, 1.1), ic=ic, seed=7)   # EEPs ~300-680 at 1 Gyr
    df = cat.df[np.isfinite(cat.df[["J_mag", "H_mag", "K_mag"]].to_numpy()).all(axis=1)]
    return truth, ic, df


def test_fit_multinest_recovers_the_truth(fit_model):
    truth, ic, df = fit_model
    mod = ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(200, 700), max_distance=2000)
    mod.fit_multinest(n_live_points=300, seed=3)
    s = mod.samples
    assert list(s.columns) == list(mod.param_names) + ["lnprob"]
    for i, name in enumerate(("age", "feh", "distance")):
        lo, hi = np.quantile(s[name], [0.025, 0.975])
        assert lo <= truth[i] <= hi, (name, lo, hi, truth[i])


def test_fit_mcmc_and_fit_dispatch(fit_model):
    truth, ic, df = fit_model
    mod = ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(200, 700), use_emcee=True)
    mod.fit(p0=truth, nwalkers=32, nburn=10, niter=20, seed=1)
    s = mod.samples
    assert len(s) == 32 * 20 and np.isfinite(s.to_numpy()).all()
    called = []
    nest = ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(200, 700))
    nest.fit_multinest = lambda **kw: called.append(kw)
    nest.fit(n_live_points=10)
    assert called == [dict(n_live_points=10)]


# -- the public path against columns from the CPU oracle and the long-double reference ---------------------------------
def _oracle_expected(mod, rows):
    """(lnlike [P], ln like_s [P][N_s]) without libiso_hip.so: each row's per-EEP columns from the CPU oracle's
    interpolators, compacted to the EEPs with a finite initial_mass as the model does, then the long-double reference."""
    ic = mod.ic
    oic = fx.make_oracle_ic(ic)
    ci = ic.model_grid.interp.column_index
    others = [q for q in mod.props if q != "parallax"]
    icols = [ci["initial_mass"], ci["dm_deep"]] + [ci[q] for q in others]
    bc = [ic.bc_grid.interp.column_index[b] for b in mod.bands]
    lo, hi = mod.bounds("eep")
    E = np.arange(lo, hi + 1).astype(float)
    mass_lo, mass_hi = mod.bounds("mass")
    nb, npr = len(mod.bands), len(mod.props)
    cols, rowpar, n_valid = [], [], []
    for p in rows:
        o = np.ones(E.size)
        v = oic.model.interp([p[0] * o, p[1] * o, E], icols)
        ok = np.isfinite(v[:, 0])
        Ek, ko = E[ok], o[ok]
        _, _, _, mags = oic.interp_mag(np.array([Ek, p[0] * ko, p[1] * ko, p[2] * ko, p[3] * ko]), bc)
        props = np.column_stack([1000.0 / p[2] * ko if q == "parallax" else v[ok, 2 + others.index(q)]
                                 for q in mod.props]) if npr else np.zeros((Ek.size, 0))
        c, rp = H.row_columns(Ek, v[ok, 0], np.log(np.abs(v[ok, 1])), mags, props, p[4], p[5], p[6], mod.minq, mass_lo,
                              mass_hi, E.size)
        cols.append(c)
        rowpar.append(rp)
        n_valid.append(Ek.size)
    meas = [mod.stars.measurements[b] for b in mod.bands] + [mod.stars.measurements[q] for q in mod.props]
    val = np.array([a for a, _ in meas], dtype=float)
    w = np.array([1.0 / (u * u) for _, u in meas], dtype=float)
    tot, ln = H.lnlike(np.array(cols), n_valid, np.array(rowpar), val, w, mod.minq, nb, npr)
    return tot.astype(float), ln.astype(float), np.array(n_valid)


def _check_oracle(mod, rows):
    lnl, per_star = mod.lnlike_stars(np.asarray(rows, dtype=float))
    tot, ln, n_valid = _oracle_expected(mod, rows)
    _close(per_star, ln, "ln like_s (oracle columns, long double)")
    _close(lnl, tot, "lnlike (oracle columns, long double)")
    return lnl, per_star, n_valid


def test_32_bands_and_8_props_against_oracle_columns():
    bands = tuple(list(ia.grids.KNOWN_BANDS) + ["X%02d" % j for j in range(32)])[:32]
    others = ("radius", "logTeff", "Teff", "logg", "logL", "Mbol", "density")
    ic = ia.synthetic_isochrone(bands=bands, ages=np.array([8.5, 9.0, 9.5]), fehs=np.array([-0.5, 0.0, 0.5]),
                                eeps=np.arange(140.0, 240.0), limits=dict(mass=(0.1, 300.0)))
    rng = np.random.default_rng(32)
    df = _stars(ic, rng, 20, 9.0, -0.1, 400.0, 0.1, bands, (180.0, 230.0))
    e = rng.uniform(180.0, 230.0, len(df))
    o = np.ones(len(df))
    truth = np.asarray(ic.interp_value([e, 9.0 * o, -0.1 * o], list(others)), dtype=float).reshape(len(df), len(others))
    for i, q in enumerate(others):
        unc = 0.05 * np.abs(truth[:, i]) + 0.05
        df[q] = truth[:, i] + unc * rng.standard_normal(len(df))
        df[q + "_unc"] = unc
    mod = ia.StarClusterModel(ic, df, bands=list(bands), props=["parallax"] + list(others), eep_bounds=(141, 238), minq=0.1)
    assert len(mod.bands) == 32 and len(mod.props) == 8
    lnl, per_star, n_valid = _check_oracle(mod, ROWS)
    assert np.all(n_valid > 64) and np.isfinite(per_star).sum() >= 20


def test_notebook_shape_against_oracle_columns(notebook):
    rows = np.array(TRUTH_NB) + np.array([[0.0] * 7, [0.02, 0.03, 5.0, 0.01, 0.2, 0.05, 0.05],
                                           [-0.02, -0.03, -5.0, 0.01, -0.2, -0.05, 0.05]])
    lnl, per_star, n_valid = _check_oracle(notebook, rows)
    assert np.isfinite(lnl).all() and np.all(n_valid > 256)
