"""The numpy twin of the chain diagnostics (tests/_diag_twin.py) against series whose answers are known."""
import numpy as np

from tests import _diag_twin as tw


def test_ar1_tau_is_near_the_analytic_value():
    """AR(1) with phi = 0.5 has tau = (1 + phi) / (1 - phi) = 3.  W = 64, T = 4000, seed 0: the twin gives 3.0219.
    Measured once over the seeds 0..7: mean 3.0002, sample standard deviation 0.0218, largest |tau - 3| 0.032.  The
    margin is five of those standard deviations, 0.11."""
    r = tw.pair_diagnostics(tw.ar1(np.random.default_rng(0), 4000, 64, 0.5))
    print("tau %.6f window %d" % (r[tw.TAU], r[tw.WINDOW]))
    assert abs(r[tw.TAU] - 3.0) < 5 * 0.0218
    assert r[tw.WINDOW_OK] == 1.0 and r[tw.WINDOW] >= 5 * r[tw.TAU]
    assert abs(r[tw.ESS] - 64 * 4000 / r[tw.TAU]) < 1e-6
    assert abs(r[tw.RHAT] - 1.0) < 0.01


def test_iid_draws_have_tau_and_rhat_near_one():
    """W T = 64 000 independent draws: rho(k) scatters by 1 / sqrt(W T) = 0.004 per lag and the window closes after
    about five lags, so tau scatters by about 2 sqrt(5) 0.004 = 0.018 around 1; 0.1 is five of those."""
    r = tw.pair_diagnostics(np.random.default_rng(1).standard_normal((1000, 64)))
    assert abs(r[tw.TAU] - 1.0) < 0.1 and r[tw.WINDOW_OK] == 1.0
    assert abs(r[tw.RHAT] - 1.0) < 0.01


def test_shifted_halves_raise_rhat():
    """Second half moved by three standard deviations: B / n = var of means = about 2.25 + ..., so R-hat is near
    sqrt(1 + 2.25) = 1.8."""
    x = np.random.default_rng(2).standard_normal((400, 16))
    x[200:] += 3.0
    r = tw.pair_diagnostics(x)
    assert r[tw.RHAT] > 1.5
    assert abs(tw.pair_diagnostics(x[:200])[tw.RHAT] - 1.0) < 0.05


def test_degenerate_slabs():
    K = 9
    const = np.full((10, 4), 2.5)
    r = tw.pair_diagnostics(const)
    assert np.isnan(r[[tw.TAU, tw.ESS, tw.RHAT]]).all() and r[tw.WINDOW] == K and r[tw.WINDOW_OK] == 0.0
    x = np.random.default_rng(3).standard_normal((10, 4))
    assert np.isnan(tw.pair_diagnostics(x[:3])[tw.RHAT]) and np.isfinite(tw.pair_diagnostics(x[:4])[tw.RHAT])
    x[4, 2] = np.nan
    assert np.isnan(tw.pair_diagnostics(x)).all()


def test_every_shared_fixture_meets_its_own_conditions():
    for name, S, D, W, T, max_lag in tw.SHAPES:
        st, dims, want = tw.fixture(name)
        assert st.shape == (T, D, S * W) and want.shape == (S, D, tw.NOUT)
    slow = tw.fixture("max_lag_binds")[2]
    assert slow[0, 1, tw.WINDOW_OK] == 0.0 and slow[0, 1, tw.WINDOW] == 32 and slow[0, 0, tw.WINDOW_OK] == 1.0
    edge = tw.fixture("edge_pairs")[2]
    assert np.isfinite(edge[0, 0]).all() and np.isfinite(edge[0, 2]).all()
    assert np.isnan(edge[0, 1, tw.TAU]) and edge[0, 1, tw.WINDOW_OK] == 0.0 and np.isnan(edge[0, 3]).all()
    assert np.isnan(tw.fixture("rhat_nan")[2][0, 0, tw.RHAT]) and np.isfinite(tw.fixture("rhat_nan")[2][0, 0, tw.TAU])
