"""libiso_emfit.so's host entries through ctypes, no GPU needed: iso_emfit_run_host against the long-double twin of
tests/_emfit_twin.py after 1, 2 and 7 steps (g within 1e-11 absolute, the objective within 1e-11 relative to max(1, sum w
|ln s1|)), a non-decreasing Q, the three ways a replicate stops, every refusal with its message, the inputs that have to
give the same bits, and iso_emfit_weights_host: the Poisson counts against the twin on the oracle's Philox, their
thresholds against a 40-digit evaluation, their mean and variance, and -log(u) against the exponential distribution."""
import math
import os
import re

import numpy as np
import pytest

from isochrones_amd import _emfit_cabi as ec
from isochrones_amd.csrc.libraries import EMFIT
from oracle.cpu_sampler import philox_kat
from tests import _emfit_twin as et

LD = et.LD
NINF = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    EMFIT.build()
    return ec.lib()


def _err(lib):
    return lib.iso_emfit_last_error().decode()


@pytest.mark.parametrize("steps", [1, 2, 7])
@pytest.mark.parametrize("S, B, R", [(1, 1, 1), (7, 2, 3), (300, 12, 3), (257, 63, 2), (64, 64, 1), (513, 17, 3)])
def test_host_entry_matches_the_twin(lib, S, B, R, steps):
    c = et.case(S, B, R)
    rc, out = et.call(lib, max_iter=steps, tol=NINF, **c)
    assert rc == 0, _err(lib)
    ref = et.run(max_iter=steps, tol=NINF, **c)
    worst = et.assert_matches(out, ref)
    print("S = %d, B = %d, R = %d, %d steps: worst error / limit = %.2e, status %s" % (S, B, R, steps, worst, out["status"]))
    live = out["status"] != ec.EMPTY
    assert (out["n_iter"][live] == steps).all() and (out["status"][live] == ec.MAX_ITER).all()
    assert (out["n_iter"][~live] == 0).all() and (out["n_live"][~live] == 0).all()
    if S > 3 and R >= 2:
        assert out["status"][R - 1] == ec.EMPTY and np.array_equal(out["g"][R - 1], c["g0"][R - 1])
        assert out["objective"][R - 1] == 0.0 and out["wsum"][R - 1] == 0.0
    assert np.all(np.abs(out["g"][live].sum(axis=1) - 1.0) <= 1e-13)
    if B > 2 and S > 3:
        assert (out["g"][live][:, 1] == 0.0).all() and (out["g"][live][:, B - 1] == 0.0).all()   # closed, and started at 0


@pytest.mark.parametrize("S, B", [(300, 12), (64, 64), (513, 5)])
def test_the_objective_never_falls(lib, S, B):
    """Q_0 <= Q_1 <= ... <= Q_7 but for rounding: the slack is 1e-11 max(1, sum w |ln s1|) with the twin's sum, the limit the
    objective itself is held to."""
    c = et.case(S, B, 2, seed=3, hard=False)
    ref = et.run(max_iter=7, tol=NINF, **c)
    Q = []
    for k in range(8):
        rc, out = et.call(lib, max_iter=k, tol=NINF, **c)
        assert rc == 0 and (out["n_iter"] == k).all()
        Q.append(out["objective"])
    Q = np.array(Q)                                                     # [step, replicate]
    slack = et.LIMIT * np.maximum(1.0, ref["absln"].astype(np.float64))
    assert np.all(np.diff(Q, axis=0) >= -slack[None, :])
    assert np.all(Q[-1] - Q[0] > 100 * slack)                           # and it does rise
    for r in range(2):
        assert np.all(np.abs(Q[:, r] - np.array(ref["trace"][r], dtype=np.float64)) <= slack[r])


def test_converged_max_iter_and_empty(lib):
    S, B = 400, 4
    c = et.case(S, B, 3, seed=1, hard=False)
    c["w"][:2] += 1.0                                                   # everybody is live in replicates 0 and 1
    c["w"][2] = 0.0                                                     # nobody is live in replicate 2
    # every star in one cell: the first step lands on the maximum and the second rise is 0
    c["A"][1:, :] = 0.0
    c["A"][0, :] = 1.0
    rc, out = et.call(lib, max_iter=50, tol=1e-8, **c)
    assert rc == 0, _err(lib)
    assert list(out["status"]) == [ec.CONVERGED, ec.CONVERGED, ec.EMPTY]
    assert list(out["n_iter"]) == [2, 2, 0] and list(out["n_live"][:2]) == [S, S] and out["n_live"][2] == 0
    assert np.array_equal(out["g"][:2], [[1.0, 0, 0, 0]] * 2)
    # a slow case stops at max_iter, and with tol = -inf whatever the rise
    c = et.case(300, 12, 2, seed=2, hard=False)
    rc, out = et.call(lib, max_iter=3, tol=1e-8, **c)
    assert rc == 0 and list(out["status"]) == [ec.MAX_ITER] * 2 and list(out["n_iter"]) == [3, 3]
    rc, zero = et.call(lib, max_iter=0, tol=1e-8, **c)
    assert rc == 0 and list(zero["status"]) == [ec.MAX_ITER] * 2 and np.array_equal(zero["g"], c["g0"])
    # the same case converges given the steps, in agreement with the twin
    rc, out = et.call(lib, max_iter=5000, tol=1e-8, **c)
    ref = et.run(max_iter=5000, tol=1e-8, **c)
    assert rc == 0 and list(out["status"]) == [ec.CONVERGED] * 2 and (out["n_iter"] < 5000).all()
    assert np.all(np.abs(out["n_iter"] - ref["n_iter"]) <= 1), (out["n_iter"], ref["n_iter"])
    # a tol of +inf stops after the first step
    rc, out = et.call(lib, max_iter=9, tol=np.inf, **c)
    assert rc == 0 and list(out["status"]) == [ec.CONVERGED] * 2 and list(out["n_iter"]) == [1, 1]


def test_refusals(lib):
    c = et.case(5, 3, 2, hard=False)
    A, scale, w, g0 = c["A"], c["scale"], c["w"], c["g0"]

    def refused(word, **over):
        rc, _ = et.call(lib, **dict(c, **over))
        assert rc == ec.ERR_INVALID and word in _err(lib) and "iso_emfit_run_host" in _err(lib), (over, _err(lib))

    for bad in (-1.0, np.nan, np.inf):
        s = scale.copy()
        s[1] = bad
        refused("scale", scale=s)
        x = w.copy()
        x[1, 2] = bad
        refused("w must", w=x)
        x = g0.copy()
        x[1, 0] = bad
        refused("g0 must", g0=x)
        refused("g0 must", g0=x[1])
    z = g0.copy()
    z[1] = 0.0
    refused("sum to something above 0", g0=z)
    refused("max_iter", max_iter=-1)
    refused("tol", tol=np.nan)
    refused("steps_per_launch", steps=-1)
    g, q, i32 = np.zeros((2, 3)), np.zeros(2), np.zeros(2, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    fn = lib.iso_emfit_run_host
    good = [p(A), 3, 5, p(scale), p(w), 2, None, p(g0), 3, 1, 0.0, 0, p(g), p(q), p(i32), p(i32), p(i32), p(q), None]
    for at, value, word in ((1, 0, "B must be"), (1, 65, "B must be"), (2, 0, "n_ens"), (5, 0, "R must be"),
                            (8, 2, "g0_stride"), (8, -3, "g0_stride"), (0, None, "null"), (3, None, "null"), (7, None, "null"),
                            (12, None, "null"), (13, None, "null"), (14, None, "null"), (15, None, "null"), (16, None, "null"),
                            (17, None, "null")):
        args = list(good)
        args[at] = value
        assert fn(*args) == ec.ERR_INVALID and word in _err(lib), (at, _err(lib))
        assert lib.iso_emfit_run(*args) == ec.ERR_INVALID and word in _err(lib) and "iso_emfit_run:" in _err(lib)
    assert fn(*good) == 0 and _err(lib) == ""
    out = np.zeros(10)
    wf = lib.iso_emfit_weights_host
    for args, word in (((2, 0, 0, 2, 5, p(out), None), "kind"), ((0, 0, -1, 2, 5, p(out), None), "first_replicate"),
                       ((0, 0, 0, 0, 5, p(out), None), "R must be"), ((0, 0, 0, 2, 0, p(out), None), "n_ens"),
                       ((0, 0, 0, 2, 5, None, None), "null"), ((0, 0, 2 ** 31 - 2, 2, 5, p(out), None), "2^31")):
        assert wf(*args) == ec.ERR_INVALID and word in _err(lib) and "iso_emfit_weights_host" in _err(lib), (args, _err(lib))
        assert lib.iso_emfit_weights(*args) == ec.ERR_INVALID and word in _err(lib)
    assert wf(0, 0, 0, 2, 5, p(out), None) == 0 and _err(lib) == ""


def test_inputs_that_give_the_same_bits(lib):
    c = et.case(300, 12, 3, seed=5, hard=False)
    run = lambda **over: et.call(lib, max_iter=7, tol=NINF, **dict(c, **over))[1]
    # a masked star and a weight of 0
    mask = np.ones(300, np.int32)
    mask[[4, 170]] = 0
    w0 = c["w"].copy()
    w0[:, [4, 170]] = 0.0
    assert et.same_bits(run(mask=mask), run(w=w0))
    # w = NULL and all ones
    assert et.same_bits(run(w=None, R=3), run(w=np.ones((3, 300))))
    # a shared g0 and the same row repeated
    row = c["g0"][1]
    assert et.same_bits(run(g0=row), run(g0=np.tile(row, (3, 1))))
    # a replicate alone and in the batch
    whole = run()
    one = run(w=c["w"][1:2], g0=c["g0"][1:2])
    assert all(one[k].tobytes() == whole[k][1:2].tobytes() for k in one)
    # steps_per_launch says nothing to the host entry, and seven calls of one step chained through g0 are seven steps
    assert et.same_bits(whole, run(steps=3))
    g = c["g0"]
    for _ in range(7):
        g = et.call(lib, max_iter=1, tol=NINF, **dict(c, g0=g))[1]["g"]
    assert g.tobytes() == whole["g"].tobytes()


# -- the weights ------------------------------------------------------------------------------------------------------
def test_poisson_thresholds_are_the_cumulative_probabilities():
    """The header's hexadecimal literals against e^-1 sum_{j <= k} 1 / j! evaluated with 40 digits: within one ulp (they are
    the correctly rounded doubles), increasing, below 1, and the next one would round to 1."""
    import mpmath
    text = open(os.path.join(ROOT, "include", "isochrones_amd_emfit.h")).read()
    body = text.split("#define ISO_EMFIT_POISSON_CDF")[1].split("\n\n")[0]
    c = [float.fromhex(x) for x in re.findall(r"0x1\.[0-9a-f]+p-\d+", body)]
    assert len(c) == ec.POISSON_TERMS == 18
    want = et.poisson_cdf(40)
    for k, (got, w) in enumerate(zip(c, want)):
        ulp = math.ulp(got)
        assert abs(mpmath.mpf(got) - w) <= ulp, (k, got)
        assert got == float(w)
    assert all(a < b for a, b in zip(c, c[1:])) and c[-1] == 1.0 - 2.0 ** -53 < 1.0
    with mpmath.workdps(40):
        assert float(want[-1] + mpmath.exp(-1) / mpmath.factorial(18)) == 1.0


def test_poisson_counts_equal_the_twin(lib):
    philox_kat()
    for seed, first, R, S in ((0, 0, 1, 1), (7, 0, 3, 257), (2 ** 63 + 12345, 5, 2, 1000), (1, 2 ** 31 - 3, 2, 9)):
        rc, got = et.call_weights(lib, ec.POISSON, seed, first, R, S)
        assert rc == 0, _err(lib)
        assert np.array_equal(got, et.weights(ec.POISSON, seed, first, R, S)), (seed, first)
        assert np.array_equal(got, np.round(got)) and got.min() >= 0 and got.max() <= 18
    # a weight depends on (seed, replicate, star) alone
    rc, whole = et.call_weights(lib, ec.POISSON, 11, 0, 6, 300)
    rc2, part = et.call_weights(lib, ec.POISSON, 11, 2, 4, 300)
    rc3, short = et.call_weights(lib, ec.POISSON, 11, 2, 4, 120)
    assert rc == rc2 == rc3 == 0 and np.array_equal(part, whole[2:]) and np.array_equal(short, whole[2:, :120])
    rc, other = et.call_weights(lib, ec.POISSON, 12, 0, 6, 300)
    assert rc == 0 and not np.array_equal(other, whole)


def test_poisson_mean_and_variance(lib):
    """10^5 counts: the mean within 5 / sqrt(n) of 1 (a Poisson(1) count has variance 1) and the sample variance within
    5 sqrt(3 / n) of 1 (its variance is (mu_4 - sigma^4) / n with mu_4 = 3 lambda^2 + lambda = 4)."""
    n = 100_000
    rc, k = et.call_weights(lib, ec.POISSON, 2024, 0, 100, n // 100)
    assert rc == 0
    k = k.reshape(-1)
    mean, var = k.mean(), k.var(ddof=1)
    print("Poisson counts: mean %.5f, variance %.5f, max %d" % (mean, var, k.max()))
    assert abs(mean - 1.0) <= 5.0 / math.sqrt(n) and abs(var - 1.0) <= 5.0 * math.sqrt(3.0 / n)
    freq = np.bincount(k.astype(int), minlength=4)[:4] / n
    want = math.exp(-1) * np.array([1, 1, 0.5, 1 / 6])
    assert np.all(np.abs(freq - want) <= 5.0 * np.sqrt(want * (1 - want) / n))


KS_BOUND = 1.95                                                     # the 0.1 % point of sqrt(n) * D, as in the draw tests
KS_SEED = 1


def _ks_exponential(x):
    x = np.sort(x)
    n = x.size
    F = -np.expm1(-x)
    i = np.arange(1, n + 1)
    return math.sqrt(n) * max(np.max(i / n - F), np.max(F - (i - 1) / n))


def test_the_ks_seed_passes_on_the_twin():
    """The seed was fixed once; a correct sampler fails a given seed once in a thousand."""
    x = et.weights(ec.EXP, KS_SEED, 0, 100, 1000).astype(np.float64).reshape(-1)
    assert _ks_exponential(x) < KS_BOUND


def test_exponential_weights(lib):
    rc, x = et.call_weights(lib, ec.EXP, KS_SEED, 0, 100, 1000)
    assert rc == 0, _err(lib)
    want = et.weights(ec.EXP, KS_SEED, 0, 100, 1000)
    assert np.all(np.abs(x - want) <= 1e-14 * np.abs(want)) and (x > 0).all() and np.isfinite(x).all()
    d = _ks_exponential(x.reshape(-1))
    print("-log(u): sqrt(n) D = %.3f (bound %.2f), mean %.5f" % (d, KS_BOUND, x.mean()))
    assert d < KS_BOUND
    rc, part = et.call_weights(lib, ec.EXP, KS_SEED, 2, 3, 1000)
    assert rc == 0 and np.array_equal(part, x[2:5])
