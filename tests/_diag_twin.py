"""numpy twin of the chain diagnostics defined in include/isochrones_amd_diag.h: np.longdouble accumulators, direct sums,
no FFT.  Also the synthetic chains and the shape list the host-ABI and the GPU test share."""
import numpy as np

LD = np.longdouble
NOUT = 5
TAU, WINDOW, WINDOW_OK, ESS, RHAT = range(NOUT)


def tau_curve(x, max_lag=1024):
    """(tau(M) for M = 0..K, A(0)) of one slab x[T, W], in long double."""
    x = np.asarray(x, dtype=LD)
    T, W = x.shape
    K = min(T - 1, int(max_lag))
    y = x - x.sum(axis=0) / LD(T)                                   # two passes: the mean, then the centred series
    A = np.array([(y[: T - k] * y[k:]).sum() for k in range(K + 1)], dtype=LD)
    if A[0] == 0 or not np.isfinite(A[0]):
        return None, A[0]
    rho = A / A[0]
    return LD(1) + LD(2) * np.concatenate([[LD(0)], np.cumsum(rho[1:])]), A[0]


def split_rhat(x):
    x = np.asarray(x, dtype=LD)
    T, W = x.shape
    n = T // 2
    if T < 4:
        return np.nan
    ch = np.concatenate([x[:n], x[T - n:]], axis=1)                 # [n, 2 W]
    mu = ch.sum(axis=0) / LD(n)
    s2 = ((ch - mu) ** 2).sum(axis=0) / LD(n - 1)
    Wv = s2.sum() / LD(2 * W)
    if Wv == 0:
        return np.nan
    grand = mu.sum() / LD(2 * W)
    B = LD(n) * ((mu - grand) ** 2).sum() / LD(2 * W - 1)
    return float(np.sqrt((LD(n - 1) / LD(n) * Wv + B / LD(n)) / Wv))


def pair_diagnostics(x, c=5.0, max_lag=1024, margins=None):
    """The five numbers of one slab x[T, W].  ``margins`` (a list): appended with |M - c tau(M)| for every M <= M*, the
    distances of the window search's decisions from a tie."""
    x = np.asarray(x, dtype=np.float64)
    T, W = x.shape
    K = min(T - 1, int(max_lag))
    if not np.isfinite(x).all():                                    # Inf - Inf in the centring makes A(0) NaN as well
        return np.full(NOUT, np.nan)
    out = np.empty(NOUT)
    out[RHAT] = split_rhat(x)
    curve, a0 = tau_curve(x, max_lag)
    if curve is None:
        out[[TAU, ESS]] = np.nan
        out[WINDOW], out[WINDOW_OK] = K, 0.0
        return out
    hit = np.nonzero(np.arange(K + 1) >= LD(c) * curve)[0]
    M = int(hit[0]) if hit.size else K
    if margins is not None:
        margins.extend(float(abs(LD(m) - LD(c) * curve[m])) for m in range(M + 1))
    tau = curve[M]
    out[TAU], out[WINDOW], out[WINDOW_OK] = float(tau), M, float(hit.size > 0)
    out[ESS] = float(LD(W) * LD(T) / tau)
    return out


def storage_diagnostics(storage, n_ens, W, c=5.0, max_lag=1024, margins=None):
    """[S, D, 5] for parameter-major storage [T, D, n_ens * W]."""
    T, D, R = storage.shape
    assert R == n_ens * W
    out = np.empty((n_ens, D, NOUT))
    for s in range(n_ens):
        for d in range(D):
            out[s, d] = pair_diagnostics(storage[:, d, s * W:(s + 1) * W], c, max_lag, margins)
    return out


def ar1(rng, T, W, phi, mean=0.0, scale=1.0):
    """x[T, W]: W independent stationary AR(1) series with coefficient phi and marginal spread `scale` about `mean`."""
    e = rng.standard_normal((T, W))
    x = np.empty((T, W))
    x[0] = e[0]
    for t in range(1, T):
        x[t] = phi * x[t - 1] + np.sqrt(1.0 - phi * phi) * e[t]
    return mean + scale * x


#: (name, S, D, W, T, max_lag): the smallest shapes at which the kernel can go wrong.  tile_plan() below says which tile
#: size and LDS path a shape gets; PLANS pins that for the shapes chosen for it.
SHAPES = (
    ("plain", 3, 2, 64, 16, 1024),
    ("reference", 2, 5, 300, 100, 1024),          # W no multiple of 64, slab larger than LDS, K = 99 beyond one wavefront
    ("odd_T", 1, 1, 34, 7, 1024),                 # split R-hat drops the middle step, W below a wavefront
    ("smallest_rhat", 2, 3, 2, 4, 1024),
    ("max_lag_binds", 1, 2, 70, 300, 32),         # parameter 1 is too slow for a window inside 32 lags
    ("rhat_nan", 1, 1, 8, 3, 1024),
    ("edge_pairs", 1, 4, 40, 60, 1024),           # one stuck walker / all constant / mean 1e3 spread 1e-2 / a NaN
    ("two_quads", 1, 3, 8, 600, 400),             # K + 1 = 401: quad 1 has 145 lags, three per lane; one tile of 8
    ("uneven_tiles", 1, 3, 21, 1200, 330),        # tiles of 5, 5, 5, 5, 1 (w0 = 5, 10, 15 are no multiple of 4); quad 1 has
                                                  # 75 lags: two per lane, the upper ones masked by max_lag
    ("large_lds", 1, 3, 8, 1500, 1024),           # two walkers fit 64 KB: the > 64 KB launch, tiles of 4; five quads, four
                                                  # lags per lane in four of them, one live lane in the last
    ("max_lag_mid_lane", 1, 3, 5, 700, 355),      # K + 1 = 356: quad 1 has 100 lags, lanes 36..63 sum a lag they drop
    ("near_limit", 1, 2, 1, 16000, 1024),         # one walker, 160 856 of the 163 840 bytes a CU has
    ("one_walker", 2, 2, 1, 50, 1024),            # walker groups 1..3 are empty, R-hat from two split chains
    ("single_step", 2, 2, 3, 1, 1024),            # K = 0 and A(0) = 0: tau, ess and rhat NaN, window 0, window_ok 0
    ("nonfinite", 1, 3, 12, 20, 1024),            # +Inf in parameter 0, -Inf in parameter 1, parameter 2 finite
)
#: the shapes with lags beyond the first quad of 256; tests also evaluate them with OPEN_C, a window factor so large that
#: the slowest parameter's window never closes: tau only sums rho(1..M*), so a wrong A(k) beyond M* changes no output,
#: and with M* = K every lag sum of the kernel enters tau
LONG_SHAPES = ("two_quads", "uneven_tiles", "large_lds", "max_lag_mid_lane", "near_limit")
OPEN_C = 1000.0
#: AR(1) coefficients of parameter 1 (window inside the lags at c = 5, beyond the first quad for most) and parameter 2
#: (too slow for any window)
LONG_PHI = {"two_quads": (0.97, 0.9995), "uneven_tiles": (0.97, 0.9995), "large_lds": (0.985, 0.9995),
            "max_lag_mid_lane": (0.97, 0.9995), "near_limit": (0.9995,)}
#: name -> (WT, LDS bytes, whether the launch asks for more than 64 KB), worked out by hand from the selection in
#: iso_diag_chain; test_diag_host_abi_cpu.py asserts that tile_plan() still says so
PLANS = {"two_quads": (8, 51680, False), "uneven_tiles": (5, 59384, False), "large_lds": (4, 81152, True),
         "max_lag_mid_lane": (5, 39672, False), "near_limit": (1, 160856, True)}
#: seeds for which no decision of any pair's window search is within 1e-6 of a tie, and for which no pair's window closes
#: only at M = T - 1: tau(T - 1) is identically zero (the autocovariances of a centred series sum to -A(0)/2 over all
#: lags), so a value there is rounding noise and a relative tolerance says nothing about it.  check_fixture asserts both.
SEEDS = {"plain": 11, "reference": 12, "odd_T": 13, "smallest_rhat": 33, "max_lag_binds": 15, "rhat_nan": 17,
         "edge_pairs": 17, "two_quads": 41, "uneven_tiles": 41, "large_lds": 41, "max_lag_mid_lane": 41, "near_limit": 41,
         "one_walker": 41, "single_step": 41, "nonfinite": 41}

TILE_WALKERS, GROUPS, LDS_PLAIN, LDS_LIMIT = 16, 4, 64 * 1024, 160 * 1024


def tile_plan(W, T, max_lag):
    """(WT, LDS bytes, big) as iso_diag_chain selects them: the arithmetic of its tile selection replayed, nothing else.
    ``big``: the launch asks for more than the 64 KB every launch gets.  ValueError where the library refuses."""
    K, Tp = min(T - 1, int(max_lag)), T | 1

    def nbytes(wt):
        return 8 * (GROUPS * (K + 1) + 4 * W + 2 * wt + wt * Tp)
    if T > LDS_LIMIT // 8:
        raise ValueError("nsteps too large")
    wt = min(W, TILE_WALKERS)
    while wt > 1 and nbytes(wt) > LDS_PLAIN:
        wt -= 1
    if nbytes(wt) > LDS_PLAIN or (wt < GROUPS and wt < W):
        wt = min(W, GROUPS)
        while wt > 1 and nbytes(wt) > LDS_LIMIT:
            wt -= 1
    if nbytes(wt) > LDS_LIMIT:
        raise ValueError("%d bytes of LDS exceed a CU's 160 KB" % nbytes(wt))
    return wt, nbytes(wt), nbytes(wt) > LDS_PLAIN


def make_storage(name):
    """Parameter-major storage [T, D, S * W] of the named shape, written pair by pair, and its (S, D, W, T, max_lag)."""
    _, S, D, W, T, max_lag = next(sh for sh in SHAPES if sh[0] == name)
    rng = np.random.default_rng(SEEDS[name])
    st = np.empty((T, D, S * W))
    for s in range(S):
        for d in range(D):
            phi = (0.3, 0.6, 0.8, 0.0, 0.5)[(s + d) % 5]
            st[:, d, s * W:(s + 1) * W] = ar1(rng, T, W, phi, mean=float(d), scale=1.0 + s)
    if name == "max_lag_binds":
        st[:, 1, :] = ar1(rng, T, W, 0.995)
    if name == "edge_pairs":
        st[:, 0, 5] = st[0, 0, 5]                                   # a single walker held constant
        st[:, 1, :] = st[0, 1, :]                                   # every walker constant
        st[:, 2, :] = ar1(rng, T, W, 0.4, mean=1e3, scale=1e-2)     # the distance column's scale
        st[T // 2, 3, 7] = np.nan
    for d, phi in enumerate(LONG_PHI.get(name, ()), start=1):
        st[:, d, :] = ar1(rng, T, W, phi)
    if name == "nonfinite":
        st[T // 2, 0, 7] = np.inf                                   # in the middle of a series
        st[0, 1, 3] = -np.inf                                       # the value the mean is taken about
    return st, (S, D, W, T, max_lag)


def check_fixture(want, T, margins):
    """The fixture's own conditions: every window decision at least 1e-6 from a tie, no finite tau taken at M = T - 1."""
    assert all(m > 1e-6 for m in margins), min(margins)
    fin = np.isfinite(want[..., TAU])
    assert (want[..., WINDOW][fin] < T - 1).all()


_CACHE = {}


def fixture(name):
    """(storage, (S, D, W, T, max_lag), twin result [S, D, 5]) of a named shape; computed once, shared, not to be changed."""
    if name not in _CACHE:
        st, dims = make_storage(name)
        margins = []
        want = storage_diagnostics(st, dims[0], dims[2], 5.0, dims[4], margins)
        check_fixture(want, dims[3], margins)
        st.setflags(write=False)
        want.setflags(write=False)
        _CACHE[name] = (st, dims, want)
    return _CACHE[name]


def open_window(name):
    """(storage, dims, twin result at c = OPEN_C) of a long shape: the fixture's storage with the window factor that keeps the
    last parameter's window open.  Both conditions are asserted on the twin alone, before anything is compared with it."""
    key = (name, OPEN_C)
    if key not in _CACHE:
        st, dims, _ = fixture(name)
        S, D, W, T, max_lag = dims
        margins = []
        want = storage_diagnostics(st, S, W, OPEN_C, max_lag, margins)
        K = min(T - 1, max_lag)
        assert (want[:, -1, WINDOW] == K).all() and (want[:, -1, WINDOW_OK] == 0).all(), want[:, -1]
        check_fixture(want, T, margins)
        want.setflags(write=False)
        _CACHE[key] = (st, dims, want)
    return _CACHE[key]


def assert_matches(got, want, rtol=1e-9):
    """tau, ess and rhat within rtol relative; window and window_ok exactly; NaN where the twin has NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    for i in (WINDOW, WINDOW_OK):
        assert np.array_equal(got[..., i], want[..., i], equal_nan=True), (i, got[..., i], want[..., i])
    for i in (TAU, ESS, RHAT):
        g, w = got[..., i], want[..., i]
        ok = ~np.isnan(w)
        rel = np.abs(g[ok] - w[ok]) / np.abs(w[ok])
        print("column %d: max relative difference %.3g" % (i, rel.max() if rel.size else 0.0))
        assert (rel <= rtol).all(), (i, rel.max())
