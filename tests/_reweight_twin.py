"""A long-double numpy statement of include/isochrones_amd_reweight.h (the population-informed per-star posteriors of
libiso_reweight.so), the cases its host and device tests share, and the one way they call the library.

The twin evaluates the family records through tests/_hier_twin.lnf in numpy's long double (64-bit mantissa), adds the rows'
terms in ascending order, sorts stably and takes a long-double cumulative sum.  The limits are those of tests/_hier_twin.py
and tests/_select_twin.py, derived the same way:

* weights: |du| <= 1e-11 * max(1, max |r - ln_norm| / 100) * u.  (r - ln_norm carries a few ulp of its size, 5e-14 at 100,
  which exp turns into that relative error of t_h; the H <= 1024 non-negative terms add H * 2^-53 = 1.1e-13 at the very
  worst; below 1e-12, so the limit leaves a factor ten.  A weight below 1e-300 is compared absolutely: subnormal results
  keep no relative precision and an underflow to 0 is the right answer.)
* wsum, ess: 1e-10 relative; mean, sd: 1e-10 of the column's scale max |y| (finite samples).  (M <= 3200 terms of weights
  good to 1e-11 and M * 2^-53 = 3.6e-13 of summation at the very worst.)
* quantiles: the twin's sample value exactly.  A case must have no near tie: |C(y_(j)) - p * tot| <= 1e-9 * tot at the
  chosen or the preceding sorted sample (``near_tie``); `assert_matches` asserts that of the case itself.  Cases made to tie
  have integer weights, for which every sum is exact (``exact``: no near-tie test)."""
import ctypes as C

import numpy as np

from isochrones_amd import _cabi, _hier_cabi as hc, _reweight_cabi as rc, hierarchical as hi, priors as P
from tests import _hier_twin as ht

LD = np.longdouble
PROBS3 = np.array([0.5, 0.16, 0.84])
PROBS8 = np.array([0.5, 0.16, 0.84, 0.025, 0.975, 0.31, 0.003, 0.69])


# -- the definition -------------------------------------------------------------------------------------------------------
def weights(x, interim, rows, ln_norm, mask=None):
    """``x`` [Q, S, M] float64, ``interim`` [Q], ``rows`` [H, Q] records, ``ln_norm`` [H, S] -> ``u`` [S, M] (long double; NaN
    rows for a masked star), ``n_bad`` [S], ``dmax`` [S] (max |r - ln_norm| over the finite ones of the good samples)."""
    Q, S, M = x.shape
    H = rows.shape[0]
    u, n_bad, dmax = np.zeros((S, M), LD), np.zeros(S, np.int32), np.zeros(S)
    with np.errstate(all="ignore"):
        for s in range(S):
            if mask is not None and not mask[s]:
                u[s] = np.nan
                continue
            l0 = [ht.lnf(interim[q], x[q, s]) for q in range(Q)]
            good = np.ones(M, bool)
            for q in range(Q):
                good &= ~np.isnan(x[q, s]) & ~np.isnan(l0[q]) & (l0[q] != -np.inf)
            n_bad[s] = M - good.sum()
            for h in range(H):
                ln = ln_norm[h, s]
                if np.isnan(ln) or ln == -np.inf:
                    continue
                r = np.zeros(M, LD)
                for q in range(Q):
                    lf = ht.lnf(rows[h, q], x[q, s])
                    lf = np.where(np.isnan(lf), LD(-np.inf), lf)
                    r = lf - l0[q] if q == 0 else r + (lf - l0[q])
                d = r - LD(ln)
                fin = np.abs(d[good & np.isfinite(d)])
                dmax[s] = max(dmax[s], float(fin.max()) if fin.size else 0.0)
                u[s] = u[s] + np.where(good, np.exp(d), LD(0))
            u[s] = np.where(good, u[s], LD(0))
    return u, n_bad, dmax


def summary(u, y, probs):
    """One (star, value column): ``u`` [M] long double, ``y`` [M] float64 -> (mean, sd, quant [K], n_nan, near_tie [K])."""
    K = len(probs)
    nan = np.isnan(y)
    uu = np.where(nan, LD(0), u)
    yy = np.where(nan, 0.0, y + 0.0).astype(LD)
    tot = uu.sum()
    if not tot > 0:
        return np.nan, np.nan, np.full(K, np.nan), int(nan.sum()), np.zeros(K, bool)
    with np.errstate(all="ignore"):
        mean = (uu * yy).sum() / tot
        sd = np.sqrt((uu * (yy - mean) ** 2).sum() / tot)
    keep = np.flatnonzero(uu > 0)
    order = keep[np.argsort(yy[keep].astype(np.float64), kind="stable")]
    ys = yy[order].astype(np.float64)
    cum = np.cumsum(uu[order])                                       # sequential, long double
    ends = np.flatnonzero(np.append(ys[1:] != ys[:-1], True))       # the last sample of every group of equal values
    quant, near = np.empty(K), np.zeros(K, bool)
    for k, p in enumerate(probs):
        target = LD(p) * tot
        hit = np.flatnonzero(cum[ends] >= target)
        g = hit[0] if hit.size else len(ends) - 1
        quant[k] = ys[ends[g]]
        look = cum[ends[max(g - 1, 0):g + 1]]
        near[k] = bool(np.any(np.abs(look - target) <= LD(1e-9) * tot))
    return float(mean), float(sd), quant, int(nan.sum()), near


def values_of(case):
    """The value columns of a case as [V, S, M] float64: ("x", q) is model column q, ("y", v) the case's own column v."""
    return np.stack([case["x"][i] if kind == "x" else case["y"][i] for kind, i in case["values"]])


def reweight(case, ln_norm=None, probs=None):
    """The whole definition for a case: dict of float64 / int arrays ``weights`` [S, M], ``wsum``, ``ess``, ``n_bad`` [S],
    ``mean``, ``sd``, ``n_nan`` [S, V], ``quant`` [S, V, K], and the twin's own ``dmax`` [S], ``near_tie`` [S, V, K], ``scale``
    [S, V]."""
    ln_norm = ell(case) if ln_norm is None else ln_norm
    probs = case["probs"] if probs is None else probs
    u, n_bad, dmax = weights(case["x"], case["interim"], case["rows"], ln_norm, case["mask"])
    yv = values_of(case)
    V, S, M = yv.shape
    K = len(probs)
    out = dict(weights=u.astype(np.float64), n_bad=n_bad, dmax=dmax, wsum=np.empty(S), ess=np.empty(S), mean=np.empty((S, V)),
               sd=np.empty((S, V)), n_nan=np.zeros((S, V), np.int32), quant=np.empty((S, V, K)),
               near_tie=np.zeros((S, V, K), bool), scale=np.ones((S, V)))
    for s in range(S):
        if case["mask"] is not None and not case["mask"][s]:
            out["wsum"][s] = out["ess"][s] = out["mean"][s] = out["sd"][s] = out["quant"][s] = np.nan
            continue
        s1, s2 = u[s].sum(), (u[s] * u[s]).sum()
        out["wsum"][s] = float(s1)
        out["ess"][s] = float(s1 * s1 / s2) if s1 > 0 else 0.0
        for v in range(V):
            fin = np.abs(yv[v, s][np.isfinite(yv[v, s])])
            out["scale"][s, v] = max(float(fin.max()) if fin.size else 0.0, 1e-300)
            out["mean"][s, v], out["sd"][s, v], out["quant"][s, v], out["n_nan"][s, v], out["near_tie"][s, v] = \
                summary(u[s], yv[v, s], probs)
    return out


def assert_matches(got, want, what="", stars=None, exact=False):
    """``got`` (of `call`) against the twin's ``want`` within the limits of the module's docstring, for the stars ``stars``
    (default: all); NaN, inf, counts and quantiles exactly.  The case must have no near tie unless it is ``exact``."""
    S = want["wsum"].shape[0]
    stars = np.arange(S) if stars is None else np.asarray(stars)
    assert exact or not want["near_tie"][stars].any(), (what, "the case has a near tie: pick another seed")
    for k in ("n_bad", "n_nan"):
        assert np.array_equal(got[k][stars], want[k][stars]), (what, k)
    for k in ("wsum", "ess", "mean", "sd", "quant"):
        g, w = got[k][stars], want[k][stars]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(g)], w[np.isinf(w)]), (what, k)
    assert np.array_equal(got["quant"][stars], want["quant"][stars], equal_nan=True), (what, "quant")
    live = stars[~np.isnan(want["wsum"][stars])]
    gu, wu = got["weights"][live], want["weights"][live]
    lim = (1e-11 * np.maximum(1.0, want["dmax"][live] / 100.0))[:, None]
    assert np.all(np.abs(gu - wu) <= lim * wu + 1e-300), (what, "weights", float(np.max(np.abs(gu - wu) / (lim * wu + 1e-300))))
    for k in ("wsum", "ess"):
        g, w = got[k][live], want[k][live]
        assert np.all(np.abs(g - w) <= 1e-10 * np.abs(w)), (what, k)
    for k in ("mean", "sd"):
        g, w, sc = got[k][live], want[k][live], want["scale"][live]
        fin = np.isfinite(w)
        assert np.all(np.abs(g[fin] - w[fin]) <= 1e-10 * sc[fin]), (what, k, float(np.max(np.abs(g[fin] - w[fin]) / sc[fin])))


# -- cases ------------------------------------------------------------------------------------------------------------
def add_values(case, V, seed, with_model=True, probs=PROBS3):
    """Give a tests/_hier_twin case ``V`` value columns: with ``with_model`` the first is model column 0 where it lies,
    the rest live in a storage of their own ([T, V + 1, S * W], columns from 1 up) at different scales; the second holds a
    copy of model column 0, so that weight and value are correlated."""
    rng = np.random.default_rng(7000 + seed)
    S, W, T = case["S"], case["W"], case["T"]
    M = W * T
    y = rng.normal(size=(V, S, M)) * (10.0 ** rng.integers(-3, 4, size=(V, 1, 1))) + rng.normal(size=(V, 1, 1))
    if V > 1:
        y[1] = case["x"][0]
    case["y"] = y
    case["values"] = [("x", 0) if with_model and v == 0 else ("y", v) for v in range(V)]
    case["probs"] = np.asarray(probs, dtype=np.float64)
    case.pop("want_rw", None)
    return case


def random_case(S, W, T, Q, H, V, seed, layout=_cabi.CHAIN_PARAM_MAJOR, probs=PROBS3):
    return add_values(ht.random_case(S, W, T, Q, H, seed, layout), V, seed, probs=probs)


def fixed_case(x, y, interim_priors, row_priors, W, T, probs=PROBS3, layout=_cabi.CHAIN_PARAM_MAJOR, mask=None, seed=0):
    """``x`` [Q, S, M] model columns, ``y`` [V, S, M] value columns of their own."""
    case = ht.fixed_case(np.ascontiguousarray(x, dtype=np.float64), interim_priors, row_priors, W, T, layout, mask, seed)
    case["y"] = np.ascontiguousarray(y, dtype=np.float64)
    case["values"] = [("y", v) for v in range(case["y"].shape[0])]
    case["probs"] = np.asarray(probs, dtype=np.float64)
    return case


def kind_case(kind):
    """tests/_hier_twin.kind_case (the kind as interim prior of column 0 and as population of column 1) with two value columns."""
    return add_values(ht.kind_case(kind), 2, kind)


def unit_case(y, W, T, H=1, probs=PROBS3, seed=0):
    """Rows equal to the interim record: with ``ln_norm = ell`` (= 0) every weight is exactly ``H``.  ``y`` [V, S, M]."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    rng = np.random.default_rng(seed)
    g = P.GaussianPrior(0.0, 1.0)
    x = rng.normal(0.0, 0.5, (1,) + y.shape[1:])
    return fixed_case(x, y, [g], [[g]] * H, W, T, probs, seed=seed)


def integer_case(y, u, W, T, probs=PROBS3):
    """Weights that are the small integers ``u`` [S, M] exactly: a flat interim prior on (0, 1), x = (m + 0.5) / M, and
    ``ln_norm = 0`` under rows FLAT on (0, 1) whose p0 = ln(k) would need one row per weight; instead the weights are made
    of H = max(u) rows, row h being flat on the samples with u > h (an interval in x after sorting by u).  ``y`` [V, S, M]."""
    y, u = np.ascontiguousarray(y, dtype=np.float64), np.asarray(u, dtype=np.int64)
    S, M = u.shape
    assert S == 1
    order = np.argsort(-u[0], kind="stable")                       # largest weight at the smallest x
    x = np.empty((1, 1, M))
    x[0, 0, order] = (np.arange(M) + 0.5) / M
    flat = hi.prior_record(P.FlatPrior((0.0, 1.0)))
    rows = []
    for h in range(int(u.max())):
        n = int((u[0] > h).sum())                                   # row h covers the n samples of weight > h
        r = hi.prior_record(P.FlatPrior((0.0, n / M)))
        r["p"][0, 0] = flat["p"][0, 0]                               # the density of the interim prior: the ratio is exactly 1
        rows.append([r])
    case = fixed_case(x, y, [flat], rows, W, T, probs)
    case["ln_norm"] = np.zeros((len(rows), 1))
    return case


def special_cases():
    """name -> case (see tests/test_gpu_reweight.py for what each is for)."""
    rng = np.random.default_rng(11)
    W, T, S = 5, 7, 3
    M = W * T
    out = {}
    flat = P.FlatPrior((-4.0, 4.0))
    gauss = [[P.GaussianPrior(0.0, 1.0)], [P.GaussianPrior(0.2, 0.4)], [P.GaussianPrior(-0.3, 0.8)]]
    # star 1 lies outside the first row's support (its ell is -inf there): one dead row among good ones; and a case whose
    # every row is dead for that star
    x = rng.normal(0.0, 0.5, (1, S, M))
    x[0, 1] = rng.uniform(1.0, 2.0, M)
    y = rng.normal(size=(2, S, M))
    out["one_dead_row"] = fixed_case(x, y, [flat], [[P.FlatPrior((-1.0, 0.9))], [P.GaussianPrior(0.0, 1.0)]], W, T)
    out["all_dead_rows"] = fixed_case(x, y, [flat], [[P.GaussianPrior(0.0, 1.0, bounds=(-1.0, 0.9))],
                                                       [P.GaussianPrior(0.2, 0.4, bounds=(-2.0, 0.95))]], W, T)
    # bad samples and NaN values on good samples
    x = rng.normal(0.0, 0.5, (2, S, M))
    x[0, 0, 3] = x[1, 0, 3] = np.nan
    x[1, 2, 7] = np.nan
    x[0, 2, 11] = 5.0                                               # outside the interim prior
    y = rng.normal(size=(2, S, M))
    y[0, 0, 5] = y[0, 0, 6] = y[1, 2, 0] = np.nan
    y[1, 1, :] = np.nan                                             # a whole column of a star: tot = 0
    out["bad_and_nan"] = fixed_case(x, y, [flat, flat], [[P.GaussianPrior(0.0, 1.0), P.GaussianPrior(0.1, 0.7)],
                                                         [P.FlatPrior((-1.0, 1.0)), P.GaussianPrior(0.0, 2.0)]], W, T)
    x = rng.normal(0.0, 0.5, (1, S, M))
    out["masked"] = fixed_case(x, rng.normal(size=(2, S, M)), [flat], gauss, W, T, mask=[1, 0, 1])
    return out


def digit_values(M, seed=0):
    """[4, 1, M] value columns for the radix select at unit weights: (0) neighbours in the last bit of the mantissa, (1)
    both signs and every exponent range, +-0, +-inf and subnormals, (2) all equal, (3) half equal."""
    rng = np.random.default_rng(seed)
    y = np.empty((4, 1, M))
    base = np.float64(1.5).view(np.uint64)
    y[0, 0] = rng.permutation((base + np.arange(M, dtype=np.uint64)).view(np.float64))
    wild = np.concatenate([[0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1e-310, 1.7e308, -1.7e308],
                           rng.choice([-1.0, 1.0], M) * 10.0 ** rng.uniform(-300, 300, M)])[:M]
    y[1, 0] = rng.permutation(wild)
    y[2, 0] = 2.75
    y[3, 0] = rng.permutation(np.where(np.arange(M) < M // 2, -1.25, rng.normal(size=M)))
    return y


def shrinkage_case(S=200, W=32, T=100, seed=3):
    """The conjugate Gaussian check: truths N(0, 1), observation error 0.5, a flat interim prior, chain samples drawn
    N(obs, 0.5^2), one row N(0, 1) as TruncatedGaussian on wide bounds.  Returns (case, obs [S])."""
    rng = np.random.default_rng(seed)
    truth = rng.normal(0.0, 1.0, S)
    obs = truth + rng.normal(0.0, 0.5, S)
    x = obs[None, :, None] + rng.normal(0.0, 0.5, (1, S, W * T))
    rec = hi.records(1)
    hi.TruncatedGaussian((-50.0, 50.0)).fill(rec, np.array([[0.0, 1.0]]))
    case = fixed_case(x, x, [P.FlatPrior((-50.0, 50.0))], [[rec]], W, T, seed=seed)
    case["values"] = [("x", 0)]
    return case, obs


# -- the calls ----------------------------------------------------------------------------------------------------------
def ell(case, hier_lib=None):
    """The case's ``ln_norm`` [H, S]: its own where it has one, otherwise ell of iso_hier_lnlike_host, computed once."""
    if case.get("ln_norm") is None:
        rc_, got = ht.call(hc.lib() if hier_lib is None else hier_lib, case, total=False)
        assert rc_ == 0
        case["ln_norm"] = got["ell"]
    return case["ln_norm"]


def want(case):
    if "want_rw" not in case:
        case["want_rw"] = reweight(case)
    return case["want_rw"]


def _value_storage(case, first, n):
    """The case's own value columns of the stars [first, first + n) as a storage [T, V + 1, n * W] (column 0 is filler)."""
    y, W, T = case["y"], case["W"], case["T"]
    V = y.shape[0]
    st = np.full((T, V + 1, n * W), -3.0)
    for v in range(V):
        st[:, v + 1, :] = y[v, first:first + n].reshape(n, T, W).transpose(1, 0, 2).reshape(T, n * W)
    if case["layout"] == _cabi.CHAIN_ROW_MAJOR:
        st = np.ascontiguousarray(st.transpose(0, 2, 1))
    return st


def call(lib, case, device=None, ens_begin=0, n_ens_out=None, rows=None, ln_norm=None, values=None, probs=None,
         value_range=None, offset=0):
    """``iso_reweight_stars_host`` on the case's numpy storages or, with ``device`` (a torch device),
    ``iso_reweight_stars`` on copies there.  ``values``: indices into the case's value columns (default: all); ``value_range``
    = (first, n): the case's own value columns come from a storage that holds only those stars; ``offset``: doubles of
    padding in front of every device storage, so that it lies at another address.  Returns ``(rc, dict)`` of numpy arrays
    ``weights`` [S, M] (the call's rows placed at their stars), ``wsum``, ``ess``, ``n_bad`` [S], ``mean``, ``sd``, ``n_nan``
    [S, V], ``quant`` [S, V, K]; what the call does not write keeps the fill value -7."""
    S, W, T = case["S"], case["W"], case["T"]
    M = W * T
    rows = case["rows"] if rows is None else rows
    ln_norm = ell(case) if ln_norm is None else ln_norm
    probs = np.ascontiguousarray(case["probs"] if probs is None else probs, dtype=np.float64)
    H, Q = rows.shape
    K = probs.size
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    picked = case["values"] if values is None else [case["values"][i] for i in values]
    V = len(picked)
    first, nval = (0, S) if value_range is None else value_range
    host_storages = list(case["storages"]) + [_value_storage(case, first, nval)]
    mask = case["mask"]
    shapes = dict(weights=(max(n_ens_out, 1), M), wsum=(S,), ess=(S,), n_bad=(S,), mean=(S, V), sd=(S, V), quant=(S, V, K),
                  n_nan=(S, V))
    ints = ("n_bad", "n_nan")
    if device is None:
        keep = host_storages
        base = [st.ctypes.data for st in keep]
        out = {k: np.full(sh, -7, np.int32) if k in ints else np.full(sh, -7.0) for k, sh in shapes.items()}
        interim, drows, dln = np.ascontiguousarray(case["interim"]), np.ascontiguousarray(rows), np.ascontiguousarray(ln_norm)
        ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)
        fn, stream = lib.iso_reweight_stars_host, None
    else:
        import torch
        from isochrones_amd import device as dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        keep, base = [], []
        for st in host_storages:
            buf = torch.full((offset + st.size,), -5.0, dtype=torch.float64, device=device)
            buf[offset:] = up(st.reshape(-1))
            keep.append(buf)
            base.append(buf.data_ptr() + 8 * offset)
        out = {k: torch.full(sh, -7, dtype=torch.int32 if k in ints else torch.float64, device=device)
               for k, sh in shapes.items()}
        interim = up(np.ascontiguousarray(case["interim"]).view(np.uint8))
        drows = up(np.ascontiguousarray(rows).view(np.uint8).reshape(-1))
        dln = up(ln_norm)
        mask = None if mask is None else up(mask)
        ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.data_ptr())
        fn, stream = lib.iso_reweight_stars, dev.stream_ptr(device.index)
    cols = (hc.IsoHierColumn * Q)(*[hc.IsoHierColumn(base[k], ncols, col, S, 0) for k, ncols, col in case["where"][:Q]])
    vals = (hc.IsoHierColumn * max(V, 1))()
    for i, (kind, j) in enumerate(picked):
        if kind == "x":
            k, ncols, col = case["where"][j]
            vals[i] = hc.IsoHierColumn(base[k], ncols, col, S, 0)
        else:
            vals[i] = hc.IsoHierColumn(base[-1], case["y"].shape[0] + 1, j + 1, nval, first)
    code = fn(cols, Q, vals, V, case["layout"], T, S, W, ens_begin, n_ens_out, ptr(interim), ptr(drows), H, ptr(dln), ptr(mask),
              probs.ctypes.data_as(C.POINTER(C.c_double)), K, *[ptr(out[k]) for k in ("weights", "wsum", "ess", "n_bad", "mean",
                                                                                      "sd", "quant", "n_nan")], stream)
    host = {k: (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for k, a in out.items()}
    full = np.full((S, M), -7.0)
    if code == 0:
        full[ens_begin:ens_begin + n_ens_out] = host["weights"][:n_ens_out]
    host["weights"] = full
    return code, host


def check_equal_rows(lib, device, H):
    """The H rows all equal to one row: u is the H = 1 value added H times in ascending order, bit for bit.  For H = 2 and
    4 that is H * u exactly (2t is exact; 3t falls half way between two doubles, and adding t to either neighbour rounds
    to 4t), so the sums scale exactly and ess and the quantiles do not move; from H = 8 on the running sum rounds (5t,
    6t, 7t each round to a multiple of 4 ulp(t)), and the definition's ascending sum is what is asserted."""
    case = random_case(2, 3, 7, 2, 1, 2, seed=5)
    code, one = call(lib, case, device)
    rows, ln = np.repeat(case["rows"], H, axis=0), np.repeat(ell(case), H, axis=0)
    code2, many = call(lib, case, device, rows=rows, ln_norm=ln)
    assert code == 0 == code2
    acc = np.zeros_like(one["weights"])
    for _ in range(H):
        acc = acc + one["weights"]
    assert np.array_equal(many["weights"], acc)
    if H <= 4:
        assert np.array_equal(acc, H * one["weights"]) and np.array_equal(many["wsum"], H * one["wsum"])
        assert np.array_equal(many["quant"], one["quant"]) and np.array_equal(many["ess"], one["ess"])
        assert np.array_equal(many["mean"], one["mean"]) and np.array_equal(many["sd"], one["sd"])


def restrict(want_, values):
    """The twin's result for a subset ``values`` of the case's value columns."""
    out = dict(want_)
    for k in ("mean", "sd", "n_nan", "near_tie", "scale"):
        out[k] = want_[k][:, values]
    out["quant"] = want_["quant"][:, values]
    return out
