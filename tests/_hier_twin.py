"""A long-double numpy statement of include/isochrones_amd_hier.h (the hierarchical likelihood of libiso_hier.so), the
cases its host and device tests share, and the one way they call the library.

The twin evaluates the family records as the header writes them, in numpy's long double (64-bit mantissa), and sums in
numpy's pairwise order: against it, |d ell| <= 1e-11 * max(1, max_m |r| / 100) and ess within 1e-10 relative.  (Worst-case
rounding of the float64 implementations at M <= 4096 samples and |r| <= 100: r carries a few ulp of 100, 5e-14, the M-term
sums add M * 2^-53 = 5e-13 relative at the very worst and 1e-14 typically; below 1e-12, so the limit leaves a factor ten.)"""
import ctypes as C

import numpy as np

from isochrones_amd import _cabi, _hier_cabi as hc, hierarchical as hi, priors as P

LD = np.longdouble
LN10 = np.log(LD(10))


def lnf(rec, x):
    """ln f(x; rec) of the header for a float64 array ``x``, in long double."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    p = [LD(v) for v in rec["p"]]
    lo, hi_, kind = LD(rec["lo"]), LD(rec["hi"]), int(rec["kind"])
    out = (x < lo) | (x > hi_)
    ninf = LD(-np.inf)
    with np.errstate(all="ignore"):
        lx = np.log(x)
        if kind == hc.FLAT:
            v = np.full(x.shape, p[0])
        elif kind == hc.FLATLOG:
            v = p[0] + x * LN10
        elif kind == hc.POWERLAW:
            v = p[0] + p[1] * lx
        elif kind in (hc.GAUSS, hc.TRUNCGAUSS):
            z = (x - p[0]) * p[3]
            v = -(z * z) / 2 + p[2]
        elif kind == hc.LOGNORMAL:
            l = lx - p[0]
            return (p[2] - l) - LD(0.5) * (l * p[3]) ** 2
        elif kind == hc.CHABRIER:
            l = lx - p[0]
            low = (p[2] - l) - LD(0.5) * (l * p[1]) ** 2
            high = np.where(out, ninf, p[4] + p[3] * lx)
            return np.where(x < p[5], low, high)
        elif kind == hc.FEH:
            if p[2] != 0:
                disk = 1 / LD(2.5066282746310007) * (LD(0.8) / LD(0.15) * np.exp(-LD(0.5) * (x - LD(0.016)) ** 2 / LD(0.15) ** 2)
                                                     + LD(0.2) / LD(0.22) * np.exp(-LD(0.5) * (x + LD(0.15)) ** 2 / LD(0.22) ** 2))
            else:
                disk = 1 / np.sqrt(2 * LD(np.pi)) / LD(0.3) * np.exp(-LD(0.5) * (x + LD(0.3)) ** 2 / LD(0.3) ** 2)
            halo = 1 / np.sqrt(2 * LD(np.pi) * LD(0.4) ** 2) * np.exp(-LD(0.5) * (x + LD(1.5)) ** 2 / LD(0.4) ** 2)
            v = np.log((p[0] * halo + (1 - p[0]) * disk) / p[1])
        else:
            return np.full(x.shape, LD(np.nan))
    return np.where(out, ninf, v)


def lnlike(x, interim, rows, mask=None):
    """``x`` [Q, S, M] float64, ``interim`` [Q] and ``rows`` [H, Q] records -> dict of float64 arrays ``ell``, ``ess``
    [H, S], ``n_bad`` [S], ``L``, ``min_ess`` [H] and ``rmax`` [H, S] (max_m |r| over the good samples with a finite r)."""
    Q, S, M = x.shape
    H = rows.shape[0]
    ell, ess, rmax = np.empty((H, S), LD), np.empty((H, S), LD), np.zeros((H, S))
    n_bad = np.zeros(S, np.int32)
    with np.errstate(all="ignore"):
        for s in range(S):
            if mask is not None and not mask[s]:
                ell[:, s] = ess[:, s] = np.nan
                continue
            l0 = [lnf(interim[q], x[q, s]) for q in range(Q)]
            good = np.ones(M, bool)
            for q in range(Q):
                good &= ~np.isnan(x[q, s]) & ~np.isnan(l0[q]) & (l0[q] != -np.inf)
            n_bad[s] = M - good.sum()
            for h in range(H):
                r = np.zeros(M, LD)
                for q in range(Q):
                    lf = lnf(rows[h, q], x[q, s])
                    lf = np.where(np.isnan(lf), LD(-np.inf), lf)
                    r = lf - l0[q] if q == 0 else r + (lf - l0[q])
                r = r[good]
                fin = r[np.isfinite(r)]
                if fin.size == 0:
                    ell[h, s], ess[h, s] = -np.inf, 0
                    continue
                mx = r.max()
                w = np.exp(r - mx)
                ell[h, s] = mx + np.log(w.sum()) - np.log(LD(M))
                ess[h, s] = w.sum() ** 2 / (w * w).sum()
                rmax[h, s] = float(np.abs(fin).max())
        keep = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
        L = ell[:, keep].sum(axis=1) if keep.any() else np.zeros(H)
        mn = ess[:, keep].min(axis=1) if keep.any() else np.full(H, np.inf)
    return dict(ell=ell.astype(np.float64), ess=ess.astype(np.float64), n_bad=n_bad, L=np.asarray(L, np.float64),
                min_ess=np.asarray(mn, np.float64), rmax=rmax)


def assert_matches(got, want, what=""):
    """``got`` against the twin's ``want`` within the limits of the module's docstring; -inf, NaN and n_bad exactly."""
    for k in ("ell", "ess", "L", "min_ess"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(g)], w[np.isinf(w)]), (what, k)
    assert np.array_equal(got["n_bad"], want["n_bad"]), what
    fin = np.isfinite(want["ell"])
    lim = 1e-11 * np.maximum(1.0, want["rmax"] / 100.0)
    with np.errstate(invalid="ignore"):
        d = np.abs(got["ell"] - want["ell"])
    assert np.all(d[fin] <= lim[fin]), (what, "ell", float(np.max(d[fin] / lim[fin])))
    e = np.abs(got["ess"][fin] - want["ess"][fin]) / np.maximum(want["ess"][fin], 1e-300)
    assert np.all(e <= 1e-10), (what, "ess", float(e.max()) if e.size else 0.0)
    finL = np.isfinite(want["L"])
    nstar = max(1, want["ell"].shape[1])
    assert np.all(np.abs(got["L"][finL] - want["L"][finL]) <= nstar * lim.max(axis=1)[finL]), (what, "L")
    m = np.isfinite(want["min_ess"])
    assert np.all(np.abs(got["min_ess"][m] - want["min_ess"][m]) <= 1e-10 * want["min_ess"][m]), (what, "min_ess")


# -- cases ------------------------------------------------------------------------------------------------------------
#: per column type: how its values are drawn, interim priors (cycled by the seed) and population families
def _mass(rng, n):
    return np.exp(rng.normal(0.0, 0.5, n)).clip(0.12, 9.0)


def _feh(rng, n):
    return rng.normal(-0.1, 0.3, n).clip(-3.5, 0.45)


def _age(rng, n):
    return rng.uniform(8.5, 10.1, n)


def _av(rng, n):
    return rng.uniform(0.0, 1.0, n)


COLUMN_TYPES = (
    (_mass, (P.ChabrierPrior(), P.PowerLawPrior(-2.35, (0.1, 10.0)), P.LogNormalPrior(0.0, 0.6)),
     lambda: hi.PowerLaw((0.1, 10.0)), lambda rng, H: rng.uniform(-3.0, 0.5, (H, 1))),
    (_feh, (P.FehPrior(bounds=(-4.0, 0.5)), P.FlatPrior((-4.0, 0.5)), P.GaussianPrior(0.0, 0.5)),
     lambda: hi.TruncatedGaussian((-4.0, 0.5)), lambda rng, H: np.column_stack([rng.uniform(-0.5, 0.2, H), rng.uniform(0.1, 0.6, H)])),
    (_age, (P.AgePrior((5, 10.15)), P.FlatPrior((5.0, 10.15))),
     lambda: hi.TruncatedGaussian((5.0, 10.15)), lambda rng, H: np.column_stack([rng.uniform(9.0, 10.0, H), rng.uniform(0.2, 1.0, H)])),
    (_av, (P.FlatPrior((0.0, 1.0)), P.GaussianPrior(0.3, 0.5, bounds=(0.0, 1.0))),
     lambda: hi.Fixed(P.PowerLawPrior(0.5, (0.0, 1.0))), lambda rng, H: np.empty((H, 0))),
)


def place(x, W, T, layout, seed, split=True):
    """The columns ``x`` [Q, S, M] (m = t * W + w) placed in storages: with ``split`` the even columns in one storage of
    Q + 2 columns, the odd ones in a second of 3 columns (different C), filled with other numbers elsewhere.  Returns
    ``(storages, where)`` with ``where[q] = (storage number, ncols, col)``."""
    Q, S, M = x.shape
    rng = np.random.default_rng(1000 + seed)
    widths = (Q + 2, 3) if split and Q > 1 else (Q + 2,)
    storages = [rng.normal(size=(T, c, S * W)) for c in widths]
    where, used = [], [0] * len(widths)
    for q in range(Q):
        k = q % len(widths)
        col = widths[k] - 1 - used[k]                               # from the last column down
        used[k] += 1
        storages[k][:, col, :] = x[q].reshape(S, T, W).transpose(1, 0, 2).reshape(T, S * W)
        where.append((k, widths[k], col))
    if layout == _cabi.CHAIN_ROW_MAJOR:
        storages = [np.ascontiguousarray(st.transpose(0, 2, 1)) for st in storages]
    return storages, where


def random_case(S, W, T, Q, H, seed, layout=_cabi.CHAIN_PARAM_MAJOR, split=True):
    """Q columns of the types above: values, interim records, H population rows, the storages."""
    rng = np.random.default_rng(seed)
    M = W * T
    x = np.empty((Q, S, M))
    fams, thetas, interim = {}, [], []
    for q in range(Q):
        draw, priors, family, theta = COLUMN_TYPES[(q + seed) % len(COLUMN_TYPES)]
        x[q] = draw(rng, S * M).reshape(S, M)
        interim.append(hi.prior_record(priors[(seed + q) % len(priors)]))
        fams["c%d" % q] = family()
        thetas.append(theta(rng, H))
    model = hi.PopulationModel(**fams)
    rows = model.pack(np.concatenate(thetas, axis=1))
    storages, where = place(x, W, T, layout, seed, split)
    return dict(x=x, interim=np.concatenate(interim), rows=rows, storages=storages, where=where, S=S, W=W, T=T, layout=layout,
                mask=None)


def fixed_case(x, interim_priors, row_priors, W, T, layout=_cabi.CHAIN_PARAM_MAJOR, mask=None, seed=0):
    """``x`` [Q, S, M]; ``interim_priors`` [Q] prior objects or records; ``row_priors`` [H][Q] likewise."""
    rec = lambda p: p if isinstance(p, np.ndarray) else hi.prior_record(p)
    interim = np.concatenate([rec(p) for p in interim_priors])
    rows = np.stack([np.concatenate([rec(p) for p in row]) for row in row_priors])
    storages, where = place(x, W, T, layout, seed)
    return dict(x=x, interim=interim, rows=rows, storages=storages, where=where, S=x.shape[1], W=W, T=T, layout=layout,
                mask=None if mask is None else np.ascontiguousarray(mask, dtype=np.int32))


def want(case):
    if "want" not in case:
        case["want"] = lnlike(case["x"], case["interim"], case["rows"], case["mask"])
    return case["want"]


def all_kinds():
    """One record of every kind whose support holds (0.2, 3), by kind."""
    tg = hi.TruncatedGaussian((0.1, 10.0))
    rec = hi.records(1)
    tg.fill(rec, np.array([[1.0, 0.7]]))
    return {hc.FLAT: hi.prior_record(P.FlatPrior((0.1, 10.0))), hc.FLATLOG: hi.prior_record(P.FlatLogPrior((-1.0, 6.0))),
            hc.POWERLAW: hi.prior_record(P.PowerLawPrior(-2.35, (0.1, 10.0))),
            hc.GAUSS: hi.prior_record(P.GaussianPrior(1.0, 0.5, bounds=(0.1, 10.0))),
            hc.LOGNORMAL: hi.prior_record(P.LogNormalPrior(0.0, 0.5)), hc.CHABRIER: hi.prior_record(P.ChabrierPrior()),
            hc.FEH: hi.prior_record(P.FehPrior(bounds=(-4.0, 6.0))), hc.TRUNCGAUSS: rec}


def kind_case(kind, W=5, T=7, S=3):
    """Column 0 has ``kind`` as its interim prior and a flat population; column 1 a flat interim and ``kind`` as ``Fixed``
    population (second row: the power law), on values in (0.2, 3)."""
    rng = np.random.default_rng(kind)
    kinds = all_kinds()
    x = rng.uniform(0.2, 3.0, (2, S, W * T))
    flat = kinds[hc.FLAT]
    return fixed_case(x, [kinds[kind], flat], [[flat, kinds[kind]], [kinds[hc.POWERLAW], kinds[kind]]], W, T, seed=kind)


def special_cases():
    """name -> case: no support under a row, NaN samples, a masked star, r spanning +-700 inside one star."""
    rng = np.random.default_rng(5)
    W, T, S = 5, 7, 3
    M = W * T
    out = {}
    flat = P.FlatPrior((-4.0, 4.0))
    x = rng.normal(0.0, 0.5, (1, S, M))
    x[0, 1] = rng.uniform(1.0, 2.0, M)                              # star 1 lies outside the first row's support
    out["no_support"] = fixed_case(x, [flat], [[P.FlatPrior((-1.0, 0.9))], [P.GaussianPrior(0.0, 1.0)]], W, T)
    x = rng.normal(0.0, 0.5, (2, S, M))
    x[0, 0, 3] = x[1, 0, 3] = np.nan                                # one sample, both columns: counted once
    x[1, 2, 7] = np.nan
    x[0, 2, 11] = 5.0                                               # outside the interim prior: bad too
    out["nan"] = fixed_case(x, [flat, flat], [[P.GaussianPrior(0.0, 1.0), P.GaussianPrior(0.1, 0.7)],
                                              [P.FlatPrior((-1.0, 1.0)), P.GaussianPrior(0.0, 2.0)]], W, T)
    x = rng.normal(0.0, 0.5, (1, S, M))
    out["masked"] = fixed_case(x, [flat], [[P.GaussianPrior(0.0, 1.0)], [P.GaussianPrior(0.2, 0.4)]], W, T, mask=[1, 0, 1])
    x = np.empty((1, S, M))
    for s in range(S):
        x[0, s] = rng.permutation(np.linspace(0.0, 37.4, M))       # r = x^2 / 2 - (x - 37.4)^2 / 2: -699 .. +699
    out["span_700"] = fixed_case(x, [P.GaussianPrior(0.0, 1.0)], [[P.GaussianPrior(37.4, 1.0)], [P.GaussianPrior(20.0, 1.0)]], W, T)
    return out


# -- the call ---------------------------------------------------------------------------------------------------------
MARGIN = 64


def guarded(shape, dtype, device):
    """``(flat, view)``: a tensor of ``shape`` on ``device`` filled with -7, inside a buffer with MARGIN more of them either
    side of it."""
    import torch
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * MARGIN,), -7, dtype=dtype, device=device)
    return flat, flat[MARGIN:MARGIN + n].view(shape)


def margins_untouched(flat):
    return bool((flat[:MARGIN] == -7).all()) and bool((flat[-MARGIN:] == -7).all())


def call(lib, case, device=None, ens_begin=0, n_ens_out=None, rows=None, total=True, out=None, guard=False):
    """``iso_hier_lnlike_host`` on the case's numpy storages or, with ``device`` (a torch device), ``iso_hier_lnlike`` on
    copies there.  Returns ``(rc, dict)`` of numpy arrays ``ell``, ``ess`` [H, S], ``n_bad`` [S], ``L``, ``min_ess`` [H];
    what the call does not write keeps the fill value -7.  With ``guard`` every device output lies between two margins of
    -7 that have to stay so."""
    S, W, T = case["S"], case["W"], case["T"]
    rows = case["rows"] if rows is None else rows
    H, Q = rows.shape
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    mask = case["mask"]
    if device is None:
        keep = list(case["storages"])
        base = [st.ctypes.data for st in keep]
        ell, ess, n_bad = np.full((H, S), -7.0), np.full((H, S), -7.0), np.full(S, -7, np.int32)
        L, mn = np.full(H, -7.0), np.full(H, -7.0)
        interim, drows = np.ascontiguousarray(case["interim"]), np.ascontiguousarray(rows)
        ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)
        fn, stream = lib.iso_hier_lnlike_host, None
    else:
        import torch
        from isochrones_amd import device as dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        keep = [up(st) for st in case["storages"]]
        base = [t.data_ptr() for t in keep]
        f64 = dict(dtype=torch.float64, device=device)
        ell, ess = torch.full((H, S), -7.0, **f64), torch.full((H, S), -7.0, **f64)
        n_bad = torch.full((S,), -7, dtype=torch.int32, device=device)
        L, mn = torch.full((H,), -7.0, **f64), torch.full((H,), -7.0, **f64)
        flats = []
        if guard:
            flats, (ell, ess, n_bad, L, mn) = zip(*[guarded(t.shape, t.dtype, device) for t in (ell, ess, n_bad, L, mn)])
        interim = up(np.ascontiguousarray(case["interim"]).view(np.uint8))
        drows = up(np.ascontiguousarray(rows).view(np.uint8).reshape(-1))
        mask = None if mask is None else up(mask)
        ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.data_ptr())
        fn, stream = lib.iso_hier_lnlike, dev.stream_ptr(device.index)
    cols = (hc.IsoHierColumn * Q)(*[hc.IsoHierColumn(base[k], ncols, col, S, 0) for k, ncols, col in case["where"][:Q]])
    rc = fn(cols, Q, case["layout"], T, S, W, ens_begin, n_ens_out, ptr(interim), ptr(drows), H, ptr(mask), ptr(ell),
            ptr(ess), ptr(n_bad), ptr(L if total else None), ptr(mn if total else None), stream)
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    if device is not None:
        assert all(margins_untouched(f) for f in flats), "a write outside an output"
    return rc, dict(ell=host(ell), ess=host(ess), n_bad=host(n_bad), L=host(L), min_ess=host(mn))
