"""A long-double numpy statement of include/isochrones_amd_binned.h (the compression of a chain to per-star cell tables and
the contraction of those tables with the rows' log cell densities, libiso_binned.so), the cases its host and device tests
share, and the one way they call the library.

The twin evaluates the family records as tests/_hier_twin.py does, in numpy's long double, and sums in numpy's pairwise
order.  The limits are that module's: |d ell| <= 1e-11 * max(1, max_m |r| / 100) with r = c_m + lnh[cell of m], ess within
1e-10 relative; a table is compared as mx + ln A and 2 mx + ln A2 within the same limit (mx itself is a rounded maximum,
so A alone is only defined up to the rounding of mx)."""
import ctypes as C

import numpy as np

from isochrones_amd import _binned_cabi as bc, _cabi, hierarchical as hi, priors as P
from tests import _hier_twin as tw

LD = np.longdouble
PM, RM = _cabi.CHAIN_PARAM_MAJOR, _cabi.CHAIN_ROW_MAJOR


def bin_of(edges, x):
    """numpy.histogram's rule: e[k] <= x < e[k + 1], the last bin closed above; -1 outside (and for a NaN)."""
    e = np.asarray(edges, dtype=np.float64)
    k = np.searchsorted(e, x, side="right") - 1
    k = np.where(x == e[-1], len(e) - 2, k)
    with np.errstate(invalid="ignore"):
        return np.where((x >= e[0]) & (x <= e[-1]), k, -1)


def n_cells(case):
    return int(np.prod([len(e) - 1 for e in case["edges"]]))


def sample_terms(case):
    """``(c [S, M] long double, cell [S, M] (-1: weighs nothing), bad [S, M], out [S, M])`` of the header's per-sample rule."""
    x, interim, frozen = case["x"], case["interim"], case["frozen"]
    Q, S, M = x.shape
    axes, edges = case["axes"], case["edges"]
    c = np.zeros((S, M), LD)
    bad = np.zeros((S, M), bool)
    inside = np.ones((S, M), bool)
    cell = np.zeros((S, M), np.int64)
    with np.errstate(all="ignore"):
        l0 = [tw.lnf(interim[q], x[q]) for q in range(Q)]
        for q in range(Q):
            bad |= np.isnan(x[q]) | np.isnan(l0[q]) | (l0[q] == -np.inf)
        for q in case["frozen_cols"]:
            lf = tw.lnf(frozen[q], x[q])
            c = c + (np.where(np.isnan(lf), LD(-np.inf), lf) - l0[q])
        for q in sorted(axes):
            c = c - l0[q]
        for a, q in enumerate(axes):
            k = bin_of(edges[a], x[q])
            inside &= k >= 0
            cell += np.maximum(k, 0) * (len(edges[1]) - 1 if a == 0 and len(axes) == 2 else 1)
        if case.get("extra") is not None:
            ex = case["extra"].reshape(S, M)
            bad |= np.isnan(ex) | (ex > 0)
            c = c + ex.astype(LD)
        out = ~bad & ~inside
        cell = np.where(~bad & inside & (c > -np.inf), cell, -1)
    return c, cell, bad, out


def compress(case):
    """dict of ``A``, ``A2`` [B, S] and ``mx`` [S] in long double, ``n_bad``, ``n_out`` [S] int32."""
    c, cell, bad, out = sample_terms(case)
    S, M = c.shape
    B, mask = n_cells(case), case.get("mask")
    A, A2, mx = np.zeros((B, S), LD), np.zeros((B, S), LD), np.full(S, LD(-np.inf))
    n_bad, n_out = bad.sum(axis=1).astype(np.int32), out.sum(axis=1).astype(np.int32)
    for s in range(S):
        if mask is not None and not mask[s]:
            mx[s], n_bad[s], n_out[s] = np.nan, 0, 0
            continue
        use = cell[s] >= 0
        if not use.any():
            continue
        mx[s] = c[s][use].max()
        w = np.exp(c[s][use] - mx[s])
        for b in np.unique(cell[s][use]):
            A[b, s], A2[b, s] = w[cell[s][use] == b].sum(), (w[cell[s][use] == b] ** 2).sum()
    return dict(A=A, A2=A2, mx=mx, n_bad=n_bad, n_out=n_out)


def lnlike(tab, lnh, M, mask=None):
    """The contraction of the tables ``tab`` (any float type) with ``lnh`` [H, B], in long double: dict of float64 ``ell``,
    ``ess`` [H, S], ``L``, ``min_ess`` [H]."""
    A, A2, mx = (np.asarray(tab[k]).astype(LD) for k in ("A", "A2", "mx"))
    lnh = np.asarray(lnh, dtype=np.float64)
    H, S = lnh.shape[0], A.shape[1]
    ell, ess = np.empty((H, S), LD), np.empty((H, S), LD)
    with np.errstate(all="ignore"):
        for h in range(H):
            l = np.where(np.isnan(lnh[h]), -np.inf, lnh[h]).astype(LD)
            hmx = l.max()
            u = np.where(l > -np.inf, np.exp(l - hmx), LD(0))
            s1, s2 = (u[:, None] * A).sum(axis=0), ((u * u)[:, None] * A2).sum(axis=0)
            ok = s1 > 0
            ell[h] = np.where(ok, (mx + hmx) + np.log(np.where(ok, s1, 1)) - np.log(LD(M)), -np.inf)
            ess[h] = np.where(ok, s1 * s1 / np.where(ok, s2, 1), 0)
        keep = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
        ell[:, ~keep] = ess[:, ~keep] = np.nan
        L = ell[:, keep].sum(axis=1) if keep.any() else np.zeros(H)
        mn = ess[:, keep].min(axis=1) if keep.any() else np.full(H, np.inf)
    return dict(ell=ell.astype(np.float64), ess=ess.astype(np.float64), L=np.asarray(L, np.float64),
                min_ess=np.asarray(mn, np.float64))


def want(case):
    """The twin's tables and, for the case's ``lnh``, its likelihood with ``rmax`` [H, S] and ``n_bad``."""
    if "want" not in case:
        tab = compress(case)
        c, cell, _, _ = sample_terms(case)
        S, M = c.shape
        out = lnlike(tab, case["lnh"], M, case.get("mask"))
        lnh = np.where(np.isnan(case["lnh"]), -np.inf, case["lnh"])
        rmax = np.zeros((lnh.shape[0], S))
        cmax = np.zeros(S)
        with np.errstate(all="ignore"):
            for s in range(S):
                use = cell[s] >= 0
                if use.any():
                    cmax[s] = float(np.abs(c[s][use]).max())
                    r = c[s][use].astype(np.float64)[None, :] + lnh[:, cell[s][use]]
                    r = np.where(np.isfinite(r), np.abs(r), 0.0)
                    rmax[:, s] = r.max(axis=1)
        case["want"] = dict(out, rmax=rmax, cmax=cmax, n_bad=tab["n_bad"], tab=tab)
    return case["want"]


def assert_tables_match(got, case, what="", stars=None):
    """The library's tables ``got`` against the twin's: zeros, -inf, NaN and the counts exactly, mx + ln A and 2 mx + ln A2
    within the module's limit."""
    w = want(case)
    tab = w["tab"]
    sl = slice(None) if stars is None else stars
    assert np.array_equal(got["n_bad"][sl], tab["n_bad"][sl]) and np.array_equal(got["n_out"][sl], tab["n_out"][sl]), what
    gm, wm = got["mx"][sl], tab["mx"][sl].astype(np.float64)
    assert np.array_equal(np.isnan(gm), np.isnan(wm)) and np.array_equal(np.isneginf(gm), np.isneginf(wm)), what
    lim = 1e-11 * np.maximum(1.0, w["cmax"][sl] / 100.0)
    worst = 0.0
    for k, f in (("A", 1), ("A2", 2)):
        g, t = got[k][:, sl], tab[k][:, sl]
        assert np.array_equal(g > 0, t > 0) and np.all(g >= 0), (what, k)
        with np.errstate(all="ignore"):
            d = np.abs((f * gm.astype(LD) + np.log(g.astype(LD))) - (f * tab["mx"][sl] + np.log(t)))
        d = np.where(t > 0, d, 0).astype(np.float64)
        worst = max(worst, float(np.max(d / lim)))
        assert np.all(d <= lim), (what, k, worst)
    return worst


def assert_device_matches_host(dtab, dout, htab, hout, case, what=""):
    """The device's tables and likelihood against the host entry's, directly: counts, zeros, -inf and NaN exactly; mx + ln A,
    2 mx + ln A2 and ell within the module's limit (1e-11 where |r| <= 100), L within S times it, ess and min_ess within
    1e-11 relative.  Returns the largest |d ell|."""
    w = want(case)
    assert np.array_equal(dtab["n_bad"], htab["n_bad"]) and np.array_equal(dtab["n_out"], htab["n_out"]), what
    assert np.array_equal(np.isnan(dtab["mx"]), np.isnan(htab["mx"])), what
    assert np.array_equal(np.isneginf(dtab["mx"]), np.isneginf(htab["mx"])), what
    lim = 1e-11 * np.maximum(1.0, w["cmax"] / 100.0)
    for k, f in (("A", 1.0), ("A2", 2.0)):
        g, h = dtab[k], htab[k]
        assert np.array_equal(g > 0, h > 0), (what, k)
        with np.errstate(all="ignore"):
            d = np.abs((f * dtab["mx"] + np.log(g)) - (f * htab["mx"] + np.log(h)))
        d = np.where(h > 0, d, 0.0)
        assert np.all(d <= lim), (what, k, float(np.max(d / lim)))
    for k in ("ell", "ess", "L", "min_ess"):
        g, h = dout[k], hout[k]
        assert np.array_equal(np.isnan(g), np.isnan(h)), (what, k)
        assert np.array_equal(np.isinf(g), np.isinf(h)) and np.array_equal(g[np.isinf(g)], h[np.isinf(h)]), (what, k)
    lim = 1e-11 * np.maximum(1.0, w["rmax"] / 100.0)
    fin = np.isfinite(hout["ell"])
    d = np.abs(dout["ell"][fin] - hout["ell"][fin])
    assert np.all(d <= lim[fin]), (what, "ell", float(np.max(d / lim[fin])))
    assert np.all(np.abs(dout["ess"][fin] - hout["ess"][fin]) <= 1e-11 * hout["ess"][fin]), (what, "ess")
    finL = np.isfinite(hout["L"])
    nstar = max(1, hout["ell"].shape[1])
    assert np.all(np.abs(dout["L"] - hout["L"])[finL] <= nstar * lim.max(axis=1)[finL]), (what, "L")
    m = np.isfinite(hout["min_ess"])
    assert np.all(np.abs(dout["min_ess"] - hout["min_ess"])[m] <= 1e-11 * hout["min_ess"][m]), (what, "min_ess")
    return float(d.max()) if d.size else 0.0


def assert_matches(got, case, what=""):
    """``ell``, ``ess``, ``L``, ``min_ess`` of the library against the twin, by tests/_hier_twin.py's rule."""
    tw.assert_matches(dict(got, n_bad=want(case)["n_bad"]), want(case), what)


# -- cases ------------------------------------------------------------------------------------------------------------
def random_lnh(rng, H, B):
    """H rows of log cell densities, a few cells of height 0 among them."""
    lnh = rng.normal(0.0, 1.5, (H, B))
    if B > 1:
        lnh[rng.random((H, B)) < 0.1] = -np.inf
        lnh[:, 0] = np.where(np.isneginf(lnh).all(axis=1), 0.0, lnh[:, 0])
    return lnh


def make_case(S, W, T, n_bins, H, seed, layout=PM, n_frozen=1, extra=False, mask=None, uniform=False):
    """``len(n_bins)`` binned axes (column 0, and column 2 or 1 for a second) and ``n_frozen`` frozen columns between and
    after them, so that the axes are not the leading columns; values that leave the grid on both sides; non-uniform edges."""
    rng = np.random.default_rng(seed)
    M = W * T
    n_axes = len(n_bins)
    Q = n_axes + n_frozen
    axes = (0,) if n_axes == 1 else ((2, 0) if Q >= 3 else (1, 0))     # axis 0 is not the lower column: k0 and q differ
    frozen_cols = tuple(q for q in range(Q) if q not in axes)
    x = np.empty((Q, S, M))
    interim = hi.records(Q)
    frozen = hi.records(Q)
    edges = []
    for a, q in enumerate(axes):
        lo, hi_ = (8.6, 10.1) if a == 0 else (-1.0, 0.5)
        x[q] = rng.uniform(lo - 0.1, hi_ + 0.1, (S, M))
        K = n_bins[a]
        e = np.linspace(lo, hi_, K + 1) if uniform else np.sort(np.concatenate([[lo, hi_], rng.uniform(lo, hi_, K - 1)]))
        edges.append(np.ascontiguousarray(e))
        interim[q] = hi.prior_record((P.GaussianPrior(0.5 * (lo + hi_), 1.0), P.FlatPrior((lo - 0.5, hi_ + 0.5)))[(seed + a) % 2])[0]
    for i, q in enumerate(frozen_cols):
        draw, priors, _, _ = tw.COLUMN_TYPES[(i + seed) % 2]               # mass or [Fe/H]
        x[q] = draw(rng, S * M).reshape(S, M)
        interim[q] = hi.prior_record(priors[(seed + i) % len(priors)])[0]
        frozen[q] = hi.prior_record(priors[(seed + i + 1) % len(priors)])[0]
    case = dict(x=x, interim=interim, frozen=frozen, frozen_cols=frozen_cols, axes=axes, edges=edges, S=S, W=W, T=T,
                layout=layout, mask=None if mask is None else np.ascontiguousarray(mask, dtype=np.int32),
                extra=np.ascontiguousarray(-rng.exponential(1.0, S * M)) if extra else None)
    case["lnh"] = random_lnh(rng, H, n_cells(case))
    case["storages"], case["where"] = tw.place(x, W, T, layout, seed)
    return case


def replace_x(case, x, **other):
    """The case with other values (and anything else), placed anew."""
    new = {k: v for k, v in case.items() if k != "want"}
    new.update(other, x=x)
    new["storages"], new["where"] = tw.place(x, new["W"], new["T"], new["layout"], 0)
    return new


def one_axis_case(x, edges, W, T, interim=None, lnh=None, extra=None, mask=None, layout=PM):
    """One column ``x`` [S, M], binned on ``edges``; a flat interim prior on [-100, 100] unless given."""
    x = np.ascontiguousarray(x, dtype=np.float64)[None]
    edges = [np.ascontiguousarray(edges, dtype=np.float64)]
    K = edges[0].size - 1
    case = dict(x=x, interim=hi.prior_record(P.FlatPrior((-100.0, 100.0)) if interim is None else interim), frozen=hi.records(1),
                frozen_cols=(), axes=(0,), edges=edges, S=x.shape[1], W=W, T=T, layout=layout,
                mask=None if mask is None else np.ascontiguousarray(mask, dtype=np.int32),
                extra=None if extra is None else np.ascontiguousarray(extra, dtype=np.float64).reshape(-1),
                lnh=np.zeros((1, K)) if lnh is None else np.ascontiguousarray(lnh, dtype=np.float64))
    case["storages"], case["where"] = tw.place(x, W, T, layout, 0)
    return case


# -- the calls --------------------------------------------------------------------------------------------------------
def _i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def _mover(device):
    """``(up, ptr, host)``: to where the call runs, its address, and back."""
    if device is None:
        return (lambda a: np.ascontiguousarray(a)), (lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)), (lambda a: a)
    import torch
    return ((lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)),
            (lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.data_ptr())), (lambda a: a.cpu().numpy()))


def _stream(device):
    if device is None:
        return None
    from isochrones_amd import device as dev
    return dev.stream_ptr(device.index)


def call_compress(lib, case, device=None, ens_begin=0, n_ens_out=None, cols=None, storages=None, **over):
    """``iso_binned_compress_host`` on the case's numpy storages or, with ``device``, ``iso_binned_compress`` on copies
    there.  ``cols``: [Q] of (storage number, ncols, col, n_ens, first) instead of the case's placement; ``over``: arguments
    to pass instead of the case's (Q, n_axes, axis_col, n_bins, n_frozen, frozen_col, layout, T, edges).  Returns
    ``(rc, dict)`` of numpy arrays ``A``, ``A2`` [B, S], ``mx``, ``n_bad``, ``n_out`` [S]; what the call does not write keeps
    the fill value -7."""
    S, W, T = case["S"], case["W"], case["T"]
    Q = over.get("Q", case["x"].shape[0])
    B = n_cells(case)
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    up, ptr, host = _mover(device)
    keep = [up(st) for st in (case["storages"] if storages is None else storages)]
    base = [ptr(t).value for t in keep]
    A, A2, mx = up(np.full((B, S), -7.0)), up(np.full((B, S), -7.0)), up(np.full(S, -7.0))
    n_bad, n_out = up(np.full(S, -7, np.int32)), up(np.full(S, -7, np.int32))
    as_bytes = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(-1) if device is not None else np.ascontiguousarray(r)
    interim, frozen = up(as_bytes(case["interim"])), up(as_bytes(case["frozen"]))
    edges = up(np.asarray(over.get("edges", np.concatenate(case["edges"])), dtype=np.float64))
    extra = None if case.get("extra") is None else up(case["extra"])
    mask = None if case.get("mask") is None else up(case["mask"])
    where = [(k, nc, col, S, 0) for k, nc, col in case["where"]] if cols is None else cols
    where = (where + where)[:max(Q, 1)]
    carr = (bc.IsoHierColumn * len(where))(*[bc.IsoHierColumn(base[k], nc, col, n, first) for k, nc, col, n, first in where])
    axis_col = over.get("axis_col", case["axes"])
    n_bins = over.get("n_bins", [len(e) - 1 for e in case["edges"]])
    frozen_col = over.get("frozen_col", case["frozen_cols"])
    fn = lib.iso_binned_compress_host if device is None else lib.iso_binned_compress
    rc = fn(carr, Q, over.get("layout", case["layout"]), over.get("T", T), S, W, ens_begin, n_ens_out, ptr(interim), ptr(frozen),
            over.get("n_frozen", len(frozen_col)), _i32(frozen_col), over.get("n_axes", len(axis_col)), _i32(axis_col),
            _i32(n_bins), ptr(edges), ptr(extra), ptr(mask), ptr(A), ptr(A2), ptr(mx), ptr(n_bad), ptr(n_out), _stream(device))
    return rc, dict(A=host(A), A2=host(A2), mx=host(mx), n_bad=host(n_bad), n_out=host(n_out))


def call_lnlike(lib, tab, lnh, M, mask=None, device=None, ens_begin=0, n_ens_out=None, total=True, B=None):
    """``iso_binned_lnlike_host`` or, with ``device``, ``iso_binned_lnlike`` on copies of the tables ``tab`` (numpy).
    Returns ``(rc, dict)`` of numpy arrays ``ell``, ``ess`` [H, S], ``L``, ``min_ess`` [H]; the fill value is -7."""
    lnh = np.ascontiguousarray(lnh, dtype=np.float64)
    H, S = lnh.shape[0], tab["mx"].shape[0]
    B = lnh.shape[1] if B is None else B
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    up, ptr, host = _mover(device)
    A, A2, mx, dl = up(tab["A"]), up(tab["A2"]), up(tab["mx"]), up(lnh)
    dm = None if mask is None else up(np.ascontiguousarray(mask, dtype=np.int32))
    ell, ess, L, mn = up(np.full((H, S), -7.0)), up(np.full((H, S), -7.0)), up(np.full(H, -7.0)), up(np.full(H, -7.0))
    fn = lib.iso_binned_lnlike_host if device is None else lib.iso_binned_lnlike
    rc = fn(ptr(A), ptr(A2), ptr(mx), B, S, ens_begin, n_ens_out, M, ptr(dl), H, ptr(dm), ptr(ell), ptr(ess),
            ptr(L if total else None), ptr(mn if total else None), _stream(device))
    return rc, dict(ell=host(ell), ess=host(ess), L=host(L), min_ess=host(mn))


def run(lib, case, device=None):
    """Compression and contraction of the whole case: ``(tables, likelihood)``."""
    rc, tab = call_compress(lib, case, device=device)
    assert rc == 0, lib.iso_binned_last_error()
    rc, out = call_lnlike(lib, tab, case["lnh"], case["W"] * case["T"], case.get("mask"), device=device)
    assert rc == 0, lib.iso_binned_last_error()
    return tab, out
