"""A long-double numpy statement of include/isochrones_amd_shrink.h (the per-(star, cell) sums over the hyper rows with the
cell probabilities, and the per-sample weights under a binned population density, libiso_shrink.so), and the one way its
host and device tests call the library.  The cases, the per-sample rule and the tables are tests/_binned_twin.py's.

Both definitions are evaluated from the float64 inputs the library itself was given (A, mx, lnh, ell; mx, lnG), in numpy's
long double: against that every output is within 1e-11 relative (|d| <= 1e-11 max(1, |lnG|) for lnG, a logarithm).  The
float64 implementations carry a few ulp of their exponent's argument, |c - mx| + |lnG| <= some tens here, so 1e-14
relative in a weight, and M * 2^-53 at the very worst in a sum of M <= 4096 terms: below 1e-12, a factor ten inside."""
import ctypes as C

import numpy as np

from isochrones_amd import _reweight_cabi as rc, _shrink_cabi as sc
from tests import _binned_twin as bt

LD = np.longdouble
LIMIT = 1e-11


def cells(A, mx, lnh, ell, mask=None):
    """``(lnG, cellp)`` [B, S] float64 of the header's definition, in long double."""
    A, lnh, ell = np.asarray(A, np.float64), np.asarray(lnh, np.float64), np.asarray(ell, np.float64)
    (B, S), H = A.shape, lnh.shape[0]
    lnG, cellp = np.empty((B, S), LD), np.empty((B, S), LD)
    with np.errstate(all="ignore"):
        for s in range(S):
            for b in range(B):
                live = np.isfinite(ell[:, s]) & ~np.isnan(lnh[:, b]) & ~np.isneginf(lnh[:, b])
                if np.isnan(mx[s]):
                    lnG[b, s] = np.nan
                elif not live.any() or np.isneginf(mx[s]):
                    lnG[b, s] = -np.inf
                else:
                    a = lnh[live, b].astype(LD) - (ell[live, s].astype(LD) - LD(mx[s]))
                    lnG[b, s] = a.max() + np.log(np.exp(a - a.max()).sum())
            pc = np.where(A[:, s] > 0, np.exp(np.log(A[:, s].astype(LD)) + lnG[:, s]), LD(0))
            tot = pc.sum()
            cellp[:, s] = pc / tot if tot > 0 and np.isfinite(tot) else np.nan
        if mask is not None:
            lnG[:, np.asarray(mask) == 0] = cellp[:, np.asarray(mask) == 0] = np.nan
    return lnG.astype(np.float64), cellp.astype(np.float64)


def weights(case, mx, lnG):
    """dict of ``u`` [S, M], ``wsum``, ``ess`` [S] (float64, from long double) and ``n_bad``, ``n_out`` [S] of the header's
    definition for the case's samples under the float64 ``mx`` [S] and ``lnG`` [B, S].  A masked star: NaN and 0."""
    c, cell, bad, out = bt.sample_terms(dict(case, extra=None))
    S, M = c.shape
    u = np.zeros((S, M), LD)
    with np.errstate(all="ignore"):
        for s in range(S):
            use = cell[s] >= 0
            u[s, use] = np.exp((c[s, use] - LD(mx[s])) + np.asarray(lnG, np.float64)[cell[s, use], s].astype(LD))
        wsum = u.sum(axis=1)
        ess = np.where(wsum == 0, LD(0), wsum * wsum / (u * u).sum(axis=1))
    n_bad, n_out = bad.sum(axis=1).astype(np.int32), out.sum(axis=1).astype(np.int32)
    res = dict(u=u.astype(np.float64), wsum=wsum.astype(np.float64), ess=ess.astype(np.float64), n_bad=n_bad, n_out=n_out)
    if case.get("mask") is not None:
        off = np.asarray(case["mask"]) == 0
        res["u"][off], res["wsum"][off], res["ess"][off], n_bad[off], n_out[off] = np.nan, np.nan, np.nan, 0, 0
    return res


def close(got, want, limit=LIMIT, log=False):
    """``got`` against ``want``: NaN and the infinities in the same places, zeros exactly, the rest within ``limit``
    relative (``log``: |d| <= limit * max(1, |want|)).  Returns the largest error over the limit."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    assert np.array_equal(got[fin] == 0, want[fin] == 0)
    scale = np.maximum(1.0, np.abs(want[fin])) if log else np.abs(want[fin])
    err = np.abs(got[fin] - want[fin])
    ok = err <= limit * scale
    worst = float(np.max(err[scale > 0] / (limit * scale[scale > 0]))) if (scale > 0).any() else 0.0
    assert ok.all(), worst
    return worst


# -- the calls --------------------------------------------------------------------------------------------------------
def call_cells(lib, tab, lnh, ell, mask=None, device=None, ens_begin=0, n_ens_out=None, B=None, with_p=True):
    """``iso_shrink_cells_host`` or, with ``device``, ``iso_shrink_cells`` on copies of the numpy inputs.  Returns
    ``(rc, dict)`` of numpy arrays ``lnG``, ``cellp`` [B, S]; the fill value is -7."""
    lnh = np.ascontiguousarray(lnh, dtype=np.float64)
    H, S = lnh.shape[0], tab["mx"].shape[0]
    B = lnh.shape[1] if B is None else B
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    up, ptr, host = bt._mover(device)
    A, mx, dl, de = up(tab["A"]), up(tab["mx"]), up(lnh), up(np.ascontiguousarray(ell, dtype=np.float64))
    dm = None if mask is None else up(np.ascontiguousarray(mask, dtype=np.int32))
    lnG, cellp = up(np.full((max(B, 1), S), -7.0)), up(np.full((max(B, 1), S), -7.0))
    fn = lib.iso_shrink_cells_host if device is None else lib.iso_shrink_cells
    rc_ = fn(ptr(A), ptr(mx), B, S, ens_begin, n_ens_out, ptr(dl), ptr(de), H, ptr(dm), ptr(lnG), ptr(cellp if with_p else None),
             bt._stream(device))
    return rc_, dict(lnG=host(lnG), cellp=host(cellp))


def call_weights(lib, case, mx, lnG, device=None, ens_begin=0, n_ens_out=None, cols=None, storages=None, **over):
    """``iso_shrink_weights_host`` on the case's numpy storages or, with ``device``, ``iso_shrink_weights`` on copies there;
    ``cols``, ``storages`` and ``over`` as tests/_binned_twin.py's call_compress takes them.  Returns ``(rc, dict)`` of numpy
    arrays ``weights`` [n_ens_out, M], ``wsum``, ``ess``, ``n_bad``, ``n_out`` [S]; the fill value is -7."""
    S, W, T = case["S"], case["W"], case["T"]
    Q = over.get("Q", case["x"].shape[0])
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    up, ptr, host = bt._mover(device)
    keep = [up(st) for st in (case["storages"] if storages is None else storages)]
    base = [ptr(t).value for t in keep]
    weights_ = up(np.full((max(n_ens_out, 1), W * T), -7.0))
    wsum, ess = up(np.full(S, -7.0)), up(np.full(S, -7.0))
    n_bad, n_out = up(np.full(S, -7, np.int32)), up(np.full(S, -7, np.int32))
    as_bytes = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(-1) if device is not None else np.ascontiguousarray(r)
    interim, frozen = up(as_bytes(case["interim"])), up(as_bytes(case["frozen"]))
    edges = up(np.asarray(over.get("edges", np.concatenate(case["edges"])), dtype=np.float64))
    dmx, dG = up(np.ascontiguousarray(mx, dtype=np.float64)), up(np.ascontiguousarray(lnG, dtype=np.float64))
    mask = None if case.get("mask") is None else up(case["mask"])
    where = [(k, nc, col, S, 0) for k, nc, col in case["where"]] if cols is None else cols
    where = (where + where)[:max(Q, 1)]
    carr = (sc.IsoHierColumn * len(where))(*[sc.IsoHierColumn(base[k], nc, col, n, first) for k, nc, col, n, first in where])
    axis_col = over.get("axis_col", case["axes"])
    n_bins = over.get("n_bins", [len(e) - 1 for e in case["edges"]])
    frozen_col = over.get("frozen_col", case["frozen_cols"])
    fn = lib.iso_shrink_weights_host if device is None else lib.iso_shrink_weights
    rc_ = fn(carr, Q, over.get("layout", case["layout"]), over.get("T", T), S, W, ens_begin, n_ens_out, ptr(interim),
             ptr(frozen), over.get("n_frozen", len(frozen_col)), bt._i32(frozen_col), over.get("n_axes", len(axis_col)),
             bt._i32(axis_col), bt._i32(n_bins), ptr(edges), ptr(dmx), ptr(dG), ptr(mask), ptr(weights_), ptr(wsum), ptr(ess),
             ptr(n_bad), ptr(n_out), bt._stream(device))
    return rc_, dict(weights=host(weights_), wsum=host(wsum), ess=host(ess), n_bad=host(n_bad), n_out=host(n_out))


def call_summary(rlib, case, values, weights_, probs, device=None, ens_begin=0, n_ens_out=None):
    """``iso_reweight_summary_host`` (``device``: ``iso_reweight_summary``) of the value columns ``values`` (indices into
    the case's columns) under ``weights_`` [n_ens_out, M].  Returns ``(rc, dict)`` of ``mean``, ``sd``, ``n_nan`` [S, V] and
    ``quant`` [S, V, K]; the fill value is -7."""
    S, W, T = case["S"], case["W"], case["T"]
    V, K = len(values), len(probs)
    n_ens_out = S - ens_begin if n_ens_out is None else n_ens_out
    up, ptr, host = bt._mover(device)
    keep = [up(st) for st in case["storages"]]
    base = [ptr(t).value for t in keep]
    carr = (rc.IsoHierColumn * V)(*[rc.IsoHierColumn(base[case["where"][q][0]], case["where"][q][1], case["where"][q][2], S, 0)
                                    for q in values])
    dw = up(np.ascontiguousarray(weights_, dtype=np.float64))
    mask = None if case.get("mask") is None else up(case["mask"])
    mean, sd, quant = up(np.full((S, V), -7.0)), up(np.full((S, V), -7.0)), up(np.full((S, V, K), -7.0))
    n_nan = up(np.full((S, V), -7, np.int32))
    q = np.ascontiguousarray(probs, dtype=np.float64)
    fn = rlib.iso_reweight_summary_host if device is None else rlib.iso_reweight_summary
    rc_ = fn(carr, V, case["layout"], T, S, W, ens_begin, n_ens_out, ptr(mask), q.ctypes.data_as(C.POINTER(C.c_double)), K,
             ptr(dw), ptr(mean), ptr(sd), ptr(quant), ptr(n_nan), bt._stream(device))
    return rc_, dict(mean=host(mean), sd=host(sd), quant=host(quant), n_nan=host(n_nan))


def run(blib, lib, case, device=None):
    """The whole route on the case: the binned library's tables and ``ell``, then the cells and the weights.  Returns
    ``(tables, likelihood, cells, weights)`` as the calls above return them."""
    tab, out = bt.run(blib, case, device=device)
    rc_, cel = call_cells(lib, tab, case["lnh"], out["ell"], case.get("mask"), device=device)
    assert rc_ == 0, lib.iso_shrink_last_error()
    rc_, wts = call_weights(lib, case, tab["mx"], cel["lnG"], device=device)
    assert rc_ == 0, lib.iso_shrink_last_error()
    return tab, out, cel, wts
