"""A long-double numpy statement of include/isochrones_amd_select.h (the detectable fraction of libiso_select.so), the
cases its host and device tests share, and the one way they call the library.

The twin evaluates the family records through tests/_hier_twin.lnf, in numpy's long double (64-bit mantissa), and sums in
numpy's pairwise order.  The limits are those of tests/_hier_twin.py: |d ln_alpha| <= 1e-11 * max(1, max_j |t| / 100) and
n_eff within 1e-10 relative.  (At J <= 3 * 4096 + 5 injections and |t| <= 100: t carries a few ulp of 100, 5e-14; the
J-term sums add J * 2^-53 = 1.4e-12 relative at the very worst, sqrt(J) * 2^-53 = 1.2e-14 typically, and the device's
chunked order no more; the limit leaves a factor of several over the worst case and a thousand over the typical one.)"""
import ctypes as C

import numpy as np

from isochrones_amd import _hier_cabi as hc, _select_cabi as sc, hierarchical as hi, priors as P
from tests import _hier_twin as ht

LD = np.longdouble


def alpha(x, lnd, draw, rows):
    """``x`` [Q, J] float64, ``lnd`` [J], ``draw`` [Q] and ``rows`` [H, Q] records -> dict of float64 arrays ``ln_alpha``,
    ``n_eff`` [H], ``n_bad`` (int) and ``tmax`` [H] (max_j |t| over the good injections with a finite t)."""
    Q, J = x.shape
    H = rows.shape[0]
    ln_alpha, n_eff, tmax = np.empty(H, LD), np.empty(H, LD), np.zeros(H)
    with np.errstate(all="ignore"):
        l0 = [ht.lnf(draw[q], x[q]) for q in range(Q)]
        good = ~np.isnan(lnd) & ~(lnd > 0)
        for q in range(Q):
            good &= ~np.isnan(x[q]) & ~np.isnan(l0[q]) & (l0[q] != -np.inf)
        for h in range(H):
            r = np.zeros(J, LD)
            for q in range(Q):
                lf = ht.lnf(rows[h, q], x[q])
                lf = np.where(np.isnan(lf), LD(-np.inf), lf)
                r = lf - l0[q] if q == 0 else r + (lf - l0[q])
            t = (r + lnd.astype(LD))[good]
            fin = t[np.isfinite(t)]
            if fin.size == 0:
                ln_alpha[h], n_eff[h] = -np.inf, 0
                continue
            mx = t.max()
            w = np.exp(t - mx)
            ln_alpha[h] = mx + np.log(w.sum()) - np.log(LD(J))
            n_eff[h] = w.sum() ** 2 / (w * w).sum()
            tmax[h] = float(np.abs(fin).max())
    return dict(ln_alpha=ln_alpha.astype(np.float64), n_eff=n_eff.astype(np.float64), n_bad=int(J - good.sum()), tmax=tmax)


def assert_matches(got, want, what="", factor=1.0):
    """``got`` against ``want`` within ``factor`` times the limits of the module's docstring; -inf and n_bad exactly."""
    for k in ("ln_alpha", "n_eff"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert not np.isnan(g).any() and not np.isnan(w).any(), (what, k)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(g)], w[np.isinf(w)]), (what, k)
    if "n_bad" in want:
        assert int(got["n_bad"]) == int(want["n_bad"]), (what, got["n_bad"], want["n_bad"])
    fin = np.isfinite(want["ln_alpha"])
    lim = factor * 1e-11 * np.maximum(1.0, want["tmax"] / 100.0)
    d = np.abs(got["ln_alpha"][fin] - want["ln_alpha"][fin])
    assert np.all(d <= lim[fin]), (what, "ln_alpha", float(np.max(d / lim[fin])))
    e = np.abs(got["n_eff"][fin] - want["n_eff"][fin]) / np.maximum(want["n_eff"][fin], 1e-300)
    assert np.all(e <= factor * 1e-10), (what, "n_eff", float(e.max()) if e.size else 0.0)
    assert (got["n_eff"][~fin] == 0.0).all(), what


# -- cases ------------------------------------------------------------------------------------------------------------
def _lnd(rng, J):
    """a mix of certainly detected, undetected and partially detected injections"""
    lnd = np.log(rng.uniform(0.01, 1.0, J))
    u = rng.random(J)
    lnd[u < 0.3] = 0.0
    lnd[u > 0.8] = -np.inf
    return lnd


def random_case(J, Q, H, seed):
    """Q columns of the column types of tests/_hier_twin.py: values, draw records (that module's interim priors), H
    population rows, lnd."""
    rng = np.random.default_rng(seed)
    x = np.empty((Q, J))
    fams, thetas, draw = {}, [], []
    for q in range(Q):
        values, priors, family, theta = ht.COLUMN_TYPES[(q + seed) % len(ht.COLUMN_TYPES)]
        x[q] = values(rng, J)
        draw.append(hi.prior_record(priors[(seed + q) % len(priors)]))
        fams["c%d" % q] = family()
        thetas.append(theta(rng, H))
    rows = hi.PopulationModel(**fams).pack(np.concatenate(thetas, axis=1))
    return dict(x=x, lnd=_lnd(rng, J), draw=np.concatenate(draw), rows=rows)


def fixed_case(x, lnd, draw_priors, row_priors):
    """``x`` [Q, J]; ``draw_priors`` [Q] prior objects or records; ``row_priors`` [H][Q] likewise."""
    rec = lambda p: p if isinstance(p, np.ndarray) else hi.prior_record(p)
    return dict(x=np.ascontiguousarray(x, dtype=np.float64), lnd=np.ascontiguousarray(lnd, dtype=np.float64),
                draw=np.concatenate([rec(p) for p in draw_priors]),
                rows=np.stack([np.concatenate([rec(p) for p in row]) for row in row_priors]))


def kind_case(kind, J=300):
    """Column 0 has ``kind`` as its draw density and a flat population; column 1 a flat draw and ``kind`` as population
    (second row: the power law), on values in (0.2, 3)."""
    rng = np.random.default_rng(kind)
    kinds = ht.all_kinds()
    flat = kinds[hc.FLAT]
    return fixed_case(rng.uniform(0.2, 3.0, (2, J)), _lnd(rng, J), [kinds[kind], flat],
                      [[flat, kinds[kind]], [kinds[hc.POWERLAW], kinds[kind]]])


def special_cases(J=300):
    """name -> case: nothing detected, NaN columns and a draw density of zero (with the same case without them), a row
    without support, t spanning +-700."""
    rng = np.random.default_rng(5)
    out = {}
    flat = P.FlatPrior((-4.0, 4.0))
    gauss = [[P.GaussianPrior(0.0, 1.0), P.GaussianPrior(0.1, 0.7)], [P.FlatPrior((-1.0, 1.0)), P.GaussianPrior(0.0, 2.0)]]
    x = rng.normal(0.0, 0.5, (2, J))
    out["none_detected"] = fixed_case(x, np.full(J, -np.inf), [flat, flat], gauss)
    lnd = _lnd(rng, J)
    out["clean"] = fixed_case(x, lnd, [flat, flat], gauss)
    xb, lb = x.copy(), lnd.copy()
    xb[0, 3] = xb[1, 3] = np.nan                                    # one injection, both columns: counted once
    xb[1, 7] = np.nan
    xb[0, 11] = 5.0                                                 # outside the draw density: bad too
    lb[13], lb[17] = np.nan, 0.25                                   # lnd NaN, lnd positive
    out["bad"] = fixed_case(xb, lb, [flat, flat], gauss)
    keep = np.ones(J, bool)
    keep[[3, 7, 11, 13, 17]] = False
    out["bad_removed"] = (keep, 5)
    x = rng.uniform(1.0, 2.0, (1, J))                               # outside the first row's support
    out["no_support"] = fixed_case(x, _lnd(rng, J), [flat], [[P.FlatPrior((-1.0, 0.9))], [P.GaussianPrior(0.0, 1.0)]])
    x = rng.permutation(np.linspace(0.0, 37.4, J))[None]            # r = x^2 / 2 - (x - 37.4)^2 / 2: -699 .. +699
    out["span_700"] = fixed_case(x, np.zeros(J), [P.GaussianPrior(0.0, 1.0)],
                                 [[P.GaussianPrior(37.4, 1.0)], [P.GaussianPrior(20.0, 1.0)]])
    return out


def want(case):
    if "want" not in case:
        case["want"] = alpha(case["x"], case["lnd"], case["draw"], case["rows"])
    return case["want"]


# -- the call ---------------------------------------------------------------------------------------------------------
def call(lib, case, device=None, rows=None, x_offset=0, guard=False):
    """``iso_select_alpha_host`` on the case's numpy arrays or, with ``device`` (a torch device), ``iso_select_alpha`` on
    copies there (``x_offset``: doubles of padding in front of x, so that it lies at another address).  Returns
    ``(rc, dict)`` of numpy ``ln_alpha``, ``n_eff`` [H] and the int ``n_bad``; what the call does not write keeps -7.  With
    ``guard`` every device output lies between two margins of -7 that have to stay so."""
    rows = case["rows"] if rows is None else rows
    H, Q = rows.shape
    J = case["x"].shape[1]
    x, lnd = np.ascontiguousarray(case["x"]), np.ascontiguousarray(case["lnd"])
    draw, drows = np.ascontiguousarray(case["draw"]), np.ascontiguousarray(rows)
    if device is None:
        la, ne, nb = np.full(H, -7.0), np.full(H, -7.0), np.full(1, -7, np.int32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.iso_select_alpha_host(ptr(x), Q, J, ptr(lnd), ptr(draw), ptr(drows), H, None, ptr(la), ptr(ne), ptr(nb), None)
        return rc, dict(ln_alpha=la, n_eff=ne, n_bad=int(nb[0]))
    import torch
    from isochrones_amd import device as dev
    up = lambda a: torch.from_numpy(a).to(device)
    buf = torch.full((x_offset + x.size,), -3.0, dtype=torch.float64, device=device)
    buf[x_offset:] = up(x.reshape(-1))
    keep = [up(lnd), up(draw.view(np.uint8).reshape(-1)), up(drows.view(np.uint8).reshape(-1))]
    f64 = dict(dtype=torch.float64, device=device)
    ws = torch.full((int(lib.iso_select_workspace_doubles(J, H)),), float("nan"), **f64)
    la, ne = torch.full((H,), -7.0, **f64), torch.full((H,), -7.0, **f64)
    nb = torch.full((1,), -7, dtype=torch.int32, device=device)
    flats = []
    if guard:
        flats, (la, ne, nb) = zip(*[ht.guarded(t.shape, t.dtype, device) for t in (la, ne, nb)])
    ptr = lambda a: C.c_void_p(a.data_ptr())
    rc = lib.iso_select_alpha(C.c_void_p(buf.data_ptr() + 8 * x_offset), Q, J, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), H,
                              ptr(ws), ptr(la), ptr(ne), ptr(nb), dev.stream_ptr(device.index))
    assert all(ht.margins_untouched(f) for f in flats), "a write outside an output"
    return rc, dict(ln_alpha=la.cpu().numpy(), n_eff=ne.cpu().numpy(), n_bad=int(nb.cpu().numpy()[0]))


def one_star_chain(case):
    """The only earlier route to these numbers, for 0/1 detection: the detected injections as the samples of one star
    (W = J_det walkers, one step), the draw densities as its interim priors.  Returns a tests/_hier_twin case and
    ln(J_det / J)."""
    det = case["lnd"] == 0.0
    assert np.all(det | np.isneginf(case["lnd"]))
    x = case["x"][:, det]
    hcase = dict(x=x[:, None, :], interim=case["draw"], rows=case["rows"], S=1, W=int(det.sum()), T=1,
                 layout=1, mask=None, storages=[np.ascontiguousarray(x[None])], where=[(0, x.shape[0], q) for q in range(x.shape[0])])
    return hcase, float(np.log(det.sum() / det.size))
