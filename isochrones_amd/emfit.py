"""Bootstrap errors for a binned population (a :class:`~isochrones_amd.binned.Histogram`, optionally ``given=``): a batch
of weighted EM fits of the cell masses with the whole iteration on the device, one workgroup per replicate
(``iso_emfit_run``, libiso_emfit.so, include/isochrones_amd_emfit.h), and the star weights of the replicates
(``iso_emfit_weights``).  All of it works on the per-star tables
:meth:`~isochrones_amd.hierarchical.PopulationPosterior.bin_tables` holds; the chain is not read again.

A replicate iterates :mod:`isochrones_amd.binfit`'s EM step, ``g <- N / sum(N)``, under a weight per star: ``g`` are the
cell masses and ``scale = 1 / cell volume`` without an injection set; with one, ``g_b = h_b a_b / alpha`` is the
distribution of the detected stars (``a_b`` the injection table) and ``scale = 1 / a``, 0 where no detected injection
covers the cell.  Resampling the stars (Poisson(1) counts, or the exponential weights of the Bayesian bootstrap) and
fitting again gives errors that hold where the maximum lies on the boundary of the simplex, which is where the Laplace
covariance of :meth:`~isochrones_amd.hierarchical.PopulationPosterior.maximize` is NaN.  DESIGN.md section 25 has the
derivation and what is refused."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _emfit_cabi as ec, binfit, device as dev

STATUS_NAMES = {ec.RUNNING: "running", ec.CONVERGED: "converged", ec.MAX_ITER: "max_iter", ec.EMPTY: "empty"}
_KINDS = {"poisson": ec.POISSON, "bayesian": ec.EXP}
_ptr = binfit._ptr


def _need_free_masses(post, what):
    binfit._need_binned(post, what)
    model = post.model
    if len(model.axes) == 2 and model.families[model.axes[1]].given is None:
        raise ValueError("%s takes one Histogram, or a second one with given=: the density of two independent Histograms is a "
                         "product of the axes' and has no free joint masses to iterate on" % what)


def _selection_table(post):
    """``a`` [B] of the injection set's one-star table, or None without a set."""
    if post.selection is None:
        return None
    t = post.selection.tables[0]
    return (t.cpu().numpy() if dev.is_tensor(t) else np.asarray(t)).reshape(-1).astype(np.float64)


def _scale(post):
    a = _selection_table(post)
    if a is None:
        return 1.0 / binfit._volumes(post.model).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a > 0, 1.0 / a, 0.0)


def start_masses(post, theta):
    """``g0`` [B] of one row ``theta`` [P]: the cell masses of its density, or with an injection set the distribution of the
    detected stars under it, ``h_b a_b / alpha``."""
    table = post.model.cell_table(np.asarray(theta, dtype=np.float64).reshape(1, -1))
    h = np.exp(table["lnh"][0])
    a = _selection_table(post)
    g = h * binfit._volumes(post.model).reshape(-1) if a is None else h * np.maximum(a, 0.0)
    return g / g.sum()


def _check_covered(post, theta):
    """``maximize``'s refusal of a cell that no detected injection covers and that holds expected stars under ``theta``."""
    a = _selection_table(post)
    if a is None or not np.any(a <= 0):
        return
    N = np.asarray(binfit.cell_counts(post, np.asarray(theta, dtype=np.float64).reshape(1, -1))[0])[0]
    bad = (a <= 0) & (N > 0)
    if np.any(bad):
        raise ValueError("a cell that no detected injection covers holds %.3g expected stars: its height has no "
                         "maximum-likelihood value (widen the injection set or merge the bin)" % N[bad].max())


def star_weights(kind, seed, first, R, S, device=None):
    """``iso_emfit_weights``: the weights [R, S] of the replicates ``first .. first + R - 1`` (a CUDA tensor on ``device``, or
    numpy with ``device=None``: the host entry).  ``kind``: "poisson" or "bayesian"."""
    lib = ec.lib()
    if device is None:
        out = np.empty((R, S))
        ec.check(lib.iso_emfit_weights_host(_KINDS[kind], C.c_uint64(seed), first, R, S, _ptr(out), None))
        return out
    import torch
    out = torch.empty(R, S, dtype=torch.float64, device=device)
    ec.check(lib.iso_emfit_weights(_KINDS[kind], C.c_uint64(seed), first, R, S, _ptr(out), dev.stream_ptr(device.index)))
    return out


def run(A, scale, w, mask, g0, R, max_iter, tol, device=None, steps_per_launch=0):
    """``iso_emfit_run`` on a table ``A`` [B, n] (a CUDA tensor on ``device``, or numpy with ``device=None``: the host
    entry).  ``scale`` [B] and ``g0`` ([B] shared, or [R, B]) are numpy; ``w`` [R, n] and ``mask`` [n] lie where ``A``
    does, or are None.  Returns numpy ``(g [R, B], objective, n_iter, status, n_live, wsum)``."""
    B, n = A.shape
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    g0 = np.ascontiguousarray(g0, dtype=np.float64)
    if scale.shape != (B,) or g0.shape not in ((B,), (R, B)):
        raise ValueError("the table has %d cells: scale must be [%d] and g0 [%d] or [%d, %d]" % (B, B, B, R, B))
    stride = B if g0.ndim == 2 else 0
    lib = ec.lib()
    if device is None:
        g, obj, wsum = np.empty((R, B)), np.empty(R), np.empty(R)
        n_iter, status, live = (np.empty(R, dtype=np.int32) for _ in range(3))
        ec.check(lib.iso_emfit_run_host(_ptr(A), B, n, _ptr(scale), _ptr(w), R, _ptr(mask), _ptr(g0), stride, int(max_iter),
                                        float(tol), int(steps_per_launch), _ptr(g), _ptr(obj), _ptr(n_iter), _ptr(status),
                                        _ptr(live), _ptr(wsum), None))
        return g, obj, n_iter, status, live, wsum
    import torch
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    ds, dg0 = torch.from_numpy(scale).to(device), torch.from_numpy(g0).to(device)
    g, obj, wsum = torch.empty(R, B, **f64), torch.empty(R, **f64), torch.empty(R, **f64)
    n_iter, status, live = (torch.empty(R, **i32) for _ in range(3))
    ec.check(lib.iso_emfit_run(_ptr(A), B, n, _ptr(ds), _ptr(w), R, _ptr(mask), _ptr(dg0), stride, int(max_iter), float(tol),
                               int(steps_per_launch), _ptr(g), _ptr(obj), _ptr(n_iter), _ptr(status), _ptr(live), _ptr(wsum),
                               dev.stream_ptr(device.index)))
    return tuple(t.cpu().numpy() for t in (g, obj, n_iter, status, live, wsum))


def _where(post):
    """``(A, mask, device)`` of the posterior's table: the device is None for a host chain."""
    A = post.bin_tables()[0]
    if post.host:
        return A, post.mask, None
    return A, post._device_state()["mask"], post.storage.device


def em_masses(post, weights=None, g0=None, max_iter=2000, tol=1e-8):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.em_masses`."""
    _need_free_masses(post, "em_masses")
    A, mask, device = _where(post)
    B, S = A.shape
    zeros = np.zeros(post.model.n_params)
    _check_covered(post, zeros)
    w, R = None, 1
    if weights is not None:
        w = np.ascontiguousarray(weights.detach().cpu().numpy() if dev.is_tensor(weights) else weights, dtype=np.float64)
        if w.ndim != 2 or w.shape[1] != S:
            raise ValueError("weights must be [R, %d]: one row per replicate, one weight per star" % S)
        if not np.all(np.isfinite(w) & (w >= 0)):
            raise ValueError("weights must be finite and not negative")
        R = w.shape[0]
    g0 = start_masses(post, zeros) if g0 is None else np.asarray(g0, dtype=np.float64)
    if g0.ndim == 2:
        R = g0.shape[0] if weights is None else R
    if not (np.all(np.isfinite(g0) & (g0 >= 0)) and np.all(g0.sum(axis=-1) > 0)):
        raise ValueError("g0 must be finite, not negative, and every row must sum to something above 0")
    if w is not None and device is not None:
        import torch
        w = torch.from_numpy(w).to(device)
    return run(A, _scale(post), w, mask, g0, R, max_iter, tol, device=device)[:5]


@dataclasses.dataclass
class BinnedBootstrap:
    """What :meth:`~isochrones_amd.hierarchical.PopulationPosterior.bootstrap` returns.  Row 0 of every per-replicate field is
    the unweighted fit (``point_masses``, ``point_density``), rows 1 .. ``n_boot`` the replicates.  ``masses``, ``density``
    [R, grid]; ``theta`` [R, P]: a replicate's hyper-parameters (a row goes into ``star_posteriors`` as a hyper row);
    ``n_iter``, ``status`` (``isochrones_amd.emfit.STATUS_NAMES``), ``objective``, ``n_live`` [R].  Over the replicates
    that are not empty, in the grid's shape: ``mass_mean``, ``mass_sd`` (ddof = 1) and ``mass_q`` [len(q), grid], the
    quantiles ``q``.  An empty replicate (no star with weight) has NaN masses."""
    masses: np.ndarray
    density: np.ndarray
    theta: np.ndarray
    n_iter: np.ndarray
    status: np.ndarray
    objective: np.ndarray
    n_live: np.ndarray
    point_masses: np.ndarray
    point_density: np.ndarray
    mass_mean: np.ndarray
    mass_sd: np.ndarray
    mass_q: np.ndarray
    q: tuple
    n_boot: int
    seed: int
    weights: str
    edges: tuple
    columns: tuple
    param_names: tuple

    def frame(self):
        """A DataFrame with one row per cell: its indices ``k<axis>``, its edges ``<column>_lo``, ``<column>_hi``, ``mass``
        (the unweighted fit), ``mass_mean``, ``mass_sd``, one ``mass_q<100 q>`` per quantile and ``density``."""
        import pandas as pd
        shape = self.point_masses.shape
        ks = np.indices(shape).reshape(len(shape), -1)
        data = {}
        for a, (col, e) in enumerate(zip(self.columns, self.edges)):
            data["k%d" % a] = ks[a]
            data["%s_lo" % col], data["%s_hi" % col] = e[ks[a]], e[ks[a] + 1]
        data["mass"] = self.point_masses.reshape(-1)
        data["mass_mean"], data["mass_sd"] = self.mass_mean.reshape(-1), self.mass_sd.reshape(-1)
        for k, qq in enumerate(self.q):
            data["mass_q%g" % (100 * qq)] = self.mass_q[k].reshape(-1)
        data["density"] = self.point_density.reshape(-1)
        return pd.DataFrame(data)


def bootstrap(post, theta0=None, n_boot=200, seed=0, weights="poisson", q=(0.16, 0.5, 0.84), max_iter=2000, tol=1e-8):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.bootstrap`."""
    _need_free_masses(post, "bootstrap")
    model = post.model
    P = model.n_params
    A, mask, device = _where(post)
    B, S = A.shape
    given = None
    if not isinstance(weights, str):
        given = np.ascontiguousarray(weights.detach().cpu().numpy() if dev.is_tensor(weights) else weights, dtype=np.float64)
        if given.ndim != 2 or given.shape[1] != S:
            raise ValueError("weights must be \"poisson\", \"bayesian\" or an array [R, %d]" % S)
        if not np.all(np.isfinite(given) & (given >= 0)):
            raise ValueError("weights must be finite and not negative")
        n_boot = given.shape[0]
    elif weights not in _KINDS:
        raise ValueError("weights must be \"poisson\", \"bayesian\" or an array [R, %d]" % S)
    n_boot = int(n_boot)
    if n_boot < 2:
        raise ValueError("n_boot must be at least 2: a standard deviation needs two replicates")
    lo, hi = model.ranges[:, 0], model.ranges[:, 1]
    theta0 = np.zeros(P) if theta0 is None else np.array(theta0, dtype=np.float64).reshape(-1)
    if theta0.size != P:
        raise ValueError("theta0 must be one row of %d hyper-parameters (%s)" % (P, ", ".join(model.param_names)))
    theta0 = np.clip(theta0, lo, hi)
    _check_covered(post, theta0)
    g0, scale = start_masses(post, theta0), _scale(post)
    R = n_boot + 1
    per = max(1, int(post.budget) // (8 * S))                           # replicates whose weights stay inside the budget
    parts = []
    for r0 in range(0, R, per):
        n = min(per, R - r0)
        if given is None:
            w = star_weights(weights, int(seed), r0, n, S, device)
            if r0 == 0:
                w[0] = 1.0
        else:
            w = np.ones((n, S))
            w[max(1 - r0, 0):] = given[max(r0 - 1, 0):r0 - 1 + n]
            if device is not None:
                import torch
                w = torch.from_numpy(w).to(device)
        parts.append(run(A, scale, w, mask, g0, n, max_iter, tol, device=device))
    g, objective, n_iter, status, n_live, _ = (np.concatenate([p[k] for p in parts]) for k in range(6))
    a = _selection_table(post)
    vol = binfit._volumes(model)
    shape = vol.shape
    masses, theta = np.full((R, B), np.nan), np.full((R, P), np.nan)
    for r in np.flatnonzero(status != ec.EMPTY):
        m = g[r]
        if a is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                m = np.where(m > 0, vol.reshape(-1) * m / a, 0.0)
        masses[r] = m / m.sum()
        theta[r] = np.clip(binfit._m_step(post, theta0, g[r], a), lo, hi)
    masses = masses.reshape((R,) + shape)
    density = masses / vol
    ok = np.flatnonzero(status[1:] != ec.EMPTY) + 1
    qs = tuple(float(x) for x in q)
    if ok.size >= 2:
        mean, sd = masses[ok].mean(axis=0), masses[ok].std(axis=0, ddof=1)
        mq = np.quantile(masses[ok], qs, axis=0)
    else:
        mean, sd, mq = np.full(shape, np.nan), np.full(shape, np.nan), np.full((len(qs),) + shape, np.nan)
    edges = tuple(model.cell_table(theta0[None, :])["edges"])
    return BinnedBootstrap(masses=masses, density=density, theta=theta, n_iter=n_iter, status=status, objective=objective,
                           n_live=n_live, point_masses=masses[0], point_density=density[0], mass_mean=mean, mass_sd=sd,
                           mass_q=mq, q=qs, n_boot=n_boot, seed=int(seed), weights=weights if given is None else "given",
                           edges=edges, columns=tuple(model.columns[k] for k in model.axes),
                           param_names=tuple(model.param_names))
