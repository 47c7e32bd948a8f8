"""Maximum-likelihood fits of a binned population (a :class:`~isochrones_amd.binned.Histogram`, optionally ``given=``): the
expected number of stars per cell and its pair sums (``iso_binfit_moments``, libiso_binfit.so,
include/isochrones_amd_binfit.h), the derivatives of ``lnlike`` with respect to the hyper-parameters built on them, and an
EM iteration with Laplace error bars.  All of it works on the per-star tables
:meth:`~isochrones_amd.hierarchical.PopulationPosterior.bin_tables` holds; the chain is not read again.

With the log cell densities ``lnh`` as coordinates, ``d lnlike / d lnh_b = N_b - S_u q_b`` and the second derivative is
``diag(N) - C - S_u (diag(q) - q q^T)``: ``N`` and ``C`` are the two moments over the stars, ``q`` the first moment of the
injection set's one-star table (0 without one), ``S_u`` the number of unmasked stars.  The chain rule to the logits goes
through the ``log_softmax`` of every histogram (:func:`softmax_blocks`); it is host arithmetic on at most 64 x 63 numbers
per row.

EM.  The mean weight of a star is linear in the cell masses, so ``masses <- N / sum(N)`` raises the likelihood at every
step.  With an injection set the substitution ``g_b = h_b a_b / alpha`` (the distribution of the detected stars; ``a_b``
the injection table) turns every star's term into a simplex mixture in ``g`` with the same ``N``, so ``g <- N / sum(N)``
and ``h proportional to g / a``, renormalised to unit mass.  DESIGN.md section 24 has the derivation and what is refused."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _binfit_cabi as fc, device as dev


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else dev.ptr(a)


def _need_binned(post, what):
    if not post.model.binned:
        raise ValueError("%s needs a population model with a Histogram column: only a binned density has cells to count "
                         "stars in" % what)


def _rows(theta):
    """``theta`` as numpy [H, P], and whether it came as a tensor."""
    as_tensor = dev.is_tensor(theta)
    th = np.atleast_2d(theta.detach().cpu().numpy() if as_tensor else np.asarray(theta, dtype=np.float64))
    return np.ascontiguousarray(th, dtype=np.float64), as_tensor


def moments(A, lnh, mask=None, pairs=False, device=None):
    """``iso_binfit_moments`` on a table ``A`` [B, n] (a CUDA tensor on ``device``, or numpy with ``device=None``: the host
    entry) under the numpy rows ``lnh`` [H, B].  Returns numpy ``(N [H, B], C [H, B, B] or None, n_live [H])``."""
    lnh = np.ascontiguousarray(lnh, dtype=np.float64)
    H, B = lnh.shape
    n = A.shape[1]
    if A.shape[0] != B:
        raise ValueError("the table has %d cells, the rows %d" % (A.shape[0], B))
    lib = fc.lib()
    if device is None:
        N, Cm, live = np.empty((H, B)), (np.empty((H, B, B)) if pairs else None), np.empty(H, dtype=np.int32)
        fc.check(lib.iso_binfit_moments_host(_ptr(A), B, n, _ptr(lnh), H, _ptr(mask), _ptr(N), _ptr(Cm), _ptr(live), None,
                                             None))
        return N, Cm, live
    import torch
    f64 = dict(dtype=torch.float64, device=device)
    N, Cm = torch.empty(H, B, **f64), (torch.empty(H, B, B, **f64) if pairs else None)
    live = torch.empty(H, dtype=torch.int32, device=device)
    ws = torch.empty(int(lib.iso_binfit_workspace_doubles(B, n, H, int(pairs))), **f64)
    dl = torch.from_numpy(lnh).to(device)
    fc.check(lib.iso_binfit_moments(_ptr(A), B, n, _ptr(dl), H, _ptr(mask), _ptr(N), _ptr(Cm), _ptr(live), _ptr(ws),
                                    dev.stream_ptr(device.index)))
    return N.cpu().numpy(), (Cm.cpu().numpy() if pairs else None), live.cpu().numpy()


def _star_moments(post, lnh, pairs):
    A = post.bin_tables()[0]
    if post.host:
        return moments(A, lnh, post.mask, pairs)
    return moments(A, lnh, post._device_state()["mask"], pairs, device=post.storage.device)


def _selection_q(post, lnh):
    """``q`` [H, B] of the injection set's one-star table, or None without a set."""
    if post.selection is None:
        return None
    return moments(post.selection.tables[0], lnh, None, False, device=post.selection.device)[0]


def _back(as_tensor, theta, *arrays):
    if as_tensor:
        import torch
        return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(theta.device) for a in arrays)
    return arrays


def cell_counts(post, theta, pairs=False):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.cell_counts`."""
    _need_binned(post, "cell_counts")
    th, as_tensor = _rows(theta)
    N, Cm, live = _star_moments(post, post.model.cell_table(th)["lnh"], pairs)
    out = _back(as_tensor, theta, N, Cm, live)
    return out if pairs else (out[0], out[2])


# -- the chain rule to the logits -------------------------------------------------------------------------------------
def softmax_blocks(model):
    """The softmaxes behind a binned model's ``lnh``: a list of ``(idx [K - 1], member [K, B])``, one per histogram and
    parent bin.  ``idx`` are the block's logits among the hyper-parameters (bin 0's logit is the constant 0); ``member[k,
    b]`` is 1 where cell ``b`` takes its log density from bin ``k`` of the block.  ``lnh_b`` is the sum over the blocks of
    ``log_softmax(a)[bin of b]`` minus the log cell volume."""
    shape = tuple(len(model.families[q].edges) - 1 for q in model.axes)
    B = int(np.prod(shape))
    cell = np.arange(B).reshape(shape)
    start = np.concatenate([[0], np.cumsum([len(f.names) for f in model.families])]).astype(int)
    blocks = []
    for a, q in enumerate(model.axes):
        fam = model.families[q]
        K = fam.n_bins
        for r in range(fam.parent_bins):
            idx = start[q] + r * (K - 1) + np.arange(K - 1)
            member = np.zeros((K, B))
            for k in range(K):
                sel = [slice(None)] * len(shape)
                sel[a] = k
                if fam.given is not None:
                    sel[0] = r
                member[k, cell[tuple(sel)].reshape(-1)] = 1.0
            blocks.append((idx, member))
    return blocks


def _chain_rule(blocks, theta, g, Hl):
    """One row: the gradient [P] and, with ``Hl`` [B, B], the Hessian [P, P] with respect to the hyper-parameters from the
    gradient ``g`` [B] and the Hessian ``Hl`` with respect to ``lnh``."""
    P, B = theta.size, g.size
    G = np.zeros((B, P))
    second = np.zeros((P, P))
    for idx, member in blocks:
        a = np.concatenate([[0.0], theta[idx]])
        e = np.exp(a - a.max())
        pi = e / e.sum()
        used = member.sum(axis=0)                               # 1 for the cells that take a bin of this block
        G[:, idx] = (member.T - used[:, None] * pi[None, :])[:, 1:]
        # d^2 log_softmax_k / da_j da_l = -(delta_jl pi_j - pi_j pi_l), whatever k: weighted by the block's share of g
        second[np.ix_(idx, idx)] -= (g * used).sum() * (np.diag(pi) - np.outer(pi, pi))[1:, 1:]
    grad = G.T @ g
    return grad, (None if Hl is None else G.T @ Hl @ G + second), G


def _lnh_derivatives(post, lnh, second):
    """``(N [H, B], g [H, B], Hl [H, B, B] or None)`` under the numpy rows ``lnh``: the expected counts, and the gradient and
    (with ``second``) the Hessian of ``lnlike`` with respect to ``lnh``, the selection term of an injection set included."""
    N, Cm, _ = _star_moments(post, lnh, second)
    q = _selection_q(post, lnh)
    Su = post.n_unmasked
    g = N if q is None else N - Su * q
    Hl = None
    if second:
        Hl = np.stack([np.diag(n) for n in N]) - Cm
        if q is not None:
            Hl = Hl - Su * (np.stack([np.diag(r) for r in q]) - q[:, :, None] * q[:, None, :])
    return N, g, Hl


def _derivatives(post, th, second):
    _, g, Hl = _lnh_derivatives(post, post.model.cell_table(th)["lnh"], second)
    blocks = softmax_blocks(post.model)
    H, P = th.shape
    grads, hess = np.empty((H, P)), (np.empty((H, P, P)) if second else None)
    for h in range(H):
        grads[h], hh, _ = _chain_rule(blocks, th[h], g[h], Hl[h] if second else None)
        if second:
            hess[h] = hh
    return grads, hess


def grad(post, theta):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.grad`."""
    _need_binned(post, "grad")
    th, as_tensor = _rows(theta)
    return _back(as_tensor, theta, _derivatives(post, th, False)[0])[0]


def hessian(post, theta):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.hessian`."""
    _need_binned(post, "hessian")
    th, as_tensor = _rows(theta)
    return _back(as_tensor, theta, _derivatives(post, th, True)[1])[0]


# -- EM ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BinnedFit:
    """What :meth:`~isochrones_amd.hierarchical.PopulationPosterior.maximize` returns.  ``theta`` [P]: the hyper-parameters
    at the maximum; ``lnlike`` there; ``n_iter`` EM steps taken; ``converged``; ``trace``: the objective at the start and
    after every step; ``on_bound``: the names of the logits held at an end of their range.  ``masses``, ``density``,
    ``mass_sd``, ``expected`` (the expected number of stars per cell): in the grid's shape.  ``cov`` [P, P]: the Laplace
    covariance of the logits, NaN for those on a bound."""
    theta: np.ndarray
    lnlike: float
    n_iter: int
    converged: bool
    trace: np.ndarray
    on_bound: tuple
    masses: np.ndarray
    density: np.ndarray
    cov: np.ndarray
    mass_sd: np.ndarray
    expected: np.ndarray
    edges: tuple
    columns: tuple
    param_names: tuple

    def frame(self):
        """A DataFrame with one row per cell: its indices ``k<axis>``, its edges ``<column>_lo``, ``<column>_hi``, ``mass``,
        ``mass_sd``, ``density`` and ``expected``."""
        import pandas as pd
        shape = self.masses.shape
        ks = np.indices(shape).reshape(len(shape), -1)
        data = {}
        for a, (col, e) in enumerate(zip(self.columns, self.edges)):
            data["k%d" % a] = ks[a]
            data["%s_lo" % col], data["%s_hi" % col] = e[ks[a]], e[ks[a] + 1]
        for name in ("mass", "mass_sd", "density", "expected"):
            data[name] = getattr(self, "masses" if name == "mass" else name).reshape(-1)
        return pd.DataFrame(data)


def _volumes(model):
    widths = [np.diff(model.families[q].edges) for q in model.axes]
    return widths[0] if len(widths) == 1 else widths[0][:, None] * widths[1][None, :]


def _logits(pi, lo, hi):
    """The logits ``a_1 .. a_{K-1}`` (``a_0 = 0``) of the probabilities ``pi``, held inside ``[lo, hi]`` by flooring masses,
    not by clipping logits one by one: bin 0 is no lighter than ``exp(-hi)`` of the heaviest bin (clipping every logit to
    ``hi`` instead would make all the other bins equal), and no other bin lighter than ``exp(lo)`` of bin 0.  A floored bin's
    logit is set to the bound itself, not computed from the floored mass, so that it is on the bound to the last bit."""
    top = pi.max()
    raised = pi[0] < top * np.exp(-hi)
    m0 = top * np.exp(-hi) if raised else pi[0]
    if not m0 > 0:
        return np.zeros(pi.size - 1)
    low = pi[1:] < m0 * np.exp(lo)
    a = np.where(low, lo, np.log(np.where(low, 1.0, pi[1:])) - np.log(m0))
    return np.where(pi[1:] == top, hi, a) if raised else a


def _m_step(post, theta, N, a_sel):
    """The hyper-parameters that maximise the expected complete-data likelihood of the counts ``N`` [B], with the masses
    floored where a logit would leave its range (:func:`_logits`)."""
    model = post.model
    fams = [model.families[q] for q in model.axes]
    shape = tuple(f.n_bins for f in fams)
    start = np.concatenate([[0], np.cumsum([len(f.names) for f in model.families])]).astype(int)
    m = N / N.sum()
    if a_sel is not None:
        if np.any((a_sel <= 0) & (N > 0)):
            raise ValueError("a cell that no detected injection covers holds %.3g expected stars: its height has no "
                             "maximum-likelihood value (widen the injection set or merge the bin)"
                             % N[(a_sel <= 0) & (N > 0)].max())
        vol = _volumes(model).reshape(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(N > 0, vol * m / a_sel, 0.0)
        m = m / m.sum()
    m = m.reshape(shape)
    new = theta.copy()
    if len(fams) == 1:
        new[start[model.axes[0]]:start[model.axes[0] + 1]] = _logits(m, *fams[0].logits)
        return new
    q0, q1 = model.axes
    if fams[1].given is None:                                   # independent axes: each takes the counts' marginal
        new[start[q0]:start[q0 + 1]] = _logits(m.sum(axis=1), *fams[0].logits)
        new[start[q1]:start[q1 + 1]] = _logits(m.sum(axis=0), *fams[1].logits)
        return new
    parent = m.sum(axis=1)
    new[start[q0]:start[q0 + 1]] = _logits(parent, *fams[0].logits)
    K1 = shape[1]
    for r in range(shape[0]):
        if parent[r] > 0:                                       # an empty parent bin says nothing of its conditional
            new[start[q1] + r * (K1 - 1):start[q1] + (r + 1) * (K1 - 1)] = _logits(m[r] / parent[r], *fams[1].logits)
    return new


def maximize(post, theta0=None, max_iter=2000, tol=1e-8, errors=True):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.maximize`."""
    _need_binned(post, "maximize")
    model = post.model
    P = model.n_params
    if P < 1:
        raise ValueError("the population model has no free parameter")
    independent = len(model.axes) == 2 and model.families[model.axes[1]].given is None
    if independent and post.selection is not None:
        raise ValueError("two independent Histograms with an injection set have no closed-form M-step: the detectable "
                         "fraction of a cell is no product of the axes' (fit the second with given=, or without injections)")
    lo, hi = model.ranges[:, 0], model.ranges[:, 1]
    theta = np.zeros(P) if theta0 is None else np.array(theta0, dtype=np.float64).reshape(-1)
    if theta.size != P:
        raise ValueError("theta0 must be one row of %d hyper-parameters (%s)" % (P, ", ".join(model.param_names)))
    theta = np.clip(theta, lo, hi)
    a_sel = None
    if post.selection is not None:
        t = post.selection.tables[0]
        a_sel = (t.cpu().numpy() if dev.is_tensor(t) else np.asarray(t)).reshape(-1)
    value = lambda th: float(np.asarray(post.lnlike(th[None, :]))[0])
    L = value(theta)
    trace, converged, n_iter = [L], False, 0
    clipped = np.zeros(P, dtype=bool)
    for n_iter in range(1, int(max_iter) + 1):
        N = _star_moments(post, model.cell_table(theta[None, :])["lnh"], False)[0][0]
        if not N.sum() > 0:
            raise ValueError("no star has weight under the current heights: nothing to fit")
        raw = _m_step(post, theta, N, a_sel)
        new = np.clip(raw, lo, hi)                              # a floored logit is the bound itself; the rest is rounding
        new_clipped = (new <= lo) | (new >= hi)
        Ln = value(new)
        trace.append(Ln)
        rise = Ln - L
        theta, L, clipped = new, Ln, new_clipped
        # a clipped step may lower the objective; the clipped iteration has converged once it stands still
        if rise < tol and (abs(rise) < tol or not clipped.any()):
            converged = True
            break
    trace = np.array(trace)
    table = model.cell_table(theta[None, :])
    shape = tuple(len(e) - 1 for e in table["edges"])
    vol = _volumes(model)
    density = np.exp(table["lnh"][0]).reshape(shape)
    masses = density * vol
    N, g, Hl = _lnh_derivatives(post, table["lnh"], errors)
    cov = np.full((P, P), np.nan)
    mass_sd = np.full(shape, np.nan)
    if errors:
        _, hess, G = _chain_rule(softmax_blocks(model), theta, g[0], Hl[0])
        free = np.flatnonzero(~clipped)
        if free.size:
            info = -hess[np.ix_(free, free)]
            try:
                singular = not np.isfinite(info).all() or np.linalg.cond(info) > 1.0 / np.finfo(float).eps
                sub = np.linalg.pinv(info) if singular else np.linalg.inv(info)
            except np.linalg.LinAlgError:
                sub = np.linalg.pinv(info)
            cov[np.ix_(free, free)] = sub
            J = masses.reshape(-1, 1) * G[:, free]              # d mass_b / d logit: ln mass_b = lnh_b + ln volume_b
            var = np.einsum("bi,ij,bj->b", J, sub, J)
            mass_sd = np.sqrt(np.maximum(var, 0.0)).reshape(shape)
    return BinnedFit(theta=theta, lnlike=L, n_iter=n_iter, converged=converged, trace=trace,
                     on_bound=tuple(n for n, c in zip(model.param_names, clipped) if c), masses=masses, density=density,
                     cov=cov, mass_sd=mass_sd, expected=N[0].reshape(shape), edges=tuple(table["edges"]),
                     columns=tuple(model.columns[q] for q in model.axes), param_names=tuple(model.param_names))
