"""A long-double numpy statement of include/isochrones_amd_binfit.h (the expected number of stars per cell, the pair sums
and the live count under a binned population density, libiso_binfit.so), of the likelihood they differentiate and of its
gradient and Hessian with respect to the logits through an analytic log_softmax Jacobian; the case builders; and the one
way the host and device tests call the library.

The moments are evaluated from the float64 inputs the library itself was given (A, lnh), in numpy's long double: against
that N and C are within 1e-11 relative to max(1, n_live).  A float64 p carries a few ulp (one exp, a sum of at most 64
products, one division), so a sum of n_live of them is off by some n_live * 1e-15 at the very worst: a factor 10^4
inside."""
import numpy as np

from tests import _binned_twin as bt
from tests._hier_twin import guarded, margins_untouched

LD = np.longdouble
LIMIT = 1e-11


# -- the definition ---------------------------------------------------------------------------------------------------
def heights(lnh):
    """u [H, B] in long double: exp(lnh - hmx), 0 for -inf and NaN."""
    lnh = np.asarray(lnh, np.float64)
    with np.errstate(all="ignore"):
        clean = np.where(np.isnan(lnh), -np.inf, lnh).astype(LD)
        hmx = clean.max(axis=1, keepdims=True)
        return np.where(np.isneginf(clean), LD(0), np.exp(clean - hmx))


def moments(A, lnh, mask=None):
    """dict of ``N`` [H, B], ``C`` [H, B, B] (long double) and ``n_live`` [H] of the header's definition."""
    A = np.asarray(A, np.float64).astype(LD)
    u = heights(lnh)
    (H, B), S = u.shape, A.shape[1]
    N, Cm, n_live = np.zeros((H, B), LD), np.zeros((H, B, B), LD), np.zeros(H, np.int32)
    on = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
    for h in range(H):
        ua = u[h][:, None] * A                                      # [B, S]
        s1 = ua.sum(axis=0)
        live = on & (s1 > 0)
        p = ua[:, live] / s1[live]
        N[h], Cm[h], n_live[h] = p.sum(axis=1), p @ p.T, live.sum()
    return dict(N=N, C=Cm, n_live=n_live)


def lnL(A, lnh, mask=None, a_sel=None):
    """The long-double objective of one row ``lnh`` [B] up to a constant: the sum over the live stars of ln sum_b exp(lnh_b)
    A[b][s], minus (with ``a_sel`` [B], the one-star injection table) S_unmasked ln sum_b exp(lnh_b) a_b."""
    A = np.asarray(A, np.float64).astype(LD)
    h = np.exp(np.asarray(lnh).astype(LD))
    on = np.ones(A.shape[1], bool) if mask is None else np.asarray(mask) != 0
    s1 = (h[:, None] * A).sum(axis=0)
    live = on & (s1 > 0)
    out = np.log(s1[live]).sum()
    if a_sel is not None:
        out = out - LD(on.sum()) * np.log((h * np.asarray(a_sel, np.float64).astype(LD)).sum())
    return out


# -- the three model shapes -------------------------------------------------------------------------------------------
def blocks(shape):
    """``shape``: ("one", K), ("given", K0, K1) or ("indep", K0, K1), with the parent's (axis 0's) logits first among the
    hyper-parameters.  Returns ``(P, B, [(idx, cells)])``: per softmax its logits' indices [K - 1] and ``cells`` [K]: the
    list of cells that take their log density from each of its bins."""
    kind, K0 = shape[0], shape[1]
    if kind == "one":
        return K0 - 1, K0, [(np.arange(K0 - 1), [[k] for k in range(K0)])]
    K1 = shape[2]
    cell = np.arange(K0 * K1).reshape(K0, K1)
    out = [(np.arange(K0 - 1), [list(cell[k]) for k in range(K0)])]
    if kind == "indep":
        out.append((K0 - 1 + np.arange(K1 - 1), [list(cell[:, k]) for k in range(K1)]))
        return K0 - 1 + K1 - 1, K0 * K1, out
    for r in range(K0):
        out.append((K0 - 1 + r * (K1 - 1) + np.arange(K1 - 1), [[cell[r, k]] for k in range(K1)]))
    return K0 - 1 + K0 * (K1 - 1), K0 * K1, out


def lnh_of(shape, theta, lnvol):
    """lnh [B] in long double of one row ``theta`` [P]: the sum of the blocks' log_softmax minus the log cell volumes."""
    P, B, bl = blocks(shape)
    out = -np.asarray(lnvol).astype(LD).reshape(B)
    for idx, cells in bl:
        a = np.concatenate([[LD(0)], np.asarray(theta).astype(LD)[idx]])
        ls = a - (a.max() + np.log(np.exp(a - a.max()).sum()))
        for k, cs in enumerate(cells):
            out[cs] += ls[k]
    return out


def objective(shape, theta, lnvol, A, mask=None, a_sel=None):
    return lnL(A, lnh_of(shape, theta, lnvol), mask, a_sel)


def derivatives(shape, theta, lnvol, A, mask=None, a_sel=None):
    """``(grad [P], hessian [P, P])`` of :func:`objective` in long double: the moments, then the chain rule with
    d log_softmax_k / d a_j = delta_kj - pi_j and d^2 log_softmax_k / d a_j d a_l = -(delta_jl pi_j - pi_j pi_l)."""
    P, B, bl = blocks(shape)
    lnh = lnh_of(shape, theta, lnvol)
    # the moments from the long-double heights themselves (not through float64 lnh)
    A_ = np.asarray(A, np.float64).astype(LD)
    h = np.exp(lnh - lnh.max())
    on = np.ones(A_.shape[1], bool) if mask is None else np.asarray(mask) != 0
    ua = h[:, None] * A_
    s1 = ua.sum(axis=0)
    live = on & (s1 > 0)
    p = ua[:, live] / s1[live]
    N, Cm = p.sum(axis=1), p @ p.T
    g, Hl = N.copy(), np.diag(N) - Cm
    if a_sel is not None:
        q = h * np.asarray(a_sel, np.float64).astype(LD)
        q = q / q.sum()
        Su = LD(on.sum())
        g, Hl = g - Su * q, Hl - Su * (np.diag(q) - np.outer(q, q))
    G, second = np.zeros((B, P), LD), np.zeros((P, P), LD)
    for idx, cells in bl:
        a = np.concatenate([[LD(0)], np.asarray(theta).astype(LD)[idx]])
        e = np.exp(a - a.max())
        pi = e / e.sum()
        share = LD(0)
        for k, cs in enumerate(cells):
            for j in range(1, len(pi)):
                G[cs, idx[j - 1]] = (1.0 if j == k else 0.0) - pi[j]
            share += g[cs].sum()
        for j in range(1, len(pi)):
            for l in range(1, len(pi)):
                second[idx[j - 1], idx[l - 1]] -= share * ((pi[j] if j == l else 0) - pi[j] * pi[l])
    return G.T @ g, G.T @ Hl @ G + second


def central_gradient(f, theta, step=1e-5):
    """Central differences of ``f`` at ``theta`` [P] with ``step``."""
    theta = np.asarray(theta, np.float64)
    out = np.empty(theta.size, LD)
    for i in range(theta.size):
        e = np.zeros(theta.size)
        e[i] = step
        out[i] = (LD(f(theta + e)) - LD(f(theta - e))) / LD(2 * step)
    return out


# -- comparing --------------------------------------------------------------------------------------------------------
def close(got, want, n_live, limit=LIMIT):
    """``got`` [H, ...] against ``want`` within ``limit * max(1, n_live[h])``.  Returns the largest error over the limit."""
    got, want = np.asarray(got, np.float64), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    scale = np.maximum(1.0, np.asarray(n_live, np.float64)).reshape((-1,) + (1,) * (got.ndim - 1))
    worst = float(np.max(np.abs(got.astype(LD) - want) / (limit * scale)))
    assert worst <= 1.0, worst
    return worst


def assert_matches(out, A, lnh, mask=None, pairs=True):
    """The library's ``N``, ``C``, ``n_live`` against the twin and both identities, all within the limit."""
    want = moments(A, lnh, mask)
    assert np.array_equal(out["n_live"], want["n_live"]), (out["n_live"], want["n_live"])
    worst = [close(out["N"], want["N"], want["n_live"])]
    worst.append(close(out["N"].sum(axis=1), want["n_live"].astype(LD), want["n_live"]))
    if pairs:
        worst.append(close(out["C"], want["C"], want["n_live"]))
        worst.append(close(out["C"].sum(axis=2), out["N"].astype(LD), want["n_live"]))
        assert np.array_equal(out["C"], out["C"].transpose(0, 2, 1))
    return max(worst)


# -- cases ------------------------------------------------------------------------------------------------------------
def random_table(S, B, seed, dead=(), sparse=0.3):
    """A [B, S]: positive entries over several decades, a fraction ``sparse`` of exact zeros, the stars ``dead`` all zero;
    every other star keeps one positive entry."""
    rng = np.random.default_rng(seed)
    A = np.exp(rng.normal(0.0, 2.0, (B, S)))
    A[rng.random((B, S)) < sparse] = 0.0
    A[rng.integers(0, B, S), np.arange(S)] = np.exp(rng.normal(0.0, 1.0, S))
    A[:, list(dead)] = 0.0
    return np.ascontiguousarray(A)


def random_lnh(H, B, seed, zero=0.1):
    """H rows of log cell densities, a few cells of height 0 among them, never a whole row."""
    rng = np.random.default_rng(seed)
    lnh = rng.normal(0.0, 1.5, (H, B))
    lnh[rng.random((H, B)) < zero] = -np.inf
    lnh[:, 0] = np.where(np.isneginf(lnh).all(axis=1), 0.0, lnh[:, 0])
    return lnh


# -- the call ---------------------------------------------------------------------------------------------------------
def call(lib, A, lnh, mask=None, device=None, pairs=True, rows=None, guard=False):
    """``iso_binfit_moments_host`` or, with ``device``, ``iso_binfit_moments`` on copies of the numpy inputs; ``rows``: a
    (first, count) sub-range of the rows of ``lnh``.  Returns ``(rc, dict)`` of numpy ``N``, ``C`` (the fill value -7 when
    ``pairs`` is False), ``n_live``.  With ``guard`` every device output lies between two margins of -7 that have to stay
    so."""
    lnh = np.ascontiguousarray(lnh, dtype=np.float64)
    if rows is not None:
        lnh = np.ascontiguousarray(lnh[rows[0]:rows[0] + rows[1]])
    A = np.ascontiguousarray(A, dtype=np.float64)
    (H, B), S = lnh.shape, A.shape[1]
    up, ptr, host = bt._mover(device)
    dA, dl = up(A), up(lnh)
    dm = None if mask is None else up(np.ascontiguousarray(mask, dtype=np.int32))
    N, Cm, live = up(np.full((H, B), -7.0)), up(np.full((H, B, B), -7.0)), up(np.full(H, -7, np.int32))
    flats = []
    if guard and device is not None:
        flats, (N, Cm, live) = zip(*[guarded(t.shape, t.dtype, device) for t in (N, Cm, live)])
    ws = None
    if device is not None:
        need = lib.iso_binfit_workspace_doubles(B, S, H, int(pairs))
        ws = up(np.full(max(int(need), 1), -7.0))
    fn = lib.iso_binfit_moments_host if device is None else lib.iso_binfit_moments
    rc = fn(ptr(dA), B, S, ptr(dl), H, ptr(dm), ptr(N), ptr(Cm if pairs else None), ptr(live), ptr(ws), bt._stream(device))
    if device is not None:
        import torch
        torch.cuda.synchronize()
        assert all(margins_untouched(f) for f in flats), "a write outside an output"
    return rc, dict(N=host(N), C=host(Cm), n_live=host(live))
