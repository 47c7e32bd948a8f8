"""A long-double numpy statement of include/isochrones_amd_emfit.h (a batch of weighted EM fits of the cell masses of a
binned population, libiso_emfit.so), a float64 statement of k_emfit_run's lane-strided summation order, the bootstrap
weights on the oracle's Philox, the Poisson thresholds at 40 digits, the case builders, and the one way the host and device
tests call the library.

The EM steps are evaluated from the float64 inputs the library itself was given, in numpy's long double.  After a step
every g_b is a quotient of two sums of at most S products that each carry a few ulp, so one step is off by some 1e-15 at
worst; over the 1, 2 and 7 steps of the tests the errors of one step feed the next through a map that is a contraction
near the maximum, and 1e-11 is four orders of magnitude inside."""
import ctypes as C

import numpy as np

from oracle.cpu_sampler import philox4x32_10
from tests import _binned_twin as bt
from tests._binfit_twin import random_table  # noqa: F401  (the tables of the binfit tests)
from tests._hier_twin import guarded, margins_untouched

LD = np.longdouble
LIMIT = 1e-11
RUNNING, CONVERGED, MAX_ITER, EMPTY = 0, 1, 2, 3
LANES = 256


# -- the definition ---------------------------------------------------------------------------------------------------
def evaluate(A, v, w, on):
    """One evaluation at the heights ``v`` [B] (any float type; the sums are taken in it): ``(Q, N [B], W, n_live, sum w
    |ln s1|)`` over the live stars."""
    ua = v[:, None] * A
    s1 = ua.sum(axis=0)
    with np.errstate(invalid="ignore"):
        live = on & (w > 0) & (s1 > 0)
    if not live.any():
        z = v.dtype.type(0)
        return z, np.zeros_like(v), z, 0, z
    ln = np.log(s1[live])
    wl = w[live]
    return (wl * ln).sum(), (ua[:, live] * (wl / s1[live])).sum(axis=1), wl.sum(), int(live.sum()), (wl * np.abs(ln)).sum()


def run(A, scale, w=None, mask=None, g0=None, max_iter=0, tol=-np.inf, R=None):
    """The header's definition in long double.  ``w`` [R, S] or None; ``g0`` [B] (shared) or [R, B].  Returns a dict of
    ``g`` [R, B], ``objective``, ``wsum``, ``absln`` (sum w |ln s1| of the last evaluation) [R] in long double, ``n_iter``,
    ``status``, ``n_live`` [R] int32 and ``trace``: per replicate the list of Q_0 .. Q_t."""
    A = np.asarray(A, np.float64).astype(LD)
    B, S = A.shape
    scale = np.asarray(scale, np.float64).astype(LD)
    g0 = np.asarray(g0, np.float64)
    R = (w.shape[0] if w is not None else (g0.shape[0] if g0.ndim == 2 else 1)) if R is None else R
    on = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
    out = dict(g=np.zeros((R, B), LD), objective=np.zeros(R, LD), wsum=np.zeros(R, LD), absln=np.zeros(R, LD),
               n_iter=np.zeros(R, np.int32), status=np.zeros(R, np.int32), n_live=np.zeros(R, np.int32), trace=[])
    for r in range(R):
        g = (g0[r] if g0.ndim == 2 else g0).astype(LD)
        wr = np.ones(S, LD) if w is None else np.asarray(w[r], np.float64).astype(LD)
        t, Qprev, trace = 0, LD(0), []
        while True:
            Q, N, W, live, absln = evaluate(A, g * scale, wr, on)
            trace.append(Q)
            if live == 0:
                status = EMPTY
            elif t >= 1 and Q - Qprev < tol:
                status = CONVERGED
            elif t == max_iter:
                status = MAX_ITER
            else:
                g, Qprev, t = N / N.sum(), Q, t + 1
                continue
            break
        out["g"][r], out["objective"][r], out["wsum"][r], out["absln"][r] = g, Q, W, absln
        out["n_iter"][r], out["status"][r], out["n_live"][r] = t, status, live
        out["trace"].append(trace)
    return out


def lane_order_step(A, scale, g, w=None, mask=None):
    """One evaluation and step of one replicate in float64 in k_emfit_run's order: lane l sums the stars l, l + 256, ... in
    ascending order from 0.0, a wavefront's 64 lane sums are combined by xor butterflies of distances 32 .. 1, and the four
    wavefront totals are added in ascending order.  Returns ``(Q, N [B], W, n_live, g_next [B])``; numpy's log stands in
    for the device's, so Q is this order's value to a few ulp per star, not bit for bit."""
    A = np.asarray(A, np.float64)
    B, S = A.shape
    v = np.asarray(g, np.float64) * np.asarray(scale, np.float64)
    on = np.ones(S, bool) if mask is None else np.asarray(mask) != 0
    wt = np.ones(S) if w is None else np.asarray(w, np.float64)
    lanes = np.zeros((LANES, B + 2))
    n_live = 0
    for s in range(S):
        s1 = 0.0
        for b in range(B):
            s1 += v[b] * A[b, s]
        if not (on[s] and wt[s] > 0 and s1 > 0):
            continue
        n_live += 1
        ratio = wt[s] / s1
        row = lanes[s % LANES]
        row[:B] += (v * A[:, s]) * ratio
        row[B] += wt[s] * np.log(s1)
        row[B + 1] += wt[s]

    def wave_sum(x):                                                    # x [64, K]: every lane ends with the same value
        for d in (32, 16, 8, 4, 2, 1):
            x = x + x[np.arange(64) ^ d]
        return x[0]
    waves = [wave_sum(lanes[64 * k:64 * k + 64]) for k in range(4)]
    tot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    N = tot[:B]
    T = 0.0
    for b in range(B):
        T += N[b]
    with np.errstate(invalid="ignore", divide="ignore"):
        return tot[B], N, tot[B + 1], n_live, N / T


# -- the weights ------------------------------------------------------------------------------------------------------
def poisson_cdf(digits=40):
    """The cumulative Poisson(1) probabilities c_0 .. c_17 evaluated with ``digits`` digits, as mpmath numbers."""
    import mpmath
    with mpmath.workdps(digits):
        e1, out, c, f = mpmath.exp(-1), [], mpmath.mpf(0), mpmath.mpf(1)
        for k in range(18):
            f = f * k if k else f
            c = c + e1 / f
            out.append(c)
        return out


def uniforms(seed, first, R, S):
    """u [R, S] of the header: Philox4x32-10 at (s, first + r, 0, 0xB7) under the key seed, philox_uniform53 of words 0, 1."""
    s, r = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(first, first + R, dtype=np.uint64))
    x0, x1, _, _ = philox4x32_10(s.ravel(), r.ravel(), np.zeros(R * S, np.uint64), np.full(R * S, 0xB7, np.uint64),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    m = (x0.astype(np.uint64) << np.uint64(21)) | (x1.astype(np.uint64) & np.uint64(0x1FFFFF))
    u = (m.astype(np.float64) + 0.5) * 2.0 ** -53
    return np.where(u < 1.0, u, 1.0 - 2.0 ** -53).reshape(R, S)


def weights(kind, seed, first, R, S):
    """The header's weights [R, S]: ``kind`` 0 the Poisson(1) counts (against float(c_k) of :func:`poisson_cdf`), 1 -log(u)
    in long double."""
    u = uniforms(seed, first, R, S)
    if kind == 1:
        return -np.log(u.astype(LD))
    c = np.array([float(x) for x in poisson_cdf()])
    return (u[:, :, None] >= c[None, None, :]).sum(axis=2).astype(np.float64)


# -- cases ------------------------------------------------------------------------------------------------------------
def case(S, B, R, seed=0, hard=True):
    """A table, a scale, weights, a mask and start masses.  With ``hard`` (and room for it): a closed cell (scale 0), a start
    mass of 0, an all-zero star, a masked star, a star of weight 0, and (R >= 2) a last replicate without a live star."""
    rng = np.random.default_rng(1000 * S + 10 * B + R + seed)
    A = random_table(S, B, seed=S + 7 * B + seed, dead=(S // 3,) if hard and S > 3 else ())
    scale = np.exp(rng.normal(0.0, 0.5, B))
    g0 = rng.dirichlet(np.ones(B), size=R)
    w = rng.poisson(1.0, (R, S)).astype(np.float64) + (rng.random((R, S)) < 0.5) * rng.random((R, S))
    mask = None
    if hard and S > 3:
        mask = np.ones(S, np.int32)
        mask[S // 2] = 0
        w[:, S - 1] = 0.0
    if hard and B > 2:
        scale[1] = 0.0
        g0[:, B - 1] = 0.0
        g0 /= g0.sum(axis=1, keepdims=True)
    if hard and R >= 2:
        w[R - 1] = 0.0
    return dict(A=A, scale=scale, w=w, mask=mask, g0=np.ascontiguousarray(g0))


# -- the calls --------------------------------------------------------------------------------------------------------
def call(lib, A, scale, w=None, mask=None, g0=None, max_iter=0, tol=-np.inf, steps=0, device=None, R=None, guard=False):
    """``iso_emfit_run_host`` or, with ``device``, ``iso_emfit_run`` on copies of the numpy inputs.  ``g0`` [B] is passed
    with g0_stride 0, [R, B] with g0_stride B.  Returns ``(rc, dict)`` of numpy ``g``, ``objective``, ``n_iter``, ``status``,
    ``n_live``, ``wsum``; what the call does not write keeps the fill value -7.  With ``guard`` every device output lies
    between two margins of -7 that have to stay so."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, S = A.shape
    g0 = np.ascontiguousarray(g0, dtype=np.float64)
    stride = B if g0.ndim == 2 else 0
    R = (w.shape[0] if w is not None else (g0.shape[0] if g0.ndim == 2 else 1)) if R is None else R
    up, ptr, host = bt._mover(device)
    dA, ds, dg0 = up(A), up(np.ascontiguousarray(scale, dtype=np.float64)), up(g0)
    dw = None if w is None else up(np.ascontiguousarray(w, dtype=np.float64))
    dm = None if mask is None else up(np.ascontiguousarray(mask, dtype=np.int32))
    outs = [up(np.full((R, B), -7.0)), up(np.full(R, -7.0)), up(np.full(R, -7, np.int32)), up(np.full(R, -7, np.int32)),
            up(np.full(R, -7, np.int32)), up(np.full(R, -7.0))]
    flats = []
    if guard and device is not None:
        flats, outs = zip(*[guarded(t.shape, t.dtype, device) for t in outs])
    g, obj, n_iter, status, n_live, wsum = outs
    fn = lib.iso_emfit_run_host if device is None else lib.iso_emfit_run
    rc = fn(ptr(dA), B, S, ptr(ds), ptr(dw), R, ptr(dm), ptr(dg0), stride, int(max_iter), float(tol), int(steps), ptr(g),
            ptr(obj), ptr(n_iter), ptr(status), ptr(n_live), ptr(wsum), bt._stream(device))
    if device is not None:
        import torch
        torch.cuda.synchronize()
        assert all(margins_untouched(f) for f in flats), "a write outside an output"
    return rc, dict(g=host(g), objective=host(obj), n_iter=host(n_iter), status=host(status), n_live=host(n_live),
                    wsum=host(wsum))


def call_weights(lib, kind, seed, first, R, S, device=None):
    """``iso_emfit_weights_host`` or, with ``device``, ``iso_emfit_weights``.  Returns ``(rc, out [R, S])``."""
    up, ptr, host = bt._mover(device)
    out = up(np.full((max(R, 1), max(S, 1)), -7.0))
    fn = lib.iso_emfit_weights_host if device is None else lib.iso_emfit_weights
    rc = fn(int(kind), C.c_uint64(seed), int(first), int(R), int(S), ptr(out), bt._stream(device))
    if device is not None:
        import torch
        torch.cuda.synchronize()
    return rc, host(out)


def same_bits(a, b, keys=("g", "objective", "n_iter", "status", "n_live", "wsum")):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


def assert_matches(out, ref, limit=LIMIT):
    """The library's outputs against :func:`run`'s: counts and statuses equal, ``g`` within ``limit`` absolute, ``objective``
    within ``limit`` relative to max(1, sum w |ln s1|), ``wsum`` within ``limit`` relative to max(1, W).  Returns the
    largest error over its limit."""
    for k in ("n_iter", "status", "n_live"):
        assert np.array_equal(out[k], ref[k]), (k, out[k], ref[k])
    eg = float(np.max(np.abs(out["g"].astype(LD) - ref["g"]))) / limit
    eq = float(np.max(np.abs(out["objective"].astype(LD) - ref["objective"]) / np.maximum(1, ref["absln"]))) / limit
    ew = float(np.max(np.abs(out["wsum"].astype(LD) - ref["wsum"]) / np.maximum(1, ref["wsum"]))) / limit
    assert max(eg, eq, ew) <= 1.0, (eg, eq, ew)
    return max(eg, eq, ew)
