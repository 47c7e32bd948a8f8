"""TEST INFRASTRUCTURE - the catalog nested sampler (isochrones_amd/csrc/nested/nested_kernel.h) in numpy, one star at a time.

It implements the text of DESIGN.md "Nested sampling of a catalog" with the device's random numbers (Philox4x32-10,
key = seed, counter = (8 chunk + call, global star index low word, lane | high word << 16, 0x4E)) and a pluggable
``loglike(theta [n, D]) -> [n]``, so that

* the ALGORITHM can be checked without a GPU against analytic evidences (tests/test_nested_catalog_cpu.py), and
* a device fit can be replayed step by step from what it stored (tests/test_gpu_nested_catalog.py): :func:`fill_draws`,
  :func:`ellipsoid_draws` and :func:`bounding_ellipsoid` are the pieces the replay regenerates.

Never imported by the product."""
import numpy as np

from oracle.cpu_sampler import philox4x32_10

BLOCK = 256
CALLS_PER_CHUNK = 8
TAG = 0x4E


def remove_per_step(nlive, D):
    return max(1, min(nlive // 10, nlive - 2 * (D + 1)))


def _uniform53(hi, lo):
    return (hi.astype(np.float64) * 2097152.0 + (lo & np.uint64(0x1FFFFF)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def _philox(seed, gidx, chunk, call, lanes):
    lanes = np.asarray(lanes, dtype=np.uint64)
    n = lanes.shape
    c0 = np.broadcast_to(np.asarray(chunk, dtype=np.uint64) * np.uint64(CALLS_PER_CHUNK) + np.uint64(call), n)
    c1 = np.full(n, int(gidx) & 0xFFFFFFFF, dtype=np.uint64)
    c2 = lanes | np.uint64(((int(gidx) >> 32) << 16) & 0xFFFFFFFF)
    return philox4x32_10(c0, c1, c2, np.full(n, TAG, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def fill_draws(seed, gidx, chunk, D, lanes=None):
    """Unit-cube draws of the lanes of fill chunk(s) ``chunk`` (scalar or array like ``lanes``): [n, D]."""
    lanes = np.arange(BLOCK) if lanes is None else np.asarray(lanes)
    u = np.empty(lanes.shape + (D,))
    for c in range((D + 1) // 2):
        r = _philox(seed, gidx, chunk, c, lanes)
        u[..., 2 * c] = _uniform53(r[0], r[1])
        if 2 * c + 1 < D:
            u[..., 2 * c + 1] = _uniform53(r[2], r[3])
    return u


def ellipsoid_draws(seed, gidx, chunk, mean, A, lanes=None):
    """Draws uniform in the ellipsoid {mean + A z, |z| <= 1}: (x [n, D], inside-the-cube flags)."""
    lanes = np.arange(BLOCK) if lanes is None else np.asarray(lanes)
    D = mean.size
    z = np.empty(lanes.shape + (2 * ((D + 1) // 2),))
    for c in range((D + 1) // 2):
        r = _philox(seed, gidx, chunk, c, lanes)
        rho = np.sqrt(-2.0 * np.log(1.0 - _uniform53(r[0], r[1])))
        ang = 2.0 * np.pi * _uniform53(r[2], r[3])
        z[..., 2 * c] = rho * np.cos(ang)
        z[..., 2 * c + 1] = rho * np.sin(ang)
    z = z[..., :D]
    r = _philox(seed, gidx, chunk, 4, lanes)
    with np.errstate(divide="ignore"):
        sc = np.exp(np.log(_uniform53(r[0], r[1])) / D) / np.sqrt(np.sum(z * z, axis=-1))
    x = mean + (z * sc[..., None]) @ np.tril(A).T
    inside = np.all((x >= 0.0) & (x <= 1.0), axis=-1)
    return x, inside


def bounding_ellipsoid(u, enlarge=1.5, dtype=np.float64):
    """mean and lower-triangular A of the enlarged bounding ellipsoid of the points u [n, D] (nested._bounding_ellipsoid)."""
    u = np.asarray(u, dtype=dtype)
    n, D = u.shape
    mean = u.sum(axis=0) / dtype(n)
    dx = u - mean
    cov = dx.T @ dx / dtype(n - 1) + dtype(1e-14) * np.eye(D, dtype=dtype)
    L = np.zeros((D, D), dtype=dtype)
    ok = True
    for a in range(D):
        for b in range(a + 1):
            s = cov[a, b] - np.dot(L[a, :b], L[b, :b])
            if a == b:
                ok = ok and s > 0
                L[a, a] = np.sqrt(s) if s > 0 else 0
            else:
                L[a, b] = s / L[b, b] if ok else 0
        if not ok:
            break
    if not ok:
        L = np.diag(np.sqrt(np.diag(cov)))
    y = np.zeros_like(dx)
    for a in range(D):
        y[:, a] = (dx[:, a] - y[:, :a] @ L[a, :a]) / L[a, a]
    r2 = np.max(np.sum(y * y, axis=1))
    return mean, L * np.sqrt(r2) * dtype(enlarge) ** (dtype(1.0) / dtype(D))


class _Stream:
    """lnZ, H and the posterior moments as streamed sums against a running reference exponent."""

    def __init__(self, D):
        self.R = -np.inf
        self.acc = np.zeros(2 * D + 2)

    def add(self, terms, logl, theta):
        Rn = max(self.R, float(np.max(terms)))
        w = np.exp(terms - Rn)
        scale = np.exp(self.R - Rn) if self.R > -np.inf else 0.0
        f = np.column_stack([np.ones_like(logl), logl, theta, theta * theta])
        acc = self.acc * scale
        for j in range(terms.size):              # in order, as the device's lanes do
            acc = acc + w[j] * f[j]
        self.acc, self.R = acc, Rn

    @property
    def lnz(self):
        return self.R + np.log(self.acc[0])


def _retire(logx, cs, logl, last_takes_all):
    n = logl.size
    lx = logx - cs[:n]
    if last_takes_all:
        lx = lx.copy()
        lx[-1] = -np.inf
    prev = np.concatenate([[logx], logx - cs[: n - 1]])
    with np.errstate(divide="ignore"):
        return prev + np.log1p(-np.exp(lx - prev)) + logl


def nested_fit(loglike, lo, hi, nlive, gidx=0, seed=0, tol=0.5, enlarge=1.5, max_iter=None, max_fill_chunks=4096,
               max_chunks=1 << 18):
    """One star's fit.  Returns a dict: lnZ, lnZ_err, H, ncall, niter, prior_fraction, status, mean, std (streamed), and the
    dead points (dead_u, dead, logl, logwt) and trace (thr, first, last, mean, A per macro-step)."""
    lo = np.asarray(lo, dtype=float)
    hi = np.asarray(hi, dtype=float)
    span = hi - lo
    D = lo.size
    K = remove_per_step(nlive, D)
    max_iter = 100 * nlive if max_iter is None else max_iter

    def evaluate(u):
        ll = np.asarray(loglike(lo + u * span), dtype=float).reshape(-1)
        return np.where(np.isfinite(ll), ll, -np.inf)

    out = dict(status=0)
    chunk, ncall, nfinite = 0, 0, 0
    live_u, live_l = np.empty((0, D)), np.empty(0)
    while live_l.size < nlive:
        if chunk >= min(max_fill_chunks, max_chunks):
            out.update(status=1, ncall=ncall, niter=0, prior_fraction=nfinite / max(chunk * BLOCK, 1))
            return out
        u = fill_draws(seed, gidx, chunk, D)
        ll = evaluate(u)
        ok = ll > -np.inf
        live_u, live_l = np.vstack([live_u, u[ok]]), np.concatenate([live_l, ll[ok]])
        nfinite += int(ok.sum())
        ncall += BLOCK
        chunk += 1
    frac = nfinite / (chunk * BLOCK)
    order = np.argsort(live_l[:nlive], kind="stable")
    live_u, live_l = live_u[:nlive][order], live_l[:nlive][order]
    csum = np.cumsum(1.0 / (nlive - np.arange(K)))
    S = _Stream(D)
    dead_u, dead_l, dead_t, trace = [], [], [], []
    logx, it = 0.0, 0
    while True:
        terms = _retire(logx, csum, live_l[:K], False)
        S.add(terms, live_l[:K], lo + live_u[:K] * span)
        dead_u.append(live_u[:K].copy()); dead_l.append(live_l[:K].copy()); dead_t.append(terms)
        thr = live_l[K - 1]
        logx -= csum[K - 1]
        it += K
        if live_l[-1] + logx < S.lnz + np.log(tol) or it >= max_iter:
            break
        sv_u, sv_l = live_u[K:], live_l[K:]
        mean, A = bounding_ellipsoid(sv_u, enlarge)
        new_u, new_l = np.empty((0, D)), np.empty(0)
        first = chunk * BLOCK
        last = None
        while new_l.size < K:
            if chunk >= max_chunks:
                out.update(status=2, ncall=ncall, niter=it, prior_fraction=frac)
                return out
            x, inside = ellipsoid_draws(seed, gidx, chunk, mean, A)
            ll = np.full(BLOCK, -np.inf)
            if inside.any():
                ll[inside] = evaluate(x[inside])
            ncall += int(inside.sum())
            good = inside & (ll > thr)
            idx = np.nonzero(good)[0][: K - new_l.size]
            new_u, new_l = np.vstack([new_u, x[idx]]), np.concatenate([new_l, ll[idx]])
            if new_l.size == K:
                last = chunk * BLOCK + int(idx[-1])
            chunk += 1
        trace.append(dict(thr=thr, first=first, last=last, mean=mean, A=A))
        # survivors first at equal logl (they are older), new points in draw order: a stable sort of [survivors | new]
        all_u, all_l = np.vstack([sv_u, new_u]), np.concatenate([sv_l, new_l])
        order = np.argsort(all_l, kind="stable")
        live_u, live_l = all_u[order], all_l[order]
    sv_u, sv_l = live_u[K:], live_l[K:]
    n_left = sv_l.size
    cs = np.cumsum(1.0 / (n_left - np.arange(n_left)))
    terms = _retire(logx, cs, sv_l, True)
    S.add(terms, sv_l, lo + sv_u * span)
    dead_u.append(sv_u); dead_l.append(sv_l); dead_t.append(terms)
    lnz0 = S.lnz
    H = max(S.acc[1] / S.acc[0] - lnz0, 0.0)
    mean = S.acc[2:2 + D] / S.acc[0]
    var = S.acc[2 + D:] / S.acc[0] - mean * mean
    dead_u = np.vstack(dead_u)
    out.update(lnZ=lnz0 + np.log(frac), lnZ_err=np.sqrt(H / nlive), H=H, ncall=ncall, niter=it, prior_fraction=frac,
               mean=mean, std=np.sqrt(np.maximum(var, 0.0)), dead_u=dead_u, dead=lo + dead_u * span,
               logl=np.concatenate(dead_l), logwt=np.concatenate(dead_t), trace=trace, K=K)
    return out
