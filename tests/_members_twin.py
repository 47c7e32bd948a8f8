"""Long-double restatement of iso_members_moments (include/isochrones_amd_members.h), written from the header, not from the
kernels, with the conventions of tests/_cluster_hp.py.

It takes exactly the C ABI's inputs in the header's layout and treats those float64 values as exact.  Everything else is
evaluated in ``np.longdouble``: the binary magnitude, ``logaddexp``, ``ln q``, the Gaussian terms, the two state weights,
every trapezoid and every quotient.  The float64 decisions that define the operation are kept:

* the mass-ratio cut ``q < minq`` is made on the float64 quotient ``m_k / m_j``, and that quotient is the weight ``q``;
* each cell's ``e`` is rounded to float64, so float64 underflow gives the operation's zeros;
* each product ``g * e`` is rounded to float64 before it is summed;
* a cell with ``e == 0`` contributes 0 to every integral (a select);
* ``n_valid`` is clamped to ``[0, ld]``.

Also here: the seeded inputs the host and the GPU tests share (:data:`CASES`), the issue's constructed case, the ctypes call of
either entry point and the comparison at ``TOL * (1 + |x|)``."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _cluster_hp as H

LD = np.longdouble
NMOM = 11
NINNER = 6
#: |got - ref| <= TOL (1 + |ref|) on ln_like and on every moment: the bound tests/test_gpu_cluster_abi.py holds the likelihood to
TOL = 1e-11
#: most stars per vectorised block of the (j, k) grid
STAR_BLOCK = 16
MARGIN = 1024
FILL = -7.0


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _logaddexp(a, b):
    hi = np.where(b > a, b, a)
    return hi + np.log(np.exp(a - hi) + np.exp(b - hi))


def _row(c, n, rp, val, w, nb, npr, minq):
    """(like_s [N_s], N_g [N_s, 11]) of one row, long double: c [3 + 2 nb + npr][ld] float64, n valid EEPs."""
    ns = val.shape[1]
    like = np.zeros(ns, dtype=LD)
    N = np.zeros((ns, NMOM), dtype=LD)
    if n < 2:
        return like, N
    eep, mass, mterm = c[0, :n], c[1, :n], c[2, :n]
    flux, mag, prop_model = c[3:3 + nb, :n], c[3 + nb:3 + 2 * nb, :n], c[3 + 2 * nb:3 + 2 * nb + npr, :n]
    ln_fb, ln_1mfb, gamma, ln_cq = (LD(v) for v in rp)
    jj, kk = np.tril_indices(n)                                         # cells (j, k <= j)
    q64 = mass[kk] / mass[jj]                                           # the float64 quotient: the cut and the weight
    keep = ~(q64 < minq)
    q = q64.astype(LD)
    pair_term = mterm[jj].astype(LD) + ln_cq + gamma * np.log(q)
    binary = -2.5 * np.log10(flux[:, jj].astype(LD) + flux[:, kk].astype(LD))   # [nb, cells]
    eL, mL = eep.astype(LD), mass.astype(LD)
    d = np.diff(eL)
    v, wt = val.astype(LD), w.astype(LD)
    mag_l, pm = mag.astype(LD), prop_model.astype(LD)
    inner_mask = np.arange(1, n)[None, :] <= np.arange(n)[:, None]      # [j, k - 1]: k <= j
    one = np.ones(n, dtype=LD)
    # moment -> (inner integral, u_j)
    outer = ((0, eL), (0, eL * eL), (0, mL), (0, mL * mL), (1, one), (2, one), (1, mL), (2, mL * mL), (3, one), (4, one), (5, one))

    def trapz_outer(inner, u):
        x = inner * u[None, :]
        return (0.5 * (x[:, :-1] + x[:, 1:]) * d[None, :]).sum(axis=1)

    def block(s0, s1):
        vs, ws = v[:, s0:s1], wt[:, s0:s1]
        S = s1 - s0
        phot = np.zeros((S, jj.size), dtype=LD)
        suma = np.zeros((S, jj.size), dtype=LD)
        sumc = np.zeros((S, n), dtype=LD)
        for b in range(nb):
            cb = ln_1mfb + -0.5 * (mag_l[b][None, :] - vs[b][:, None]) ** 2 * ws[b][:, None]             # [S, n]
            ab = ln_fb + -0.5 * (binary[b][None, :] - vs[b][:, None]) ** 2 * ws[b][:, None]              # [S, cells]
            phot = phot + _logaddexp(ab, cb[:, jj])
            suma = suma + ab
            sumc = sumc + cb
        prop = np.zeros((S, n), dtype=LD)
        for p in range(npr):
            prop = prop + -0.5 * (vs[nb + p][:, None] - pm[p][None, :]) ** 2 * ws[nb + p][:, None]
        L = phot + pair_term[None, :] + prop[:, jj]
        e64 = np.where(keep[None, :], np.exp(np.where(keep[None, :], L, 0)).astype(np.float64), 0.0)
        dead = e64 == 0                                                  # a NaN is not dead: it goes through
        safe = np.where(dead, 0, phot)
        pairw = np.exp(np.where(dead, 0, suma) - safe)
        singlew = np.exp(np.where(dead, 0, sumc[:, jj]) - safe)
        e = e64.astype(LD)
        inner = []
        for g in (None, q[None, :], (q * q)[None, :], pairw, singlew, q[None, :] * pairw):
            x64 = e64 if g is None else np.where(dead, 0.0, (g * e).astype(np.float64))   # g * e rounded to float64
            grid = np.zeros((S, n, n), dtype=LD)
            grid[:, jj, kk] = x64
            seg = 0.5 * (grid[:, :, :-1] + grid[:, :, 1:]) * d[None, None, :]
            inner.append(np.where(inner_mask[None], seg, 0).sum(axis=2))                    # [S, j]
        like[s0:s1] = trapz_outer(inner[0], one)
        for m, (g, u) in enumerate(outer):
            N[s0:s1, m] = trapz_outer(inner[g], u)

    with np.errstate(all="ignore"):
        step = max(1, min(STAR_BLOCK, -(-ns // _threads())))
        spans = [(s, min(s + step, ns)) for s in range(0, ns, step)]
        if len(spans) == 1:
            block(*spans[0])
        else:
            with ThreadPoolExecutor(_threads()) as ex:
                list(ex.map(lambda sp: block(*sp), spans))
    return like, N


def moments(cols, n_valid, rowpar, star_val, star_w, minq, n_bands, n_props):
    """The operation on host arrays -> ``(ln_like [P][N_s], moments [P][N_s][11])``, both long double."""
    cols = np.asarray(cols, dtype=np.float64)
    P, ncol, ld = cols.shape
    assert ncol == 3 + 2 * n_bands + n_props, (ncol, n_bands, n_props)
    val, w = np.asarray(star_val, dtype=np.float64), np.asarray(star_w, dtype=np.float64)
    rowpar = np.asarray(rowpar, dtype=np.float64).reshape(P, 4)
    nv = np.asarray(n_valid).reshape(P)
    ns = val.shape[1]
    ln_like = np.empty((P, ns), dtype=LD)
    mom = np.empty((P, ns, NMOM), dtype=LD)
    for r in range(P):
        n = int(min(max(int(nv[r]), 0), ld))
        like, N = _row(cols[r], n, rowpar[r], val, w, n_bands, n_props, float(minq))
        with np.errstate(all="ignore"):
            ln_like[r] = np.log(like)
            mom[r] = np.where((like == 0)[:, None], np.nan, N / np.where(like == 0, 1, like)[:, None])
    return ln_like, mom


# -- inputs -------------------------------------------------------------------------------------------------------------
def draw(seed, ns, nb, npr, n_valid, ld, fB=None, minq=0.1, off=()):
    """ABI inputs of one launch: every row is an isochrone of ``ld`` EEPs (filled to its clamped ``n_valid``, NaN past it,
    so a read past ``n_valid`` shows), with uneven EEP steps; the stars are drawn near it, singles and pairs above the
    cut, at uncertainties 0.01 - 0.03.  off: stars moved 50 mag off the isochrone at uncertainty 0.01 (every cell
    underflows)."""
    rng = np.random.default_rng(seed)
    n_valid = np.asarray(n_valid, dtype=np.int32)
    P = n_valid.size
    fill = np.clip(n_valid, 0, ld)
    t = np.arange(ld) / max(ld - 1, 1)
    eep = 150.0 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, ld - 1))])
    mass = 0.3 + 0.9 * t ** 1.3
    lndm = np.log(0.01 + 0.005 * np.cos(3 * t))
    base = rng.uniform(6.0, 12.0, nb)
    color = rng.uniform(-0.5, 0.5, nb)
    mags = base[None, :] - 3.0 * (mass[:, None] - 0.3) + color[None, :] * t[:, None]          # [ld, nb]
    props = np.column_stack([np.sin((p + 1) * t) + 0.1 * p for p in range(npr)]) if npr else np.zeros((ld, 0))
    cols = np.full((P, 3 + 2 * nb + npr, ld), np.nan)
    rowpar = np.empty((P, 4))
    for r in range(P):
        alpha, gamma = rng.uniform(-3.0, -2.0), rng.uniform(0.1, 0.5)
        fb = rng.uniform(0.2, 0.5) if fB is None else fB
        c, rp = H.row_columns(eep, mass, lndm, mags, props, alpha, gamma, fb, minq, 0.1, 300.0, ld)
        n = int(fill[r])
        cols[r][:, :n] = c[:, :n]
        rowpar[r] = rp
    span = int(max(1, fill.max()))
    j = rng.integers(0, span, ns)
    k = (j * rng.uniform(0.3, 1.0, ns)).astype(int)
    binary = (rng.random(ns) < (0.35 if fB is None else fB)) & ~(mass[k] / mass[j] < minq)
    flux = 10 ** (-0.4 * mags)
    obs = np.where(binary[:, None], -2.5 * np.log10(flux[j] + flux[k]), mags[j])
    unc = rng.uniform(0.01, 0.03, (ns, nb))
    obs = obs + unc * rng.standard_normal((ns, nb))
    for s in off:
        obs[s] += 50.0
        unc[s] = 0.01
    punc = rng.uniform(0.05, 0.2, (ns, npr))
    pobs = props[j] + punc * rng.standard_normal((ns, npr))
    star_val = np.ascontiguousarray(np.concatenate([obs.T, pobs.T]))
    star_w = np.ascontiguousarray(1.0 / np.concatenate([unc.T, punc.T]) ** 2)
    return dict(cols=cols, n_valid=n_valid, rowpar=rowpar, star_val=star_val, star_w=star_w, minq=float(minq), nb=nb,
                npr=npr, ld=ld, ns=ns)


def rows_of(ld):
    """The n_valid of a launch's rows: {0, 1, 2, ld - 3, ld}."""
    return [0, 1, 2, max(ld - 3, 0), ld]


#: the launches the host and the GPU tests draw from; every one has the rows of :func:`rows_of`
CASES = {
    "1star_ld5_1band": dict(ns=1, nb=1, npr=0, ld=5),
    "65stars_ld66_32bands_2props": dict(ns=65, nb=32, npr=2, ld=66),
    "130stars_ld130_3bands_8props": dict(ns=130, nb=3, npr=8, ld=130),
    "fB0": dict(ns=65, nb=3, npr=0, ld=66, fB=0.0),
    "fB1": dict(ns=65, nb=3, npr=0, ld=66, fB=1.0),
    "minq09_1band": dict(ns=65, nb=1, npr=2, ld=130, minq=0.9),
    "underflow_star": dict(ns=65, nb=3, npr=0, ld=66, off=(10,)),
    "63stars_ld64_1band": dict(ns=63, nb=1, npr=0, ld=64),
    "64stars_ld65_8props": dict(ns=64, nb=3, npr=8, ld=65),
    "65stars_ld66_32bands": dict(ns=65, nb=32, npr=0, ld=66),
    "130stars_ld129": dict(ns=130, nb=3, npr=0, ld=129),
}
HOST_CASES = ("1star_ld5_1band", "65stars_ld66_32bands_2props", "130stars_ld130_3bands_8props", "fB0", "fB1", "minq09_1band",
              "underflow_star")
GPU_CASES = ("63stars_ld64_1band", "64stars_ld65_8props", "65stars_ld66_32bands", "130stars_ld129",
             "130stars_ld130_3bands_8props", "fB0", "fB1", "minq09_1band", "underflow_star")
#: seeds whose draws :func:`reference` accepts (no like_s in the subnormal range, which the short rows invite)
SEEDS = {"1star_ld5_1band": 2600, "65stars_ld66_32bands_2props": 2602, "130stars_ld130_3bands_8props": 2612, "fB0": 2600,
         "fB1": 2602, "minq09_1band": 2608, "underflow_star": 2601, "63stars_ld64_1band": 2603, "64stars_ld65_8props": 2601,
         "65stars_ld66_32bands": 2602, "130stars_ld129": 2604}
_CACHE = {}


def reference(a):
    """(ln_like, moments) of the twin as float64, after checking the draw: every like_s is exactly 0 or above 1e-280, so no
    comparison is decided in the subnormal range."""
    ln, mom = moments(a["cols"], a["n_valid"], a["rowpar"], a["star_val"], a["star_w"], a["minq"], a["nb"], a["npr"])
    like = np.exp(ln)
    bad = (like != 0) & (like <= 1e-280)
    assert not bad.any(), "draw has like_s in (0, 1e-280]: %s" % np.argwhere(bad)[:5]
    return ln.astype(np.float64), mom.astype(np.float64)


def case(name):
    """(inputs, (ln_like, moments) of the twin) of a named launch; computed once and shared."""
    if name not in _CACHE:
        c = dict(CASES[name])
        a = draw(SEEDS[name], n_valid=rows_of(c["ld"]), **c)
        _CACHE[name] = (a, reference(a))
    return _CACHE[name]


def constructed():
    """The issue's case that says the numbers mean something: 130 EEPs, a power-law mass function, three bands; star A has
    exactly the magnitudes of EEP index 70, star B those of the pair (70, 60)."""
    i = np.arange(130)
    eep = 200.0 + 2.0 * i
    mass = 0.6 + 1.2 * i / 129.0
    mass_term = -2.35 * np.log(mass) + np.log(1.2 / 129.0 / 2.0)
    lm = np.log10(mass)
    mags = np.stack([8.0 - 6.0 * lm, 7.5 - 4.5 * lm, 7.0 - 3.0 * lm])                       # [3, 130]
    flux = 10.0 ** (-0.4 * mags)
    gamma, minq, fB = 0.3, 0.1, 0.3
    g1 = gamma + 1.0
    cols = np.concatenate([eep[None], mass[None], mass_term[None], flux, mags])[None]
    rowpar = np.array([[np.log(fB), np.log(1.0 - fB), gamma, np.log(g1 / (1.0 - minq ** g1))]])
    star_a = mags[:, 70]
    star_b = -2.5 * np.log10(flux[:, 70] + flux[:, 60])
    star_val = np.ascontiguousarray(np.stack([star_a, star_b], axis=1))
    star_w = np.full((3, 2), 1.0 / 0.02 ** 2)
    return dict(cols=np.ascontiguousarray(cols), n_valid=np.array([130], np.int32), rowpar=rowpar, star_val=star_val,
                star_w=star_w, minq=minq, nb=3, npr=0, ld=130, ns=2)


# -- calls ---------------------------------------------------------------------------------------------------------------
def call(lib, a, device=None, rows=None, stream=None, **over):
    """``iso_members_moments_host`` on the numpy inputs or, with ``device`` (a torch device), ``iso_members_moments`` on copies
    there; ``rows``: the rows to pass (default: all); ``over``: arguments to pass instead of the case's (n_bands, n_props,
    cols, ...; a pointer given as None is a null pointer).  Returns ``(rc, ln_like [P, N_s], moments [P, N_s, 11], work
    [P, N_s, 6, ld])`` as numpy; what the call does not write keeps the fill value -7, and on the device every output lies
    between two margins of -7 that have to stay so."""
    rows = np.arange(a["n_valid"].size) if rows is None else np.asarray(rows)
    P, ns, ld = rows.size, a["ns"], a["ld"]
    arrays = dict(cols=np.ascontiguousarray(a["cols"][rows]), n_valid=np.ascontiguousarray(a["n_valid"][rows], dtype=np.int32),
                  rowpar=np.ascontiguousarray(a["rowpar"][rows]), star_val=np.ascontiguousarray(a["star_val"]),
                  star_w=np.ascontiguousarray(a["star_w"]))
    shapes = dict(work=(P, ns, NINNER, ld), ln_like=(P, ns), moments=(P, ns, NMOM))
    if device is None:
        outs = {k: np.full(s, FILL) for k, s in shapes.items()}
        ptr = lambda x: C.c_void_p(x.ctypes.data)                                            # noqa: E731
        fn, st = lib.iso_members_moments_host, None
    else:
        import torch
        arrays = {k: torch.from_numpy(x).to(device) for k, x in arrays.items()}
        flats = {k: torch.full((int(np.prod(s)) + 2 * MARGIN,), FILL, dtype=torch.float64, device=device)
                 for k, s in shapes.items()}
        outs = {k: flats[k][MARGIN:MARGIN + int(np.prod(s))] for k, s in shapes.items()}
        ptr = lambda x: C.c_void_p(x.data_ptr())                                             # noqa: E731
        fn = lib.iso_members_moments
        cur = torch.cuda.current_stream(device)
        cur.synchronize()
        st = C.c_void_p((cur if stream is None else stream).cuda_stream)
    p = {k: ptr(x) for k, x in {**arrays, **outs}.items()}
    for k in list(over):
        if k in p:
            v = over.pop(k)
            p[k] = C.c_void_p(0) if v is None else v
    rc = fn(p["cols"], over.get("ld", ld), over.get("n_rows", P), p["n_valid"], p["rowpar"], p["star_val"], p["star_w"],
            over.get("n_stars", ns), over.get("n_bands", a["nb"]), over.get("n_props", a["npr"]), float(a["minq"]), p["work"],
            p["ln_like"], p["moments"], st)
    if device is not None:
        torch.cuda.synchronize(device)
        for k, f in flats.items():
            assert bool((f[:MARGIN] == FILL).all()) and bool((f[-MARGIN:] == FILL).all()), "%s: a write outside it" % k
        outs = {k: x.cpu().numpy() for k, x in outs.items()}
    return rc, outs["ln_like"].reshape(shapes["ln_like"]), outs["moments"].reshape(shapes["moments"]), \
        outs["work"].reshape(shapes["work"])


def close(got, want, what, worst=None):
    """Same NaN / -inf / +inf pattern and |got - want| <= TOL (1 + |want|) elsewhere; returns the largest error over its
    limit's TOL-free part (and keeps the largest in ``worst[what]``)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    for kind, f in (("NaN", np.isnan), ("-inf", np.isneginf), ("+inf", np.isposinf)):
        assert np.array_equal(f(got), f(want)), (what, kind + " pattern", np.argwhere(f(got) != f(want))[:5])
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / (1 + np.abs(want[fin]))
    e = float(err.max()) if err.size else 0.0
    if worst is not None:
        worst[what] = max(worst.get(what, 0.0), e)
    assert e <= TOL, (what, e)
    return e


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
