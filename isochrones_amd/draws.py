"""Random draws of synthetic populations and injection sets by libiso_draw.so (``iso_draw_systems``; the definition is in
include/isochrones_amd_draw.h): every column of every system from counter-based uniforms (Philox4x32-10) through an exact
inverse distribution function, on the device where the columns are used or, with ``device=None``, through the library's host
entry.  A system's draws depend on ``(seed, global number, stream, round)`` only, so a population can be redrawn row by row
and extended without changing the rows it has.

A :class:`DrawPlan` is a list of columns, each one of

* a device prior (``isochrones_amd.priors.DEVICE_PRIOR_TYPES``),
* a population family bound to one row of hyper-parameters (:func:`bound`, or the pair ``(family, theta_row)``),
* a float (a constant),
* a frozen ``scipy.stats.uniform`` of ages in Gyr (a star-formation history): uniform in linear age, drawn as log10 years,
* one of the columns made by :func:`table`, :func:`lingauss`, :func:`powerlaw`, :func:`truncgauss`,
* anything else that has ``sample`` or ``rvs``: a *host column*, drawn from ``numpy.random.default_rng([seed, round])`` and
  uploaded (``plan.host_columns`` names them).  A call's n systems take the generator's first n values whatever ``first``
  and ``index`` are: a host column is reproducible per (seed, round, n), not per system, and every round has fresh values.

:func:`uniforms` returns the uniforms behind a column's draws (``iso_draw_uniforms_host``), for twins and tests."""
from __future__ import annotations

import math

import numpy as np

from . import _draw_cabi as dc, device as dev
from . import priors as _p

_ROOT2 = math.sqrt(2.0)


def _phi(z):
    z = float(z)
    if z == -math.inf:
        return 0.0
    if z == math.inf:
        return 1.0
    return 0.5 * math.erfc(-z / _ROOT2)


class Column:
    """One device column: the fields of an ``iso_draw_record``, the name of its parent and its table, if any."""

    def __init__(self, kind, lo, hi, p=(), on=None, table=None):
        self.kind, self.lo, self.hi, self.on, self.table = int(kind), float(lo), float(hi), on, table
        self.p = [float(v) for v in p] + [0.0] * (dc.NPAR - len(p))
        if len(self.p) != dc.NPAR:
            raise ValueError("a draw record has %d parameters" % dc.NPAR)


def _window(mu, sigma, lo, hi, what):
    """(Phi(a), Phi(b) - Phi(a), flip) of a Gaussian's standardised bounds, the mass taken in the lower tail."""
    if not sigma > 0:
        raise ValueError("%s: sigma must be positive" % what)
    a, b = (lo - mu) / sigma, (hi - mu) / sigma
    flip = a > 0
    if flip:
        a, b = -b, -a
    fa, fb = _phi(a), _phi(b)
    if not fb - fa > 0:
        raise ValueError("%s: the window [%g, %g] holds no mass of the Gaussian (%g, %g)" % (what, lo, hi, mu, sigma))
    return fa, fb - fa, 1.0 if flip else 0.0


def _plaw(a1, lo, hi, what):
    """(a1, E, mode) of the header's power-law inverse on [lo, hi]."""
    if not (0 <= lo < hi < math.inf):
        raise ValueError("%s: a power law needs bounds 0 <= lo < hi, finite" % what)
    if lo == 0:
        if not a1 > 0:
            raise ValueError("%s: a power law from 0 needs alpha > -1" % what)
        return a1, 0.0, 2.0
    span = math.log(hi / lo)
    if a1 == 0:
        return 0.0, span, 1.0
    try:
        E = math.expm1(a1 * span)
    except OverflowError:
        raise ValueError("%s: hi^(alpha + 1) / lo^(alpha + 1) overflows" % what)
    return a1, E, 0.0


def powerlaw(alpha, bounds):
    """x^alpha on ``bounds`` (alpha = -1 included; lo = 0 for alpha > -1)."""
    lo, hi = float(bounds[0]), float(bounds[1])
    return Column(dc.POWERLAW, lo, hi, _plaw(float(alpha) + 1.0, lo, hi, "powerlaw"))


def truncgauss(mean, sigma, bounds=None):
    """A Gaussian, renormalised on ``bounds`` if given."""
    if bounds is None:
        if not sigma > 0:
            raise ValueError("truncgauss: sigma must be positive")
        return Column(dc.GAUSS, -math.inf, math.inf, (mean, sigma, 0.0, 1.0, 0.0))
    lo, hi = float(bounds[0]), float(bounds[1])
    return Column(dc.TRUNCGAUSS, lo, hi, (mean, sigma) + _window(float(mean), float(sigma), lo, hi, "truncgauss"))


def lingauss(on, bounds, intercept, slope, sigma, pivot=0.0):
    """A Gaussian renormalised on ``bounds`` about ``intercept + slope * (x_on - pivot)``, ``on`` another column of the plan."""
    lo, hi = float(bounds[0]), float(bounds[1])
    if not (lo < hi and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("lingauss needs finite bounds lo < hi")
    if not sigma > 0:
        raise ValueError("lingauss: sigma must be positive")
    return Column(dc.LINGAUSS, lo, hi, (intercept, sigma, 0.0, 1.0 / sigma, slope, pivot), on=str(on))


def table(edges, masses, given=None, parent_edges=None):
    """A piecewise-constant density: ``masses`` [K] over the bins ``edges`` [K + 1]; with ``given`` (another column of the
    plan) ``masses`` is [parent bins, K], one row per bin of ``parent_edges``."""
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    K = edges.size - 1
    if edges.ndim != 1 or K < 1 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
        raise ValueError("a table needs at least 2 finite, strictly increasing edges")
    if K > dc.MAX_BINS:
        raise ValueError("a table has at most %d bins (got %d)" % (dc.MAX_BINS, K))
    m = np.atleast_2d(np.asarray(masses, dtype=np.float64))
    if m.ndim != 2 or m.shape[1] != K or not np.all(m >= 0) or not np.all(m.sum(axis=1) > 0) or not np.all(np.isfinite(m)):
        raise ValueError("masses must be [%s%d], not negative, with a positive finite sum" % ("parent bins, " if given else "", K))
    cum = np.concatenate([np.zeros((m.shape[0], 1)), np.cumsum(m, axis=1)], axis=1)
    cum = cum / cum[:, -1:]
    cum[:, -1] = 1.0
    cum = np.minimum.accumulate(cum[:, ::-1], axis=1)[:, ::-1]          # (rounding: never above what follows)
    if given is None:
        if m.shape[0] != 1:
            raise ValueError("masses of a table without a parent must be [K]")
        pe = None
    else:
        pe = np.ascontiguousarray(parent_edges, dtype=np.float64)
        if pe.ndim != 1 or pe.size - 1 != m.shape[0] or not np.all(np.diff(pe) > 0):
            raise ValueError("parent_edges must be the %d + 1 ascending edges of the parent's bins" % m.shape[0])
        if pe.size - 1 > dc.MAX_BINS:
            raise ValueError("a table's parent has at most %d bins" % dc.MAX_BINS)
    return Column(dc.TABLE, edges[0], edges[-1], (0.0, K, 0 if pe is None else pe.size - 1, 0.0),
                  on=None if given is None else str(given), table=(edges, np.ascontiguousarray(cum), pe))


def prior_column(prior):
    """The column of a device prior: the exact inverse of its distribution function on its bounds."""
    lo, hi = (float(b) for b in prior.bounds)
    name = type(prior).__name__
    if isinstance(prior, _p.FlatPrior):
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError("%s needs finite bounds" % name)
        return Column(dc.FLAT, lo, hi)
    if isinstance(prior, _p.FlatLogPrior):
        with np.errstate(all="ignore"):
            return Column(dc.FLATLOG, lo, hi, (10.0 ** lo, 10.0 ** hi - 10.0 ** lo))
    if isinstance(prior, _p.PowerLawPrior):
        return Column(dc.POWERLAW, lo, hi, _plaw(prior.alpha + 1.0, lo, hi, name))
    if isinstance(prior, _p.GaussianPrior):
        return truncgauss(prior.mean, prior.sigma, (lo, hi) if prior.bounded else None)
    if isinstance(prior, _p.LogNormalPrior):
        return Column(dc.LOGNORMAL, 0.0, math.inf, (prior.mu, prior.sigma))
    if isinstance(prior, _p.ChabrierPrior):
        return _chabrier(prior, lo, hi)
    if isinstance(prior, _p.FehPrior):
        return _feh(prior, lo, hi)
    raise TypeError("no device draw for %r" % (prior,))


def _chabrier(prior, lo, hi):
    low, high, bp = prior.low, prior.high, prior.breakpoint
    mu, s = low.mu, low.sigma
    plo, phi = (float(b) for b in high.bounds)
    a1 = high.alpha + 1.0
    # the lognormal piece on [l0, l1], the power law on [q0, q1]: the bounds met with each piece's own support
    l0, l1 = max(lo, 0.0), min(hi, bp)
    q0, q1 = max(lo, bp, plo), min(hi, phi)
    p = [0.0] * dc.NPAR
    m_low = m_high = 0.0
    if l1 > l0:
        za = (math.log(l0) - mu) / s if l0 > 0 else -math.inf
        zb = (math.log(l1) - mu) / s
        flip = za > 0
        if flip:
            za, zb = -zb, -za
        fa, fb = _phi(za), _phi(zb)
        m_low = fb - fa
        p[1:6] = mu, s, fa, fb - fa, 1.0 if flip else 0.0
    if q1 > q0:
        ratio = high(bp) / low(bp)
        b1, E, mode = _plaw(a1, q0, q1, "ChabrierPrior")
        inner = E if mode == 1.0 else E / b1                    # the integral of x^alpha over the window / q0^a1
        m_high = high._C() * q0 ** a1 * inner / ratio
        p[6:10] = b1, E, q0, mode
    if not m_low + m_high > 0:
        raise ValueError("ChabrierPrior: the bounds (%g, %g) hold no mass" % (lo, hi))
    p[0] = m_low / (m_low + m_high)
    if m_high == 0.0:
        p[0], p[8] = 1.0, 1.0
    return Column(dc.CHABRIER, lo, hi, p)


def _feh(prior, lo, hi):
    comps = ([(0.8, 0.016, 0.15), (0.2, -0.15, 0.22)] if prior.local else [(1.0, -0.3, 0.3)])
    comps = [(w * (1 - prior.halo_fraction), m, s) for w, m, s in comps] + [(prior.halo_fraction, -1.5, 0.4)]
    p = [0.0] * dc.NPAR
    p[0] = 1.0 if prior.local else 0.0
    weights, flips = [], 0
    for k, (w, m, s) in enumerate(comps):
        a, b = (lo - m) / s, (hi - m) / s
        flip = a > 0
        if flip:
            a, b = -b, -a
        fa, fb = _phi(a), _phi(b)
        p[3 + 2 * k], p[4 + 2 * k] = fa, fb - fa
        flips |= (1 << k) if flip else 0
        weights.append(w * (fb - fa))
    tot = sum(weights)
    if not tot > 0:
        raise ValueError("FehPrior: the window [%g, %g] holds no mass" % (lo, hi))
    cum = np.cumsum(weights) / tot
    p[1] = float(cum[0])
    p[2] = float(cum[1]) if len(comps) == 3 else 1.0
    p[9] = float(flips)
    return Column(dc.FEH, lo, hi, p)


def bound(family, theta=()):
    """The column of a population family of :mod:`isochrones_amd.hierarchical` / :mod:`isochrones_amd.relations` at one row of
    its hyper-parameters (a Histogram is bound by ``PopulationModel.sample``, which knows the grid)."""
    from . import hierarchical as h
    from .relations import LinearGaussian
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if theta.size != len(family.names):
        raise ValueError("%s takes %d hyper-parameters (%s), got %d" % (type(family).__name__, len(family.names),
                                                                          ", ".join(family.names), theta.size))
    if isinstance(family, h.PowerLaw):
        return powerlaw(theta[0], family.bounds)
    if isinstance(family, h.TruncatedGaussian):
        return truncgauss(theta[0], theta[1], family.bounds)
    if isinstance(family, h.Fixed):
        return prior_column(family.prior)
    if isinstance(family, LinearGaussian):
        return lingauss(family.on, family.bounds, theta[0], theta[1], theta[2], family.pivot)
    raise TypeError("no draw for the family %r" % (family,))


def _is_scipy_uniform(x):
    return getattr(getattr(x, "dist", None), "name", None) == "uniform" and hasattr(x, "support")


def _column(spec):
    """A :class:`Column`, or None for a host column."""
    from .hierarchical import _Family
    if isinstance(spec, Column):
        return spec
    if not _p.is_host_prior(spec):
        return prior_column(spec)
    if isinstance(spec, _p.DEVICE_PRIOR_TYPES):      # a subclass with a density of its own: its sample() is the parent's
        raise TypeError("a column of a DrawPlan is a device prior, a bound family, a float, a scipy uniform or an object "
                        "with sample / rvs (got %r, which overrides its family's density)" % (spec,))
    if isinstance(spec, _Family):
        return bound(spec)
    if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], _Family):
        return bound(*spec)
    if isinstance(spec, (int, float, np.floating, np.integer)) and not isinstance(spec, bool):
        return Column(dc.CONSTANT, -math.inf, math.inf, (float(spec),))
    if _is_scipy_uniform(spec):
        a, b = (float(v) for v in spec.support())
        with np.errstate(divide="ignore"):
            lo, hi = (float(v) for v in np.log10(1e9 * np.array([a, b])))
        return prior_column(_p.FlatLogPrior((lo, hi)))
    if hasattr(spec, "sample") or hasattr(spec, "rvs"):
        return None
    raise TypeError("a column of a DrawPlan is a device prior, a bound family, a float, a scipy uniform or an object with "
                    "sample / rvs (got %r)" % (spec,))


class DrawPlan:
    """``DrawPlan({"mass": ChabrierPrior(), "feh": FehPrior(), "distance": 10.0})``; ``streams`` = ``{name: 0 .. 255}`` gives
    a column its number in the Philox counter (default: its place in the plan), so that a column keeps its draws when the
    plan around it changes."""

    def __init__(self, columns, streams=None):
        columns = dict(columns)
        if not columns:
            raise ValueError("a DrawPlan needs at least one column")
        streams = dict(streams or {})
        self.names = tuple(columns)
        self.specs = columns
        cols = {name: _column(spec) for name, spec in columns.items()}
        #: the columns drawn on the host from ``numpy.random.default_rng([seed, round])``
        self.host_columns = tuple(n for n in self.names if cols[n] is None)
        self.device_columns = tuple(n for n in self.names if cols[n] is not None)
        C_ = len(self.device_columns)
        if C_ > dc.MAX_COLS:
            raise ValueError("a DrawPlan has at most %d device columns, got %d (C = %d is refused)" % (dc.MAX_COLS, C_, C_))
        rec = np.zeros(max(C_, 1), dtype=dc.RECORD)[:C_]
        tables, parents = [], []
        at = 0
        for q, name in enumerate(self.device_columns):
            col = cols[name]
            stream = int(streams.get(name, self.names.index(name)))
            if not 0 <= stream <= 255:
                raise ValueError("the stream of %r must be 0 to 255" % (name,))
            parent = -1
            if col.on is not None:
                if col.on == name:
                    raise ValueError("column %r follows itself" % (name,))
                if col.on not in self.device_columns:
                    raise ValueError("column %r follows %r, which is no device column of the plan (parent out of range)"
                                     % (name, col.on))
                parent = self.device_columns.index(col.on)
            parents.append(parent)
            p = list(col.p)
            if col.table is not None:
                edges, cum, pe = col.table
                p[0] = float(at)
                tables += [edges, cum.reshape(-1)]
                at += edges.size + cum.size
                if pe is not None:
                    p[3] = float(at)
                    tables.append(pe)
                    at += pe.size
            rec[q] = (col.kind, parent, stream, 0, col.lo, col.hi, p)
        self.records = rec
        self.parents = tuple(parents)
        self.order = np.asarray(self._order(), dtype=np.int32)
        self.tables = np.ascontiguousarray(np.concatenate(tables)) if tables else np.zeros(0)
        self._device_tables = {}

    def _order(self):
        """The device columns, a parent before its child; a cycle is refused."""
        order, state = [], {}

        def visit(q):
            if state.get(q) == 1:
                raise ValueError("the links of the plan form a cycle through %r" % (self.device_columns[q],))
            if state.get(q) == 2:
                return
            state[q] = 1
            if self.parents[q] >= 0:
                visit(self.parents[q])
            state[q] = 2
            order.append(q)

        for q in range(len(self.parents)):
            visit(q)
        return order

    def _host_draws(self, n, seed, round):
        # one generator per (seed, round): a redraw round (StarPopulation.generate, exact_N) must not hand the redrawn systems
        # the values the first systems of the round before had
        rng = np.random.default_rng([seed, int(round)])
        out = {}
        for name in self.host_columns:
            spec = self.specs[name]
            if hasattr(spec, "sample"):
                out[name] = np.ascontiguousarray(spec.sample(n, rng), dtype=np.float64)
            else:
                out[name] = np.ascontiguousarray(spec.rvs(n, random_state=rng), dtype=np.float64)
        return out

    def draw(self, n, seed, round=0, first=0, index=None, device=None):
        """``{name: [n]}``: CUDA tensors on ``device`` (an index or a torch device), drawn by ``iso_draw_systems`` on the
        current stream, or with ``device=None`` numpy arrays from ``iso_draw_systems_host``.  System i has the global number
        ``index[i]`` (an int64 array or tensor) or ``first + i``."""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        C_ = len(self.device_columns)
        lib = dc.lib()
        host = self._host_draws(n, seed, round) if self.host_columns else {}
        if device is None:
            x = np.empty((C_, n))
            if index is not None:
                index = np.ascontiguousarray(_to_host(index), dtype=np.int64)
                if index.shape != (n,):
                    raise ValueError("index must be [n] = [%d]" % n)
            if C_ and n:
                dc.check(lib.iso_draw_systems_host(
                    self.records.ctypes.data, C_, self.order.ctypes.data, self.tables.ctypes.data if self.tables.size else None,
                    self.tables.size, seed, int(round), int(first), None if index is None else index.ctypes.data, n,
                    x.ctypes.data, None))
            out = {name: x[q] for q, name in enumerate(self.device_columns)}
            out.update(host)
            return {name: out[name] for name in self.names}
        import torch
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type != "cuda":
            raise ValueError("device must be a CUDA device or None (the host entry)")
        di = device.index if device.index is not None else dev.current_device()
        device = torch.device("cuda", di)
        x = torch.empty((C_, n), dtype=torch.float64, device=device)
        if index is not None:
            index = (index if dev.is_tensor(index) else torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)))
            index = index.to(device=device, dtype=torch.int64).contiguous()
            if tuple(index.shape) != (n,):
                raise ValueError("index must be [n] = [%d]" % n)
        tb = None
        if self.tables.size:
            if di not in self._device_tables:
                self._device_tables[di] = torch.from_numpy(self.tables).to(device)
            tb = self._device_tables[di]
        if C_ and n:
            with torch.cuda.device(di):
                dc.check(lib.iso_draw_systems(
                    self.records.ctypes.data, C_, self.order.ctypes.data, dev.ptr(tb), self.tables.size, seed, int(round),
                    int(first), dev.ptr(index), n, dev.ptr(x), dev.stream_ptr(di)))
        out = {name: x[q] for q, name in enumerate(self.device_columns)}
        out.update({name: torch.from_numpy(v).to(device) for name, v in host.items()})
        return {name: out[name] for name in self.names}


def _to_host(a):
    return a.detach().cpu().numpy() if dev.is_tensor(a) else np.asarray(a)


def uniforms(seed, j, column, round=0):
    """``[n, 2]``: the uniforms (u0, u1) of the systems ``j`` for the stream ``column`` (``iso_draw_uniforms_host``)."""
    j = np.ascontiguousarray(j, dtype=np.int64).reshape(-1)
    u = np.empty((j.size, 2))
    dc.check(dc.lib().iso_draw_uniforms_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(round), j.ctypes.data, j.size, int(column),
                                             u.ctypes.data))
    return u
