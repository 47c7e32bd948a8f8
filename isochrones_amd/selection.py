"""Selection effects in the hierarchical population likelihood from an injection set.  A magnitude-limited catalog holds
the stars of the population that could be detected, not the population; the likelihood of
:mod:`isochrones_amd.hierarchical` corrected for that is (Mandel, Farr & Gair 2019)

    ln L_sel(theta) = sum_s ell_s(theta) - S_unmasked * ln alpha(theta),

with alpha(theta) the fraction of the population ``theta`` that the survey detects.  alpha is estimated from a large set of
*injections*: stars drawn from a known density g, pushed through the model grid and the survey's cut, and reweighted to
every hyper row (Farr 2019),

    alpha(theta) = (1/J) sum_j d_j  prod_q f_q(x_jq; theta) / g_q(x_jq),

by the HIP kernels of libiso_select.so (``iso_select_alpha``; the definition is in include/isochrones_amd_select.h), which
also return the effective number of injections n_eff behind every row's estimate.  ``PopulationPosterior(...,
injections=InjectionSet...)`` applies the correction; its ``lnpost`` refuses a row whose estimate rests on fewer than
``min_neff_factor`` * S effective injections (Farr 2019's condition: below it the error of alpha biases the posterior).

A drawn column that the population model does not name is assumed to follow its draw density in the population: its ratio
f / g is one and it enters alpha through the detection probability only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _select_cabi as sc, device as dev
from .hierarchical import prior_record

#: the arguments of ``evaluate_binaries`` an injection set may draw, with the value of an argument that is not drawn
_TRACK_COLUMNS = {"mass": None, "age": None, "feh": None, "distance": 10.0, "AV": 0.0}


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else dev.ptr(a)


def _host(a):
    return a.detach().cpu().numpy() if dev.is_tensor(a) else np.asarray(a)


def detection_lnd(mags, limits):
    """``(lnd [J], off [J] bool)`` of the magnitudes ``mags`` = ``{band: [J] tensor}`` under ``limits`` =
    ``{band: (faint_limit, sigma)}``, as :meth:`InjectionSet.draw` states it: a handful of framework ops, run once per
    injection set (not a kernel, by design)."""
    import torch
    lnd, off = None, None
    for band, (limit, sigma) in limits.items():
        mag = mags[band]
        nan = torch.isnan(mag)
        off = nan if off is None else off | nan
        if sigma > 0:
            term = torch.special.log_ndtr((float(limit) - mag) / float(sigma))
        else:
            term = torch.where(mag <= float(limit), 0.0, -np.inf).to(torch.float64)
        lnd = term if lnd is None else lnd + term
    return torch.where(off, -np.inf, lnd).contiguous(), off


class InjectionSet:
    """``columns``: ``{name: [J] numpy array or CUDA tensor}``, the injections in the coordinates the population model's
    columns are stated in (on evolution tracks ``mass``, ``age`` as log10 years, ``feh``, ``distance``, ``AV``); ``draw``:
    ``{name: prior}``, the density every column was drawn from, one of ``isochrones_amd.priors.DEVICE_PRIOR_TYPES``;
    ``lnd``: [J], the natural log of every injection's detection probability (-inf: not detected, 0: certainly)."""

    def __init__(self, columns, draw, lnd, n_off=None):
        self.columns = {name: v if dev.is_tensor(v) else np.asarray(v, dtype=np.float64) for name, v in dict(columns).items()}
        lnd = lnd if dev.is_tensor(lnd) else np.asarray(lnd, dtype=np.float64)
        #: the density every column was drawn from
        self.priors = dict(draw)
        if not self.columns:
            raise ValueError("an injection set needs at least one column")
        sizes = {int(v.shape[0]) if len(v.shape) == 1 else -1 for v in self.columns.values()}
        if len(sizes) != 1 or -1 in sizes:
            raise ValueError("every column of an injection set is one [J] array")
        self.J = sizes.pop()
        if self.J < 1:
            raise ValueError("an injection set needs at least one injection")
        if tuple(lnd.shape) != (self.J,):
            raise ValueError("lnd must be [J] = [%d], got %s" % (self.J, tuple(lnd.shape)))
        self.lnd = lnd
        for name in self.priors:
            if name not in self.columns:
                raise ValueError("draw prior for %r, which is not a column of the injection set" % (name,))
        #: ``iso_hier_record`` of every draw density (a host-evaluated prior is refused here)
        self.records = {name: prior_record(p) for name, p in self.priors.items()}
        #: injections off the model or BC grid (:meth:`draw` counts them; they are undetected and stay in J)
        self.n_off = n_off

    _backend = None                                             # (the CPU tests route the evaluation to the host entries)

    @classmethod
    def draw(cls, ic, draw, n, limits, seed=None, accurate="exact", rng="numpy"):
        """``n`` single stars drawn on the host from ``draw`` = ``{column: prior}`` (``mass``, ``age``, ``feh`` and
        optionally ``distance``, ``AV``; one ``numpy.random.default_rng(seed)``, ``prior.sample(n, rng)`` in the order of
        ``draw``), evaluated on the model and BC grid by :func:`isochrones_amd.populations.evaluate_binaries` (one EEP solve,
        one ``iso_population_eval`` launch) and cut by ``limits`` = ``{band: (faint_limit, sigma)}``: with sigma > 0 a
        band's term of ``lnd`` is ``log_ndtr((limit - mag) / sigma)``, the chance that a magnitude observed with Gaussian
        noise sigma passes; with sigma = 0 it is 0 where ``mag <= limit`` and -inf elsewhere.  The terms are added over
        the bands in the order given.  An injection off the grid (a NaN magnitude) is a star that cannot be observed:
        ``lnd`` = -inf; ``n_off`` counts them.  ``rng="philox"`` draws the columns on the device instead
        (:class:`isochrones_amd.draws.DrawPlan`, ``seed=None`` is 0): they never visit the host."""
        from .populations import evaluate_binaries
        draw = dict(draw)
        for name in draw:
            if name not in _TRACK_COLUMNS:
                raise ValueError("an injection set on tracks draws %s; got %r" % (", ".join(_TRACK_COLUMNS), name))
        for name, default in _TRACK_COLUMNS.items():
            if default is None and name not in draw:
                raise ValueError("no draw prior for %r" % (name,))
        if not limits:
            raise ValueError("limits = {band: (faint_limit, sigma)} needs at least one band")
        for band, (_, sigma) in limits.items():
            if not sigma >= 0:
                raise ValueError("the sigma of band %r must be 0 or positive" % (band,))
        records = {name: prior_record(p) for name, p in draw.items()}          # refuses a host-evaluated prior before any work
        del records
        if rng not in ("numpy", "philox"):
            raise ValueError("rng is 'numpy' or 'philox'")
        on_host = getattr(cls._backend, "device", None) == "host"
        if rng == "philox":
            from .draws import DrawPlan
            streams = {name: k for k, name in enumerate(_TRACK_COLUMNS)}
            cols = DrawPlan(draw, streams={name: streams[name] for name in draw}).draw(
                int(n), 0 if seed is None else int(seed), device=None if on_host else dev.current_device())
        else:
            rng = np.random.default_rng(seed)
            cols = {name: np.ascontiguousarray(p.sample(int(n), rng), dtype=np.float64) for name, p in draw.items()}
        args = {name: cols.get(name, default) for name, default in _TRACK_COLUMNS.items()}
        bands = tuple(limits)
        out = evaluate_binaries(ic, args["mass"], 0.0, args["age"], args["feh"], args["distance"], args["AV"], bands=bands,
                                props=("mass",), accurate=accurate, _backend=cls._backend)
        if on_host:                                             # detection_lnd is stated in framework ops
            import torch
            lnd, off = detection_lnd({band: torch.from_numpy(np.ascontiguousarray(out["%s_mag" % band])) for band in bands}, limits)
            return cls(cols, draw, lnd.numpy(), n_off=int(off.sum().item()))
        lnd, off = detection_lnd({band: out["%s_mag" % band] for band in bands}, limits)
        return cls(cols, draw, lnd, n_off=int(off.sum().item()))


class Selection:
    """The injection set of a :class:`~isochrones_amd.hierarchical.PopulationPosterior`, packed for its population model
    and moved once to where the chain lies (``device``: a torch device, or None for a host chain)."""

    def __init__(self, injections, model, device):
        if not isinstance(injections, InjectionSet):
            raise TypeError("injections must be an InjectionSet (got %r)" % (injections,))
        for col in model.columns:
            if col not in injections.columns or col not in injections.records:
                raise ValueError("the injection set has no column %r with a draw prior (it has %s)"
                                 % (col, ", ".join(sorted(injections.records)) or "none"))
        self.model, self.device, self.J, self.Q = model, device, injections.J, len(model.columns)
        x = [injections.columns[c] for c in model.columns]
        draw = np.concatenate([injections.records[c] for c in model.columns])
        if device is None:
            self.x = np.ascontiguousarray(np.stack([_host(v) for v in x]), dtype=np.float64)
            self.lnd = np.ascontiguousarray(_host(injections.lnd), dtype=np.float64)
            self.draw = draw
        else:
            import torch
            to = lambda v: (v if dev.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(device=device, dtype=torch.float64)
            self.x = torch.stack([to(v) for v in x]).contiguous()
            self.lnd = to(injections.lnd).contiguous()
            self.draw = torch.from_numpy(draw.view(np.uint8).copy()).to(device)

    def alpha(self, theta):
        """``(ln_alpha [H], n_eff [H], n_bad)`` of the rows ``theta`` [H, P] where the injections lie: numpy arrays for a
        host set, CUDA tensors otherwise."""
        rows = np.ascontiguousarray(self.model.pack(theta))
        H = rows.shape[0]
        lib = sc.lib()
        if self.device is None:
            la, ne, nb = np.empty(H), np.empty(H), np.empty(1, dtype=np.int32)
            sc.check(lib.iso_select_alpha_host(_ptr(self.x), self.Q, self.J, _ptr(self.lnd), _ptr(self.draw), _ptr(rows), H, None,
                                               _ptr(la), _ptr(ne), _ptr(nb), None))
            return la, ne, nb
        import torch
        f64 = dict(dtype=torch.float64, device=self.device)
        drows = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(self.device)
        ws = torch.empty(int(lib.iso_select_workspace_doubles(self.J, H)), **f64)
        la, ne = torch.empty(H, **f64), torch.empty(H, **f64)
        nb = torch.empty(1, dtype=torch.int32, device=self.device)
        sc.check(lib.iso_select_alpha(_ptr(self.x), self.Q, self.J, _ptr(self.lnd), _ptr(self.draw), _ptr(drows), H, _ptr(ws),
                                      _ptr(la), _ptr(ne), _ptr(nb), dev.stream_ptr(self.device.index)))
        return la, ne, nb
