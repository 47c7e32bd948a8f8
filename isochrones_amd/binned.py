"""Population densities without a shape: a histogram over one column (an age distribution, a star-formation history, a
metallicity distribution) or over one column per bin of another (the non-parametric form of an age-metallicity relation).
The mean importance weight of a star under a piecewise-constant density is linear in the cell heights,

    (1/M) sum_m f(x_m; theta) / f0(x_m) = (1/M) sum_b h_b(theta) A[s][b],   A[s][b] = sum_{m in cell b} 1 / f0(x_m),

so :class:`~isochrones_amd.hierarchical.PopulationPosterior` reads the chain once, compresses it to a table of B numbers per
star (``iso_binned_compress``) and answers every likelihood call after that with a contraction of the table
(``iso_binned_lnlike``); the kernels are libiso_binned.so's (include/isochrones_amd_binned.h).  A model with a
:class:`Histogram` is *binned*; its other columns are :class:`~isochrones_amd.hierarchical.Fixed`.  The selection term of an
injection set is the same compression of the injections, one star of J samples (:class:`BinnedSelection`)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _binned_cabi as bc, _cabi, device as dev
from .hierarchical import _Binned


class Histogram(_Binned):
    """A density that is constant on each of the K bins ``edges`` (K + 1 strictly increasing finite values, uniform or
    not).  The bin probabilities are ``softmax(a)`` of the logits ``a0 = 0, a1 .. a{K-1}``, the free parameters, each flat in
    the range ``logits``; the log density of bin k is ``log_softmax(a)_k - ln(width_k)``.  ``given="age"`` makes it
    conditional on the bin of another Histogram column of the model: one set of K - 1 logits per parent bin, named
    ``a<j>|<parent bin>``.  A value falls in bin k if ``edges[k] <= x < edges[k + 1]``, the last bin closed above
    (``numpy.histogram``'s rule)."""

    def __init__(self, edges, logits=(-10.0, 10.0), given=None):
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        if self.edges.ndim != 1 or self.edges.size < 2 or not np.all(np.isfinite(self.edges)) or not np.all(np.diff(self.edges) > 0):
            raise ValueError("Histogram needs at least 2 finite, strictly increasing edges")
        if given is not None and not isinstance(given, str):
            raise TypeError("given must be the name of another Histogram column of the model (got %r)" % (given,))
        self.given = given
        self.logits = (float(logits[0]), float(logits[1]))
        if not self.logits[0] < self.logits[1]:
            raise ValueError("the range of the logits must be (lo, hi) with lo < hi")
        self.n_bins = self.edges.size - 1
        self._bind(None)

    def _bind(self, parent_bins):
        """Called by ``PopulationModel`` on its own copy of the family: the number of bins of the column this one is given,
        or None."""
        self.parent_bins = 1 if parent_bins is None else int(parent_bins)
        if parent_bins is None:
            self.names = tuple("a%d" % j for j in range(1, self.n_bins))
        else:
            self.names = tuple("a%d|%d" % (j, k) for k in range(self.parent_bins) for j in range(1, self.n_bins))
        self.ranges = (self.logits,) * len(self.names)

    def lnheights(self, theta):
        """``theta`` [H, len(names)] -> the log density of every bin, [H, parent bins (1 without ``given``), K]."""
        theta = np.asarray(theta, dtype=np.float64)
        H = theta.shape[0]
        a = np.concatenate([np.zeros((H, self.parent_bins, 1)), theta.reshape(H, self.parent_bins, self.n_bins - 1)], axis=2)
        top = a.max(axis=2, keepdims=True)
        lse = top + np.log(np.sum(np.exp(a - top), axis=2, keepdims=True))
        return (a - lse) - np.log(np.diff(self.edges))

    def fill(self, rec, theta):
        raise ValueError("a Histogram has no record per row: a binned model's rows are PopulationModel.cell_table(theta)")


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else dev.ptr(a)


def _host(a):
    return a.detach().cpu().numpy() if dev.is_tensor(a) else np.asarray(a)


class BinnedSelection:
    """The injection set of a :class:`~isochrones_amd.hierarchical.PopulationPosterior` with a binned model: compressed once,
    where the chain lies (``device``: a torch device, or None for a host chain), to the table of one star of J samples -
    x [Q][J] is a parameter-major storage of one step, ``extra`` the injections' ``lnd``, the interim records their draw
    records.  ``chunk``: None compresses the set as one ensemble; a number (by default, beyond 65 536 injections, 4 096) cuts
    it into ensembles of that many injections and a ragged remainder in a second call, whose tables are combined on the
    host in float64 in ascending order, rescaled to the largest ``mx``.  ``alpha(theta)`` is ``ell`` and ``ess`` of ``iso_binned_lnlike`` on that table with M = J."""

    #: ``chunk="auto"``: one ensemble up to AUTO_ABOVE injections, ensembles of AUTO_CHUNK beyond (one workgroup walks an
    #: ensemble's samples tile by tile, so a large set as one ensemble leaves the rest of the device idle)
    AUTO_ABOVE, AUTO_CHUNK = 65536, 4096

    def __init__(self, injections, model, device, chunk="auto"):
        from .selection import InjectionSet
        if not isinstance(injections, InjectionSet):
            raise TypeError("injections must be an InjectionSet (got %r)" % (injections,))
        for col in model.columns:
            if col not in injections.columns or col not in injections.records:
                raise ValueError("the injection set has no column %r with a draw prior (it has %s)"
                                 % (col, ", ".join(sorted(injections.records)) or "none"))
        self.model, self.device, self.J, self.Q = model, device, injections.J, len(model.columns)
        if self.J > np.iinfo(np.int32).max:
            raise ValueError("an injection set of more than 2^31 - 1 injections")
        self.grid = grid = model.bin_grid()
        x = np.ascontiguousarray(np.stack([_host(injections.columns[c]) for c in model.columns]), dtype=np.float64)
        lnd = np.ascontiguousarray(_host(injections.lnd), dtype=np.float64)
        draw = np.concatenate([injections.records[c] for c in model.columns])
        edges = np.ascontiguousarray(np.concatenate(grid["edges"]), dtype=np.float64)
        frozen = grid["frozen"]
        if device is not None:
            import torch
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            x, lnd, edges = up(x), up(lnd), up(edges)
            draw, frozen = up(draw.view(np.uint8).copy()), up(frozen.view(np.uint8).copy())
        self.x, self.lnd = x, lnd
        J = self.J
        if isinstance(chunk, str):
            chunk = None if J <= self.AUTO_ABOVE else self.AUTO_CHUNK
        self._buffers = (draw, frozen, edges)
        if chunk is None or int(chunk) >= J:
            parts = [(0, 1, J)]
        else:
            chunk = int(chunk)
            if chunk < 1:
                raise ValueError("chunk must be at least 1")
            n_full = J // chunk
            parts = [(0, n_full, chunk)] + ([(n_full * chunk, 1, J - n_full * chunk)] if J % chunk else [])
        tables = [self._compress(first, n, W, draw, frozen, edges) for first, n, W in parts]
        A, A2, mx = (np.concatenate([t[k] for t in tables], axis=-1) for k in range(3))
        self.n_bad, self.n_out = (int(sum(t[k].sum() for t in tables)) for k in (3, 4))
        # one star: the chunks in ascending order, rescaled to the largest mx
        top = mx.max()
        B = grid["n_cells"]
        tA, tA2 = np.zeros((B, 1)), np.zeros((B, 1))
        if top > -np.inf:
            for c in range(mx.size):
                f = np.exp(mx[c] - top)
                tA[:, 0] += A[:, c] * f
                tA2[:, 0] += A2[:, c] * (f * f)
        tmx = np.array([top])
        if device is not None:
            import torch
            tA, tA2, tmx = (torch.from_numpy(a).to(device) for a in (tA, tA2, tmx))
        self.tables = (tA, tA2, tmx)

    def _compress(self, first, n, W, draw, frozen, edges):
        """The tables (numpy) of the ``n`` ensembles of ``W`` injections that start at injection ``first``."""
        grid, Q, J, B = self.grid, self.Q, self.J, self.grid["n_cells"]
        i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
        base = _ptr(self.x).value + 8 * first
        cols = (bc.IsoHierColumn * Q)(*[bc.IsoHierColumn(base + 8 * q * J, 1, 0, n, 0) for q in range(Q)])
        extra = C.c_void_p(_ptr(self.lnd).value + 8 * first)
        lib = bc.lib()
        if self.device is None:
            A, A2, mx = np.empty((B, n)), np.empty((B, n)), np.empty(n)
            n_bad, n_out = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
            fn, stream = lib.iso_binned_compress_host, None
        else:
            import torch
            f64 = dict(dtype=torch.float64, device=self.device)
            A, A2, mx = torch.empty(B, n, **f64), torch.empty(B, n, **f64), torch.empty(n, **f64)
            n_bad = torch.empty(n, dtype=torch.int32, device=self.device)
            n_out = torch.empty(n, dtype=torch.int32, device=self.device)
            fn, stream = lib.iso_binned_compress, dev.stream_ptr(self.device.index)
        bc.check(fn(cols, Q, _cabi.CHAIN_PARAM_MAJOR, 1, n, W, 0, n, _ptr(draw), _ptr(frozen), len(grid["frozen_cols"]),
                    i32(grid["frozen_cols"]), len(grid["axes"]), i32(grid["axes"]), i32([len(e) - 1 for e in grid["edges"]]),
                    _ptr(edges), extra, None, _ptr(A), _ptr(A2), _ptr(mx), _ptr(n_bad), _ptr(n_out), stream))
        return tuple(_host(a) for a in (A, A2, mx, n_bad, n_out))

    def alpha(self, theta):
        """``(ln_alpha [H], n_eff [H], n_bad)`` of the rows ``theta`` [H, P] where the injections lie: numpy arrays for a
        host set, CUDA tensors otherwise."""
        lnh = self.model.cell_table(np.atleast_2d(theta))["lnh"]
        H, B = lnh.shape
        A, A2, mx = self.tables
        lib = bc.lib()
        if self.device is None:
            la, ne = np.empty((H, 1)), np.empty((H, 1))
            fn, stream, nb = lib.iso_binned_lnlike_host, None, np.array([self.n_bad], dtype=np.int32)
        else:
            import torch
            f64 = dict(dtype=torch.float64, device=self.device)
            la, ne = torch.empty(H, 1, **f64), torch.empty(H, 1, **f64)
            lnh = torch.from_numpy(lnh).to(self.device)
            nb = torch.tensor([self.n_bad], dtype=torch.int32, device=self.device)
            fn, stream = lib.iso_binned_lnlike, dev.stream_ptr(self.device.index)
        bc.check(fn(_ptr(A), _ptr(A2), _ptr(mx), B, 1, 0, 1, self.J, _ptr(lnh), H, None, _ptr(la), _ptr(ne), None, None, stream))
        return la.reshape(H), ne.reshape(H), nb
