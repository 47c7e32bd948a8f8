"""Derived stellar properties along a stored ensemble chain: model-grid columns (mass, radius, Teff, logg, age ...)
interpolated at every sample by the HIP kernel of libiso_derived.so (``iso_derived_chain``; the definition is in
include/isochrones_amd_derived.h).  The result is a chain of its own in the sampler's parameter-major layout, so the
quantile kernel summarises it where it lies.

Model-grid columns only: band magnitudes go through the bolometric-correction grid and are served by
:mod:`isochrones_amd.predictive` (libiso_predict.so)."""
from __future__ import annotations

import ctypes as C

import functools

from . import _cabi, _chain, _derived_cabi, _tables, device as dev

#: what ``derived=True`` asks for in a catalog fit, as far as the model grid has the column and the fit does not sample it
DEFAULT_PROPS = ("mass", "radius", "age", "Teff", "logg")
#: device memory one slice of a derived chain may take in ``FusedEnsembleSampler.derived_quantiles``
DERIVED_BUDGET_BYTES = 2 << 30


def fit_param_names(ic, N=1):
    """The parameters a fit on ``ic`` samples (the names of ``StarModel.param_names``)."""
    base = tuple(ic.param_names)
    return base if N == 1 else tuple(["eep_%d" % i for i in range(N)] + list(base[1:]))


def components(ic, N=1):
    """Per star of the system the chain parameters that give its coordinates on the model grid's axes, ``[(p0, p1, pk)]``:
    the first three of ``ic.param_index_order`` for a single star; an N-star system on an isochrone grid samples
    (eep_0 .. eep_{N-1}, age, feh, ...)."""
    N = int(N)
    if not 1 <= N <= _derived_cabi.MAX_COMPS:
        raise ValueError("N must be 1 to %d" % _derived_cabi.MAX_COMPS)
    if N == 1:
        return [tuple(int(i) for i in ic.param_index_order[:3])]
    if ic.eep_replaces != "mass":
        raise ValueError("a multiple system (N > 1) is sampled on an isochrone grid")
    return [(N, N + 1, k) for k in range(N)]


def resolve_props(ic, props, N=1):
    """``props`` -> (labels, columns): an item is a model-grid column name or a ``(label, column)`` pair.  A label that is
    one of the fit's parameter names is refused (on a track grid the parameter ``mass`` is the initial mass, the grid column
    ``mass`` the current one: two different numbers under one name), and so is a column the grid lacks."""
    if isinstance(props, str):
        props = (props,)
    names = fit_param_names(ic, N)
    have = ic.model_grid.interp.column_index
    labels, cols = [], []
    for item in props:
        label, col = (item, item) if isinstance(item, str) else tuple(item)
        if col not in have:
            raise ValueError("the model grid has no column %r (it has %s)" % (col, ", ".join(ic.model_grid.interp.columns)))
        if label in names or label in ic.param_names:
            raise ValueError("%r is a parameter of the fit; the grid column %r is another quantity - pass (label, column), "
                             "e.g. (%r, %r)" % (label, col, label + "_now", col))
        if label in labels:
            raise ValueError("label %r given twice" % (label,))
        labels.append(label)
        cols.append(col)
    if not cols:
        raise ValueError("no derived property asked for")
    return tuple(labels), tuple(cols)


def default_props(ic, N=1):
    """``derived=True``: those of ``DEFAULT_PROPS`` that are model-grid columns and not parameters of the fit."""
    names = set(fit_param_names(ic, N)) | set(ic.param_names)
    have = ic.model_grid.interp.column_index
    return tuple(p for p in DEFAULT_PROPS if p in have and p not in names)


def expand_labels(labels, N=1):
    """Output column names in the kernel's order (component-major): the labels for N = 1, ``{label}_{k}`` for N > 1."""
    return tuple(labels) if N == 1 else tuple("%s_%d" % (l, k) for k in range(N) for l in labels)


class DerivedTable:
    """Up to 8 columns of a model grid packed ``[n0, n1, nk, Q]`` on a device with its axes, and the ``iso_derived_table``
    that points at them."""

    def __init__(self, interp, icols, device):
        self.device = device
        self.cols, self.axes, shape = _tables.pack_model(interp, icols, functools.partial(dev.to_device_f64, device=device))
        self.Q = shape[3]
        self.table = _tables.fill(_derived_cabi.IsoDerivedTable, self.cols, self.axes, shape)


def derived_tables(ic, columns, device):
    """The packed tables of ``columns`` (one per 8 columns), made once per (interpolator, device, column tuple) and remade
    when the model table was rebuilt (``_chain.cached_by_generation``); ``ic.release()`` drops them."""
    dfi, M = ic.model_grid.interp, _derived_cabi.MAX_COLS
    icols = [dfi.column_index[c] for c in columns]
    return _chain.cached_by_generation(ic, "_derived_tables", (device, tuple(columns)), dfi._handles.generation, lambda: [
        DerivedTable(dfi, icols[i:i + M], device) for i in range(0, len(icols), M)])


def derive_storage(storage, n_ens, nwalkers, ic, props, N=1, layout=_cabi.CHAIN_PARAM_MAJOR, ens_begin=0, n_ens_out=None):
    """``props`` along the ensembles ``[ens_begin, ens_begin + n_ens_out)`` of a stored chain: ``storage`` is a contiguous
    float64 CUDA tensor, ``[nsteps, ndim, n_ens * nwalkers]`` (parameter-major, the sampler's) or ``[nsteps, n_ens * nwalkers,
    ndim]`` (``layout=_cabi.CHAIN_ROW_MAJOR``).  Returns ``(derived_storage, nan_count)``: ``[nsteps, C * Q, n_ens_out *
    nwalkers]`` float64 with column ``c * Q + q`` (see :func:`expand_labels`) and ``[n_ens_out, C * Q]`` int32, both CUDA
    tensors, on the current stream, without a synchronise.  One launch per 8 columns."""
    import torch
    labels, cols = resolve_props(ic, props, N)
    comps = components(ic, N)
    n_ens, W = int(n_ens), int(nwalkers)
    x, nsteps, ndim = _chain.check_storage(storage, n_ens, W, layout, "derived properties take")
    if ndim < len(fit_param_names(ic, N)):
        raise ValueError("the chain has %d parameters, a fit on this grid samples %d" % (ndim, len(fit_param_names(ic, N))))
    n_out = n_ens - int(ens_begin) if n_ens_out is None else int(n_ens_out)     # (the range is the C call's to check)
    device = x.device.index
    Cn, Qt, R = len(comps), len(cols), n_out * W
    out = torch.empty(nsteps, Cn * Qt, max(R, 0), dtype=torch.float64, device=x.device)
    nan_count = torch.empty(max(n_out, 0), Cn * Qt, dtype=torch.int32, device=x.device)
    carr = (C.c_int32 * (3 * Cn))(*[i for comp in comps for i in comp])
    lib = _derived_cabi.lib()
    tables = derived_tables(ic, cols, device)
    with torch.cuda.device(x.device):
        q0 = 0
        for tb in tables:
            whole = len(tables) == 1
            o = out if whole else torch.empty(nsteps, Cn * tb.Q, R, dtype=torch.float64, device=x.device)
            nc = nan_count if whole else torch.empty(n_out, Cn * tb.Q, dtype=torch.int32, device=x.device)
            _derived_cabi.check(lib.iso_derived_chain(C.byref(tb.table), dev.ptr(x), int(layout), nsteps, n_ens, W, ndim,
                                                      int(ens_begin), n_out, carr, Cn, dev.ptr(o), dev.ptr(nc),
                                                      dev.stream_ptr(device)))
            if not whole:       # more than 8 columns: each launch's block of columns goes to its place inside every component
                out.view(nsteps, Cn, Qt, R)[:, :, q0:q0 + tb.Q] = o.view(nsteps, Cn, tb.Q, R)
                nan_count.view(n_out, Cn, Qt)[:, :, q0:q0 + tb.Q] = nc.view(n_out, Cn, tb.Q)
            q0 += tb.Q
    return out, nan_count


def chain_derived(chain, ic, props, N=1, n_ens=None, nwalkers=None):
    """Model-grid columns ``props`` of ``ic`` at every sample of ``chain``: the ``[S, W, T, D]`` (or ``[W, T, D]``) view
    ``sampler.chain`` returns - passed on without a copy when it is a view of parameter-major storage, as the sampler's is -
    or, with ``n_ens`` and ``nwalkers`` given, the parameter-major storage ``[T, D, n_ens * nwalkers]`` itself.  Returns
    ``(derived, names)``: a ``[S, W, T, C * Q]`` (``[W, T, C * Q]``) CUDA view of the derived storage and the column names
    (``{label}_{k}`` for N > 1).  ``props`` items are a column name or a ``(label, column)`` pair.  NaN where the sample lies
    off the grid or next to its NaN padding."""
    import torch
    if not dev.is_tensor(chain) or chain.dtype != torch.float64 or not chain.is_cuda:
        raise ValueError("chain_derived takes a float64 CUDA tensor")
    storage, n_ens, nwalkers, single = _chain.as_storage(chain, n_ens, nwalkers)
    labels, _ = resolve_props(ic, props, N)
    out, _ = derive_storage(storage, n_ens, nwalkers, ic, props, N)
    return _chain.from_storage(out, n_ens, nwalkers, single), expand_labels(labels, N)
