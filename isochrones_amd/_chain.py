"""The stored ensemble chain as what post-processes it sees it (:mod:`diagnostics`, :mod:`derived`, :mod:`predictive`, the
sampler's summaries of them): the ``[S, W, T, D]`` view <-> the parameter-major storage ``[T, D, S * W]``, the checks on a
storage tensor, the one call of the quantile kernel, a summary sliced by a memory budget, per-device tables that follow a
grid's generation.  A further post-processing library puts ``as_storage`` / ``check_storage`` in front of its C call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi, device as dev


def as_storage(chain, n_ens=None, nwalkers=None):
    """``(storage, n_ens, W, single)`` of the ``[S, W, T, D]`` (or ``[W, T, D]``: ``single``) view ``sampler.chain`` returns -
    passed on without a copy when it is a view of parameter-major storage, as the sampler's is - or, with ``n_ens`` and
    ``nwalkers``, of the storage ``[T, D, n_ens * nwalkers]`` itself.  A torch tensor or a host numpy array, and so is the storage."""
    if (n_ens is None) != (nwalkers is None):
        raise ValueError("give both n_ens and nwalkers (parameter-major storage) or neither (a [S, W, T, D] chain)")
    if nwalkers is not None:
        return chain, int(n_ens), int(nwalkers), False
    single = len(chain.shape) == 3
    chain = chain[None] if single else chain
    if len(chain.shape) != 4:
        raise ValueError("chain must be [S, W, T, D] or [W, T, D]")
    S, W = int(chain.shape[0]), int(chain.shape[1])
    t = chain.swapaxes(0, 2).swapaxes(1, 3)                                     # [T, D, S, W]
    t = np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t.contiguous()
    return t.reshape(t.shape[0], t.shape[1], S * W), S, W, single


def from_storage(out, n_ens, W, single):
    """The ``[S, W, T, C]`` (``single``: ``[W, T, C]``) view of parameter-major storage ``[T, C, n_ens * W]``."""
    view = out.reshape(out.shape[0], out.shape[1], int(n_ens), int(W)).swapaxes(0, 2).swapaxes(1, 3)
    return view[0] if single else view


def check_storage(storage, n_ens, W, layout, what, host=False):
    """``(contiguous storage, nsteps, ndim)`` of a stored chain of ``n_ens * W`` rows in ``layout``: a float64 CUDA tensor
    or, with ``host``, a host numpy array.  ``what`` starts the message about the wrong kind ("derived properties take")."""
    is_host = host and isinstance(storage, np.ndarray)
    if not is_host:
        import torch
        if not (dev.is_tensor(storage) and storage.is_cuda and storage.dtype == torch.float64):
            raise ValueError("%s a float64 CUDA tensor%s" % (what, " or a host numpy array" if host else ""))
    rows_axis = 2 if layout == _cabi.CHAIN_PARAM_MAJOR else 1
    if len(storage.shape) != 3 or storage.shape[rows_axis] != int(n_ens) * int(W):
        raise ValueError("parameter-major storage is [nsteps, ndim, n_ens * nwalkers]" if rows_axis == 2 else
                         "row-major storage is [nsteps, n_ens * nwalkers, ndim]")
    nsteps, ndim = int(storage.shape[0]), int(storage.shape[3 - rows_axis])
    if nsteps < 1:
        raise ValueError("no stored chain")
    return (np.ascontiguousarray(storage, dtype=np.float64) if is_host else storage.contiguous()), nsteps, ndim


def quantiles_layout(device_index, storage, nsteps, n_ens, W, ncols, q, out):
    """``iso_chain_quantiles_layout`` on contiguous parameter-major storage ``[nsteps, ncols, n_ens * W]``: the quantiles ``q``
    (float64 numpy, at most 8) of every (ensemble, column) into ``out`` ``[n_ens, ncols, len(q)]``, on the current stream."""
    _cabi.check(_cabi.lib().iso_chain_quantiles_layout(dev.context(device_index), dev.ptr(storage), _cabi.CHAIN_PARAM_MAJOR,
                                                       int(nsteps), int(n_ens), int(W), int(ncols),
                                                       q.ctypes.data_as(C.POINTER(C.c_double)), q.size, dev.ptr(out),
                                                       dev.stream_ptr(device_index)))


def sliced_quantiles(device_index, nsteps, S, W, ncols, q, budget, make, who, too_big):
    """Quantiles ``[S, ncols, len(q)]`` and NaN counts ``[S, ncols]`` (int32) of a chain made for the purpose, in slices of
    whole ensembles of at most ``budget`` bytes: ``make(s0, n)`` -> (parameter-major storage ``[nsteps, ncols, n * W]``, NaN
    counts ``[n, ncols]``) of the ensembles ``[s0, s0 + n)``, summarised where it lies.  A column of an ensemble with a NaN
    sample has NaN quantiles.  ``who`` refuses more than 8 levels ``q``; ``too_big``: the message (two ``%d``: one ensemble's
    bytes, the budget) when not one ensemble fits."""
    import torch
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.size < 1 or q.size > 8:
        raise ValueError("%s takes 1 to 8 quantile levels per call (the quantile kernel's limit)" % who)
    step = budget // (nsteps * ncols * W * 8)
    if step < 1:
        raise ValueError(too_big % (nsteps * ncols * W * 8, budget))
    device = torch.device("cuda", device_index)
    out = torch.empty(S, ncols, q.size, dtype=torch.float64, device=device)
    counts = torch.empty(S, ncols, dtype=torch.int32, device=device)
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        storage, counts[s0:s0 + n] = make(s0, n)
        quantiles_layout(device_index, storage, nsteps, n, W, ncols, q, out[s0:s0 + n])
    return torch.where((counts > 0)[:, :, None], torch.full_like(out, float("nan")), out), counts


def cached_by_generation(owner, slot, key, generation, make):
    """``make()`` once per ``key`` in ``owner.__dict__[slot]`` and again when ``generation`` (of the table it was made from)
    has changed; ``ModelGridInterpolator.release()`` drops the slots."""
    cache = owner.__dict__.setdefault(slot, {})
    entry = cache.get(key)
    if entry is None or entry[0] != generation:
        entry = cache[key] = (generation, make())
    return entry[1]
