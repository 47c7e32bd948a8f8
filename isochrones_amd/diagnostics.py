"""Convergence diagnostics of a stored ensemble chain, per (ensemble, parameter) pair: integrated autocorrelation time
with Sokal's window, effective sample size and split R-hat (the definition is in include/isochrones_amd_diag.h).

A CUDA tensor goes through the HIP kernel of libiso_diag.so (``iso_diag_chain``: one workgroup per pair, on the current
stream, no host round trip); a host numpy array goes through the library's plain C++ statement of the same definition
(``iso_diag_chain_host``), which needs no GPU."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _cabi, _chain, _diag_cabi

ChainDiagnostics = namedtuple("ChainDiagnostics", ["tau", "window", "window_ok", "ess", "rhat"])
ChainDiagnostics.__doc__ = """Per-pair diagnostics, each [S, D] (or [D] for a single ensemble): ``tau`` integrated
autocorrelation time in steps, ``window`` Sokal's window M*, ``window_ok`` 1 where a window was found inside the lags
looked at (0: ``tau`` is a lower bound from a chain too short to tell), ``ess`` = W T / tau, ``rhat`` split R-hat."""


def _check(c, max_lag):
    c, max_lag = float(c), int(max_lag)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("c must be finite and > 0")
    if max_lag < 1:
        raise ValueError("max_lag must be at least 1")
    return c, max_lag


def diag_storage(storage, n_ens, nwalkers, c=_diag_cabi.DEFAULT_C, max_lag=_diag_cabi.DEFAULT_MAX_LAG):
    """The raw [S, D, 5] result (``_diag_cabi.TAU`` .. ``RHAT`` order) for parameter-major storage
    ``[nsteps, ndim, n_ens * nwalkers]``: a contiguous float64 CUDA tensor (result: CUDA tensor, asynchronous) or a host
    numpy array (result: numpy array)."""
    import ctypes as C
    c, max_lag = _check(c, max_lag)
    n_ens, nwalkers = int(n_ens), int(nwalkers)
    x, nsteps, ndim = _chain.check_storage(storage, n_ens, nwalkers, _cabi.CHAIN_PARAM_MAJOR, "chain_diagnostics takes",
                                           host=True)
    lib = _diag_cabi.lib()
    if isinstance(x, np.ndarray):
        out = np.empty((n_ens, ndim, _diag_cabi.NOUT))
        _diag_cabi.check(lib.iso_diag_chain_host(x.ctypes.data_as(C.c_void_p), _cabi.CHAIN_PARAM_MAJOR, nsteps, n_ens, nwalkers,
                                                 ndim, c, max_lag, out.ctypes.data_as(C.c_void_p), None))
        return out
    import torch
    from . import device as dev
    out = torch.empty(n_ens, ndim, _diag_cabi.NOUT, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _diag_cabi.check(lib.iso_diag_chain(dev.ptr(x), _cabi.CHAIN_PARAM_MAJOR, nsteps, n_ens, nwalkers, ndim, c, max_lag,
                                            dev.ptr(out), dev.stream_ptr(x.device.index)))
    return out


def chain_diagnostics(chain, c=_diag_cabi.DEFAULT_C, max_lag=_diag_cabi.DEFAULT_MAX_LAG, n_ens=None, nwalkers=None):
    """Diagnostics of ``chain``: the ``[S, W, T, D]`` (or ``[W, T, D]``) view ``sampler.chain`` returns - passed on without
    a copy when it is a view of parameter-major storage, as the sampler's is - or, with ``n_ens`` and ``nwalkers`` given,
    the parameter-major storage ``[T, D, n_ens * nwalkers]`` itself.  ``c`` is Sokal's window factor, ``max_lag`` the largest
    lag summed.  Returns a :class:`ChainDiagnostics` of ``[S, D]`` (``[D]`` for a ``[W, T, D]`` chain) arrays of the
    input's kind."""
    storage, n_ens, nwalkers, single = _chain.as_storage(chain, n_ens, nwalkers)
    out = diag_storage(storage, n_ens, nwalkers, c, max_lag)
    if single:
        out = out[0]
    return ChainDiagnostics(*(out[..., i] for i in range(_diag_cabi.NOUT)))
