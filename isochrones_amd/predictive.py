"""Posterior-predictive check along a stored ensemble chain: at every sample the model's magnitudes (through the
bolometric-correction grid), Teff, logg, [Fe/H] and parallax, compared with the star's own measurements by the HIP kernel of
libiso_predict.so (``iso_predict_chain``; the definition is in include/isochrones_amd_predict.h).  Per ensemble: the mean
chi-square of every term, their mean over the terms (the reference's ``StarModel.posterior_predictive``), the sample of
largest log-probability (``map_pars``) and the system-magnitude chain in the sampler's parameter-major layout, which the
quantile kernel summarises where it lies."""
from __future__ import annotations

import ctypes as C

import numpy as np

import functools

from . import _cabi, _chain, _predict_cabi, _tables, derived as dv, device as dev

#: the terms after the bands, in the kernel's order
SPEC_TERMS = ("Teff", "logg", "feh", "parallax")
#: device memory one slice of a magnitude chain may take in ``FusedEnsembleSampler.predictive``
PREDICT_BUDGET_BYTES = 2 << 30


class PredictiveResult:
    """What one ``iso_predict_chain`` call returns, CUDA tensors: ``mags`` [nsteps, B, n_ens_out * W] (parameter-major
    storage; None when not asked for), ``term_chi2`` [n_ens_out, B + 4], ``ppc`` [n_ens_out], ``n_bad`` [n_ens_out] int32,
    ``mag_nan`` [n_ens_out, B] int32 (NaN magnitudes per band), ``map_index`` [n_ens_out] int64 and ``map_pars``
    [n_ens_out, ndim] (both None without ``lnprob``), and ``bands``."""

    def __init__(self, bands, mags, term_chi2, ppc, n_bad, map_index, map_pars, mag_nan=None):
        self.bands = tuple(bands)
        self.mags, self.term_chi2, self.ppc, self.n_bad, self.mag_nan = mags, term_chi2, ppc, n_bad, mag_nan
        self.map_index, self.map_pars = map_index, map_pars

    @property
    def terms(self):
        return self.bands + SPEC_TERMS


def term_names(bands):
    """The B + 4 terms in the kernel's order: the bands, then Teff, logg, feh, parallax."""
    return tuple(bands) + SPEC_TERMS


def result_labels(bands, param_names):
    """The columns ``predictive`` adds to a catalog result row, in order."""
    cols = ["ppc", "ppc_nbad"]
    for b in bands:
        cols += ["%s_mag_%s" % (b, s) for s in ("median", "p16", "p84")]
    cols += ["chi2_%s" % t for t in term_names(bands)]
    cols += ["map_%s" % p for p in param_names]
    return cols


def pack_obs(obs, bands, n_ens):
    """``obs`` -> (obs_val, obs_unc), float64 numpy ``[n_ens, B + 4]``.  ``obs`` is that pair itself, or the dict
    ``CatalogPosterior.build_columns`` makes (``mag_val``, ``mag_unc``, ``spec_val``, ``spec_unc``, ``has_plx``, ``plx_val``,
    ``plx_unc``), or a dict ``{term: (value, uncertainty)}`` of one star (a :class:`BasicStarModel`'s ``kwargs``), repeated
    for every ensemble.  A NaN value is an absent term."""
    B = len(bands)
    if isinstance(obs, DeviceObs):
        if obs.shape != (n_ens, B + 4):
            raise ValueError("observations on the device are [n_ens, B + 4] = %s, got %s" % ((n_ens, B + 4), obs.shape))
        return obs
    if isinstance(obs, dict) and "mag_val" in obs:
        val = np.full((n_ens, B + 4), np.nan)
        unc = np.full((n_ens, B + 4), np.nan)
        val[:, :B], unc[:, :B] = obs["mag_val"], obs["mag_unc"]
        val[:, B:B + 3], unc[:, B:B + 3] = obs["spec_val"], obs["spec_unc"]
        has = np.asarray(obs["has_plx"]).astype(bool)
        val[:, B + 3] = np.where(has, obs["plx_val"], np.nan)
        unc[:, B + 3] = np.where(has, obs["plx_unc"], np.nan)
    elif isinstance(obs, dict):
        val = np.full((n_ens, B + 4), np.nan)
        unc = np.full((n_ens, B + 4), np.nan)
        for j, t in enumerate(term_names(bands)):
            if t in obs and obs[t] is not None:
                val[:, j], unc[:, j] = float(obs[t][0]), float(obs[t][1])
    else:
        val, unc = (np.array(a, dtype=np.float64, ndmin=2) for a in obs)
    val = np.ascontiguousarray(val, dtype=np.float64)
    unc = np.ascontiguousarray(unc, dtype=np.float64)
    if val.shape != (n_ens, B + 4) or unc.shape != (n_ens, B + 4):
        raise ValueError("observations are [n_ens, B + 4] = %s values and uncertainties (bands, then Teff, logg, feh, "
                         "parallax), got %s and %s" % ((n_ens, B + 4), val.shape, unc.shape))
    return val, unc


class DeviceObs:
    """Packed observations already on a device (``val``, ``unc``: float64 CUDA tensors ``[n_ens, B + 4]``): what
    :func:`predict_storage` takes as ``obs`` to skip the packing and the upload, e.g. once for all slices of a chain."""

    def __init__(self, val, unc, device):
        self.val, self.unc = dev.to_device_f64(val, device), dev.to_device_f64(unc, device)
        self.shape = tuple(self.val.shape)


class PredictTables:
    """(Teff, logg, feh, Mbol) of the model grid packed ``[n0, n1, nk, 4]`` and the ``bands`` columns of the BC grid packed
    ``[nT, ng, nf, nA, B]`` on a device, with their axes and the two structs that point at them."""

    def __init__(self, ic, bands, device):
        put = functools.partial(dev.to_device_f64, device=device)
        self.cols, self.axes, shape = _tables.pack_model(ic.model_grid.interp, ic._cols, put)
        self.bc, self.bc_axes, bshape = _tables.pack_bc(ic, bands, put)
        self.B = bshape[4]
        self.model = _tables.fill(_predict_cabi.IsoPredictModelTable, self.cols, self.axes, shape[:3], 0)
        self.bct = _tables.fill(_predict_cabi.IsoPredictBcTable, self.bc, self.bc_axes, bshape, 0)


def predict_tables(ic, bands, device):
    """The packed tables, made once per (interpolator, device, bands) and remade when the model or the BC table was rebuilt
    (``_chain.cached_by_generation``); ``ic.release()`` drops them."""
    gen = (ic.model_grid.interp._handles.generation, ic.bc_grid.interp._handles.generation)
    return _chain.cached_by_generation(ic, "_predict_tables", (device, tuple(bands)), gen,
                                       lambda: PredictTables(ic, bands, device))


def predict_storage(storage, lnprob, n_ens, nwalkers, ic, bands, obs, N=1, layout=_cabi.CHAIN_PARAM_MAJOR, ens_begin=0,
                    n_ens_out=None, want_mags=True):
    """The posterior-predictive check of the ensembles ``[ens_begin, ens_begin + n_ens_out)`` of a stored chain.
    ``storage``: a contiguous float64 CUDA tensor ``[nsteps, ndim, n_ens * nwalkers]`` (parameter-major, the sampler's) or
    ``[nsteps, n_ens * nwalkers, ndim]`` (``layout=_cabi.CHAIN_ROW_MAJOR``); ``lnprob``: ``[nsteps, n_ens * nwalkers]`` or
    None (then no MAP); ``obs``: see :func:`pack_obs`, rows indexed by the ensemble.  Returns a :class:`PredictiveResult` on
    the current stream, without a synchronise.  One ``iso_predict_chain`` launch."""
    import torch
    bands = _tables.check_bands(ic, bands, _predict_cabi.MAX_BANDS)
    comps = dv.components(ic, N)
    n_ens, W = int(n_ens), int(nwalkers)
    x, nsteps, ndim = _chain.check_storage(storage, n_ens, W, layout, "the posterior-predictive check takes")
    if ndim < len(dv.fit_param_names(ic, N)):
        raise ValueError("the chain has %d parameters, a fit on this grid samples %d" % (ndim, len(dv.fit_param_names(ic, N))))
    if lnprob is not None:
        if not (dev.is_tensor(lnprob) and lnprob.is_cuda and lnprob.dtype == torch.float64):
            raise ValueError("lnprob is a float64 CUDA tensor")
        if tuple(lnprob.shape) != (nsteps, n_ens * W):
            raise ValueError("lnprob is [nsteps, n_ens * nwalkers]")
    n_out = n_ens - int(ens_begin) if n_ens_out is None else int(n_ens_out)
    if int(ens_begin) < 0 or n_out < 1 or int(ens_begin) + n_out > n_ens:
        raise ValueError("ensemble range [ens_begin, ens_begin + n_ens_out) must be non-empty and inside [0, n_ens)")
    packed = pack_obs(obs, bands, n_ens)
    lp = None if lnprob is None else lnprob.contiguous()
    device = x.device.index
    B, R = len(bands), n_out * W
    f64 = dict(dtype=torch.float64, device=x.device)
    mags = torch.empty(nsteps, B, R, **f64) if want_mags else None
    term = torch.empty(n_out, B + 4, **f64)
    ppc = torch.empty(n_out, **f64)
    n_bad = torch.empty(n_out, dtype=torch.int32, device=x.device)
    mi = torch.empty(n_out, dtype=torch.int64, device=x.device) if lp is not None else None
    mp = torch.empty(n_out, ndim, **f64) if lp is not None else None
    dobs = packed if isinstance(packed, DeviceObs) else DeviceObs(packed[0], packed[1], device)
    dval, dunc = dobs.val, dobs.unc
    mag_nan = torch.empty(n_out, B, dtype=torch.int32, device=x.device)
    out = _predict_cabi.IsoPredictOut(dev.ptr(mags), dev.ptr(term), dev.ptr(ppc), dev.ptr(n_bad), dev.ptr(mi), dev.ptr(mp),
                                      dev.ptr(mag_nan))
    carr = (C.c_int32 * (3 * len(comps)))(*[i for comp in comps for i in comp])
    tb = predict_tables(ic, bands, device)
    Nn = len(comps)
    with torch.cuda.device(x.device):
        _predict_cabi.check(_predict_cabi.lib().iso_predict_chain(
            C.byref(tb.model), C.byref(tb.bct), dev.ptr(x), dev.ptr(lp), int(layout), nsteps, n_ens, W, ndim, int(ens_begin),
            n_out, carr, Nn, Nn + 2, Nn + 3, dev.ptr(dval), dev.ptr(dunc), C.byref(out), dev.stream_ptr(device)))
    res = PredictiveResult(bands, mags, term, ppc, n_bad, mi, mp, mag_nan)
    res._keep = (dval, dunc)            # the observation buffers live until the stream has run the launch
    return res


def chain_predictive(chain, lnprob, ic, bands, obs, N=1):
    """The same for the ``[S, W, T, D]`` (or ``[W, T, D]``) view ``sampler.chain`` returns and the ``[S, W, T]`` (``[W, T]``)
    view ``sampler.lnprobability`` returns (or None).  The result's ``mags`` is a ``[S, W, T, B]`` (``[W, T, B]``) view and the
    per-ensemble outputs lose the leading axis for a single ensemble."""
    import torch
    if not dev.is_tensor(chain) or chain.dtype != torch.float64 or not chain.is_cuda:
        raise ValueError("chain_predictive takes a float64 CUDA tensor")
    storage, S, W, single = _chain.as_storage(chain)
    nsteps, lp = int(storage.shape[0]), None
    if lnprob is not None:
        lnprob = lnprob[None] if single else lnprob
        if not dev.is_tensor(lnprob) or tuple(lnprob.shape) != (S, W, nsteps):
            raise ValueError("lnprob must be [S, W, T] (or [W, T])")
        lp = lnprob.permute(2, 0, 1).contiguous().reshape(nsteps, S * W)
    r = predict_storage(storage, lp, S, W, ic, bands, obs, N=N)
    r.mags = _chain.from_storage(r.mags, S, W, single)
    if single:
        r.term_chi2, r.ppc, r.n_bad, r.mag_nan = r.term_chi2[0], r.ppc[0], r.n_bad[0], r.mag_nan[0]
        if r.map_index is not None:
            r.map_index, r.map_pars = r.map_index[0], r.map_pars[0]
    return r
