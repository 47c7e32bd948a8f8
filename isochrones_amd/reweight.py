"""Population-informed posteriors of the individual stars: the other half of Hogg, Myers & Bovy (2010).  Once
:class:`~isochrones_amd.hierarchical.PopulationPosterior` has fitted the population, every star's stored samples are
reweighted from the prior its fit used to that population ("shrinkage"),

    u[s][m] = sum_h  prod_q f_q(x_q[s][m]; theta_h) / f0_q(x_q[s][m])  /  Z_s(theta_h),        ln Z_s = ell[h][s],

over rows ``theta_h`` taken as equally weighted draws of the hyper posterior, and the star's age, mass, [Fe/H] ... are
summarised under those weights: weighted mean, standard deviation and quantiles (the inverted weighted distribution
function), the weights' effective sample size.  The HIP kernels of libiso_reweight.so do both on the stored chain where it
lies (``iso_reweight_stars``; the definition is in include/isochrones_amd_reweight.h); ``ell`` is what ``iso_hier_lnlike``
returns for the same rows.  The selection term does not enter: a star in the catalog was detected whatever the population.

Under a binned model (a :class:`~isochrones_amd.binned.Histogram`) the sum over the rows depends on the star and the sample's
cell alone, ``u = exp(c_m - mx) * G[s][cell]``: libiso_shrink.so takes ``G`` once per (star, cell) from the per-star tables
(``iso_shrink_cells``, which also gives the posterior probability of the star lying in each cell), then the weights of a
slice of stars once (``iso_shrink_weights``), and ``iso_reweight_summary`` summarises the value columns under them, eight at
a time (include/isochrones_amd_shrink.h).

:meth:`PopulationPosterior.star_posteriors`, :meth:`PopulationPosterior.star_weights` and
:meth:`PopulationPosterior.star_bin_probabilities` are the public calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi, _hier_cabi as hc, _reweight_cabi as rc, device as dev

#: rows of the hyper posterior a call takes when none are given
DEFAULT_ROWS = 64


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else dev.ptr(a)


def stat_names(q):
    """The suffixes of the quantile columns: the catalog's ``median``, ``p16``, ``p84`` for 0.5, 0.16, 0.84, ``q<100 p>``
    otherwise (``q2.5``)."""
    known = {0.5: "median", 0.16: "p16", 0.84: "p84"}
    return [known.get(float(p), "q%g" % (100.0 * float(p))) for p in q]


def default_theta(post):
    """At most :data:`DEFAULT_ROWS` rows spread evenly over the samples of ``post.fit_mcmc``."""
    if post._sampler is None:
        raise ValueError("theta=None takes rows of the fitted hyper posterior: run fit_mcmc first, or pass theta [H, P]")
    chain = post.sampler.flatchain
    chain = chain.detach().cpu().numpy() if dev.is_tensor(chain) else np.asarray(chain)
    n = chain.shape[0]
    pick = np.unique(np.round(np.linspace(0, n - 1, min(DEFAULT_ROWS, n))).astype(np.int64))
    return np.ascontiguousarray(chain[pick], dtype=np.float64)


def _theta(post, theta):
    if theta is None:
        return default_theta(post)
    th = theta.detach().cpu().numpy() if dev.is_tensor(theta) else np.asarray(theta, dtype=np.float64)
    return np.atleast_2d(th)


def value_columns(post, columns):
    """``(names, chain column or None per name, derived names)`` of the value columns ``columns`` (default: the chain's
    parameters, then the model's derived columns)."""
    names = list(post.chain_names) + list(post.derived_cols) if columns is None else \
        ([columns] if isinstance(columns, str) else list(columns))
    if not names:
        raise ValueError("no value column")
    have = post.ic.model_grid.interp.column_index if post.ic is not None else {}
    where, derived = [], []
    for col in names:
        if col in post.chain_names:
            where.append(post.chain_names.index(col))
        elif col in have:
            if post.host:
                raise ValueError("column %r is a model-grid column: it is derived on the device, so the chain must be a "
                                 "CUDA tensor" % (col,))
            where.append(None)
            if col not in derived:
                derived.append(col)
        else:
            raise ValueError("column %r is neither a parameter of the chain (%s) nor a column of the model grid"
                             % (col, ", ".join(post.chain_names)))
    return names, where, derived


def _slices(post, n_derived, stars=None):
    """The star slices ``(s0, n)`` under the posterior's ``budget_bytes``: a slice holds the model's derived chain, the
    derived value columns and the weights of its stars."""
    per_star = post.T * post.W * 8 * (len(post.derived_cols) + n_derived + 1)
    step = post.budget // per_star
    if step < 1:
        raise ValueError("the columns and weights of one star take %d bytes, more than budget_bytes = %d: raise the budget or "
                         "thin the chain" % (per_star, post.budget))
    lo, hi = (0, post.S) if stars is None else stars
    return [(s0, min(step, hi - s0)) for s0 in range(lo, hi, step)]


def _slice_columns(post, derived, s0, n):
    """``(the model's column descriptors, the storage of the derived value columns or None, its column names, the model's
    derived chain or None)`` for the stars [s0, s0 + n).  The descriptors hold addresses, not references: the caller keeps
    the last item alive while it uses them."""
    model_derived = post._derived(s0, n) if post.derived_cols else None
    cols = post._columns(model_derived, s0, n)
    value_derived, value_names = None, []
    if derived and all(c in post.derived_cols for c in derived):
        value_derived, value_names = model_derived, list(post.derived_cols)
    elif derived:
        from . import derived as dv
        value_derived, _ = dv.derive_storage(post.storage, post.S, post.W, post.ic, tuple(derived), ens_begin=s0, n_ens_out=n)
        value_names = derived
    return cols, value_derived, value_names, model_derived


def _value_group(post, names, where, value_derived, value_names, group, s0, n):
    """The descriptors of the value columns ``group`` (indices into ``names``) for the stars [s0, s0 + n)."""
    vals = (hc.IsoHierColumn * len(group))()
    for i, v in enumerate(group):
        if where[v] is not None:
            vals[i] = hc.IsoHierColumn(_ptr(post.storage).value, post.D, where[v], post.S, 0)
        else:
            vals[i] = hc.IsoHierColumn(_ptr(value_derived).value, len(value_names), value_names.index(names[v]), n, s0)
    return vals


def shrink_cells(post, theta):
    """``(cell table, lnG [B, S], cellp [B, S])`` of a binned model under the rows ``theta`` [H, P], where the chain lies:
    ``iso_shrink_cells`` on the per-star tables, the rows' log cell densities and their ``ell``."""
    from . import _shrink_cabi as sc
    table = post.model.cell_table(theta)
    lnh = table["lnh"]
    H, B = lnh.shape
    S = post.S
    A, _, mx, _, _ = post.bin_tables()
    ell = post._evaluate_binned(theta if post.host else _as_tensor(post, theta))[2]       # [H, S] where the chain lies
    lib = sc.lib()
    if post.host:
        lnG, cellp, ell, mask = np.empty((B, S)), np.empty((B, S)), np.ascontiguousarray(ell), post.mask
        fn, stream = lib.iso_shrink_cells_host, None
    else:
        import torch
        device = post.storage.device
        lnG, cellp = (torch.empty(B, S, dtype=torch.float64, device=device) for _ in range(2))
        lnh, ell, mask = torch.from_numpy(lnh).to(device), ell.contiguous(), post._device_state()["mask"]
        fn, stream = lib.iso_shrink_cells, dev.stream_ptr(device.index)
    sc.check(fn(_ptr(A), _ptr(mx), B, S, 0, S, _ptr(lnh), _ptr(ell), H, _ptr(mask), _ptr(lnG), _ptr(cellp), stream))
    return table, lnG, cellp


def _reweight_binned(post, theta, names, where, derived, q, stars, keep_weights):
    """:func:`reweight` for a binned model, with ``n_out`` [S] next to ``n_bad``: ``iso_shrink_cells`` once, then per slice
    of stars the weights once (``iso_shrink_weights``) and ``iso_reweight_summary`` per group of at most MAX_VALUES value
    columns."""
    from . import _shrink_cabi as sc
    grid, lnG, _ = shrink_cells(post, theta)
    Q, S, W, T, M, V, K = len(post.model.columns), post.S, post.W, post.T, post.W * post.T, len(names), q.size
    lo, hi = (0, S) if stars is None else stars
    ci32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
    axes, n_bins = ci32(grid["axes"]), ci32([len(e) - 1 for e in grid["edges"]])
    frozen_cols = ci32(grid["frozen_cols"])
    edges = np.ascontiguousarray(np.concatenate(grid["edges"]), dtype=np.float64)
    mx = post.bin_tables()[2]
    lib, rlib = sc.lib(), rc.lib()
    if post.host:
        new = lambda shape, dtype=np.float64, fill=np.nan: np.full(shape, fill, dtype=dtype)
        i32 = np.int32
        interim, frozen, mask, stream = post.interim, grid["frozen"], post.mask, None
        weigh, summarise = lib.iso_shrink_weights_host, rlib.iso_reweight_summary_host
    else:
        import torch
        device = post.storage.device
        st = post._device_state()
        new = lambda shape, dtype=torch.float64, fill=float("nan"): torch.full(shape, fill, dtype=dtype, device=device)
        i32 = torch.int32
        interim, mask = st["interim"], st["mask"]
        frozen = torch.from_numpy(grid["frozen"].view(np.uint8).copy()).to(device)
        edges = torch.from_numpy(edges).to(device)
        weigh, summarise, stream = lib.iso_shrink_weights, rlib.iso_reweight_summary, dev.stream_ptr(device.index)
    out = dict(wsum=new((S,)), ess=new((S,)), n_bad=new((S,), i32, 0), n_out=new((S,), i32, 0), mean=new((S, V)),
               sd=new((S, V)), n_nan=new((S, V), i32, 0), quant=new((S, V, K)))
    kept = new((hi - lo, M)) if keep_weights else None
    for s0, n in _slices(post, len(derived), stars):
        cols, value_derived, value_names, _model_derived = _slice_columns(post, derived, s0, n)
        weights = kept[s0 - lo:s0 - lo + n] if keep_weights else new((n, M))
        sc.check(weigh(cols, Q, _cabi.CHAIN_PARAM_MAJOR, T, S, W, s0, n, _ptr(interim), _ptr(frozen), len(grid["frozen_cols"]),
                       frozen_cols, len(grid["axes"]), axes, n_bins, _ptr(edges), _ptr(mx), _ptr(lnG), _ptr(mask),
                       _ptr(weights), _ptr(out["wsum"]), _ptr(out["ess"]), _ptr(out["n_bad"]), _ptr(out["n_out"]), stream))
        # the weights once a slice; at most MAX_VALUES value columns a summary call
        for v0 in range(0, V, rc.MAX_VALUES):
            group = range(v0, min(v0 + rc.MAX_VALUES, V))
            vals = _value_group(post, names, where, value_derived, value_names, group, s0, n)
            whole = len(group) == V
            part = out if whole else dict(mean=new((S, len(group))), sd=new((S, len(group))),
                                          n_nan=new((S, len(group)), i32, 0), quant=new((S, len(group), K)))
            rc.check(summarise(vals, len(group), _cabi.CHAIN_PARAM_MAJOR, T, S, W, s0, n, _ptr(mask),
                               q.ctypes.data_as(C.POINTER(C.c_double)), K, _ptr(weights), _ptr(part["mean"]), _ptr(part["sd"]),
                               _ptr(part["quant"]), _ptr(part["n_nan"]), stream))
            if not whole:
                for k in ("mean", "sd", "n_nan", "quant"):
                    out[k][s0:s0 + n, v0:v0 + len(group)] = part[k][s0:s0 + n]
    if keep_weights:
        out["weights"] = kept
    return out


def bin_probabilities(post, theta=None):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.star_bin_probabilities`."""
    if not post.model.binned:
        raise ValueError("star_bin_probabilities needs a population model with a Histogram column: only a binned density "
                         "has cells for a star to lie in")
    grid, _, cellp = shrink_cells(post, _theta(post, theta))
    shape = (post.S,) + tuple(len(e) - 1 for e in grid["edges"])
    if post.host:
        return np.ascontiguousarray(cellp.T).reshape(shape)
    return cellp.t().contiguous().reshape(shape)


def reweight(post, theta, names, where, derived, q, stars=None, keep_weights=False):
    """The library call over the star slices.  Returns a dict of [S]-leading arrays (numpy for a host chain, CUDA tensors
    otherwise): ``wsum``, ``ess``, ``n_bad`` [S], ``mean``, ``sd``, ``n_nan`` [S, V], ``quant`` [S, V, K]; with ``keep_weights``
    also ``weights`` [n, M] of the stars ``stars`` = (lo, hi).  Stars outside ``stars`` keep NaN / 0."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.ndim != 1 or not 1 <= q.size <= rc.MAX_PROBS:
        raise ValueError("q must hold 1 to %d probabilities (the kernel's limit)" % rc.MAX_PROBS)
    if not np.all((q > 0) & (q < 1)):
        raise ValueError("every q must lie inside (0, 1)")
    if post.model.binned:                       # histograms: the rows' sum per (star, cell), then one exp per sample
        return _reweight_binned(post, theta, names, where, derived, q, stars, keep_weights)
    rows = post.model.pack(theta)
    H, Q = rows.shape
    S, W, T, M, V, K = post.S, post.W, post.T, post.W * post.T, len(names), q.size
    ell = post._evaluate(theta if post.host else _as_tensor(post, theta))[2]     # [H, S] where the chain lies
    lib = rc.lib()
    lo, hi = (0, S) if stars is None else stars
    if post.host:
        new = lambda shape, dtype=np.float64, fill=np.nan: np.full(shape, fill, dtype=dtype)
        interim, mask, drows = post.interim, post.mask, np.ascontiguousarray(rows)
        ell = np.ascontiguousarray(ell)
        fn, stream = lib.iso_reweight_stars_host, None
    else:
        import torch
        device = post.storage.device
        st = post._device_state()
        new = lambda shape, dtype=torch.float64, fill=float("nan"): torch.full(shape, fill, dtype=dtype, device=device)
        interim, mask = st["interim"], st["mask"]
        drows = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1)).to(device)
        ell = ell.contiguous()
        fn, stream = lib.iso_reweight_stars, dev.stream_ptr(device.index)
    i32 = np.int32 if post.host else __import__("torch").int32
    out = dict(wsum=new((S,)), ess=new((S,)), n_bad=new((S,), i32, 0), mean=new((S, V)), sd=new((S, V)),
               n_nan=new((S, V), i32, 0), quant=new((S, V, K)))
    kept = new((hi - lo, M)) if keep_weights else None
    for s0, n in _slices(post, len(derived), stars):
        cols, value_derived, value_names, _model_derived = _slice_columns(post, derived, s0, n)
        weights = kept[s0 - lo:s0 - lo + n] if keep_weights else new((n, M))
        # at most MAX_VALUES value columns a call: a further group evaluates the weights again
        for v0 in range(0, V, rc.MAX_VALUES):
            group = range(v0, min(v0 + rc.MAX_VALUES, V))
            vals = _value_group(post, names, where, value_derived, value_names, group, s0, n)
            whole = len(group) == V
            part = out if whole else dict(out, mean=new((S, len(group))), sd=new((S, len(group))),
                                          n_nan=new((S, len(group)), i32, 0), quant=new((S, len(group), K)))
            rc.check(fn(cols, Q, vals, len(group), _cabi.CHAIN_PARAM_MAJOR, T, S, W, s0, n, _ptr(interim), _ptr(drows), H,
                        _ptr(ell), _ptr(mask), q.ctypes.data_as(C.POINTER(C.c_double)), K, _ptr(weights), _ptr(part["wsum"]),
                        _ptr(part["ess"]), _ptr(part["n_bad"]), _ptr(part["mean"]), _ptr(part["sd"]), _ptr(part["quant"]),
                        _ptr(part["n_nan"]), stream))
            if not whole:
                for k in ("mean", "sd", "n_nan", "quant"):
                    out[k][s0:s0 + n, v0:v0 + len(group)] = part[k][s0:s0 + n]
    if keep_weights:
        out["weights"] = kept
    return out


def _as_tensor(post, theta):
    import torch
    return torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float64)).to(post.storage.device)


def star_posteriors(post, theta=None, columns=None, q=(0.5, 0.16, 0.84), as_tensors=False):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.star_posteriors`."""
    theta = _theta(post, theta)
    names, where, derived = value_columns(post, columns)
    res = reweight(post, theta, names, where, derived, q)
    out = {}
    stats = stat_names(q)
    if len(set(stats)) != len(stats):
        raise ValueError("q repeats a probability")
    for v, col in enumerate(names):
        for k, stat in enumerate(stats):
            out["%s_%s" % (col, stat)] = res["quant"][:, v, k]
        out["%s_mean" % col] = res["mean"][:, v]
        out["%s_sd" % col] = res["sd"][:, v]
    out["ess"], out["n_bad"] = res["ess"], res["n_bad"]
    if "n_out" in res:                          # a binned model: the good samples outside its grid
        out["n_out"] = res["n_out"]
    if as_tensors:
        if post.host:
            import torch
            out = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in out.items()}
        return out
    import pandas as pd
    return pd.DataFrame({k: (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for k, a in out.items()})


def star_weights(post, theta=None, stars=None):
    """See :meth:`isochrones_amd.hierarchical.PopulationPosterior.star_weights`."""
    theta = _theta(post, theta)
    if stars is None:
        lo, hi = 0, post.S
        pick = None
    elif isinstance(stars, slice):
        lo, hi, stride = stars.indices(post.S)
        if stride != 1 or hi <= lo:
            raise ValueError("stars must be a non-empty contiguous slice, an index or a sequence of indices")
        pick = None
    else:
        pick = np.atleast_1d(np.asarray(stars, dtype=np.int64))
        if pick.size < 1 or pick.min() < 0 or pick.max() >= post.S:
            raise ValueError("stars must be indices in [0, %d)" % post.S)
        lo, hi = int(pick.min()), int(pick.max()) + 1
    names, where, derived = value_columns(post, [post.chain_names[0]])
    res = reweight(post, theta, names, where, derived, (0.5,), stars=(lo, hi), keep_weights=True)
    w, total = res["weights"], res["wsum"][lo:hi]
    if pick is not None:
        idx = pick - lo
        idx = idx if post.host else __import__("torch").from_numpy(idx).to(w.device)
        w, total = w[idx], total[idx]
    # a masked star's row is NaN, as its summaries are; a star whose weights are all zero divides 0 by 0 likewise
    if post.host:
        with np.errstate(invalid="ignore", divide="ignore"):
            return w / total[:, None]
    return w / total[:, None]
