"""A catalog fit with every optional block of its result row switched on: each column, found by its name, holds what the
block's own entry point computes from the returned chain, bit for bit, and a star without start points is a blank row with
ok = 0.  The smallest fit in which every block has something to say: W = 32 >= 2 D walkers, 16 stored steps (split chains of
8; the diagnostics kernel needs 4), 3 bands, one and two stars per system."""
import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd import _chain, catalog as cat, derived as dv, predictive as pv
from tests import _fixtures as fx

pytestmark = pytest.mark.gpu

BANDS = ("J", "H", "K")
FIT = dict(nwalkers=32, nburn=8, niter=16, seed=5)
Q = np.array([0.5, 0.16, 0.84])
STATS = ("median", "p16", "p84")
_made = {}


def _grid_and_catalog():
    """One isochrone grid and five stars drawn on it.  Star 2 has a J uncertainty of zero: log(0) in the likelihood of every
    candidate, so it has no start point.  (A magnitude that is merely far off - 40 mag too faint, say - does not do that: its
    Gaussian term is large and finite everywhere, and the star is fitted.)"""
    if not _made:
        ic = ia.synthetic_isochrone(bands=BANDS)
        c, truth = cat.synthetic_catalog(ic, 5, bands=list(BANDS), seed=8)
        c.measurements["J"][1][2] = 0.0
        _made.update(ic=ic, cat=c, truth=truth.values)
    return _made["ic"], _made["cat"], _made["truth"]


def _host_lnpost(ic, c, truth, N, stars):
    """The CPU oracle's lnpost of every star at the parameters it was drawn from (a binary: with a companion half-way down
    the EEP axis), each star with its own model."""
    oic = fx.make_oracle_ic(ic)
    eep0 = float(ic.model_grid.interp.index_columns[2][0])
    out = []
    for s in stars:
        p = truth[s]
        if N == 2:
            p = np.concatenate([[p[0], eep0 + 0.5 * (p[0] - eep0)], p[1:]])
        out.append(float(oic.lnpost(c.model(int(s), ic, N=N).model_desc(), np.ascontiguousarray(p[:, None]), parts=False)[0]))
    return np.array(out)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def _quantiles(view, nan_count):
    """[S, C, 3]: the sampler's quantile call on a [S, W, T, C] chain of its own, NaN where the column of the ensemble has
    a NaN sample."""
    import torch
    storage, S, W, _ = _chain.as_storage(view)
    out = torch.empty(S, storage.shape[1], 3, dtype=torch.float64, device=view.device)
    _chain.quantiles_layout(view.device.index, storage, storage.shape[0], S, W, storage.shape[1], Q, out)
    out = out.cpu().numpy()
    out[nan_count.cpu().numpy() > 0] = np.nan
    return out


@pytest.mark.parametrize("N,stars", [(1, (0, 1, 2, 3, 4)), (2, (0, 1, 2, 3))])
def test_every_column_by_name(N, stars):
    import torch
    ic, c, truth = _grid_and_catalog()
    stars, bad = np.array(stars), 2
    host = _host_lnpost(ic, c, truth, N, stars)
    assert np.isfinite(host[stars != bad]).all() and not np.isfinite(host[stars == bad]).any(), host
    rows, chain, lnp = cat.fit_stars_gpu(c, ic, stars, N=N, diagnostics=True, derived=True, predictive=True, return_chains=True,
                                         **FIT)
    names = cat._catalog_param_names(ic, N)
    props = dv.default_props(ic, N)
    labels = dv.expand_labels(props, N)
    cols = cat.result_columns(names, True, labels, BANDS)
    S, D = len(stars), N + 4
    assert rows.shape == (S, len(cols)) and chain.shape == (S, 32, 16, D) and len(props) == 4 and len(set(cols)) == len(cols)
    col = {n: rows[:, j] for j, n in enumerate(cols)}
    # the failed row is blank, ok is the last column
    assert cols[-1] == "ok" and np.array_equal(rows[:, -1], (stars != bad).astype(float))
    assert np.isnan(rows[stars == bad, :-1]).all() and not np.isnan(rows[stars != bad][:, :3 * D + 2]).any()
    ok = stars != bad

    dg = ia.chain_diagnostics(chain)
    tau, ess, rhat, wok = (getattr(dg, k).cpu().numpy() for k in ("tau", "ess", "rhat", "window_ok"))
    assert np.isfinite(tau[ok]).all() and np.isfinite(rhat[ok]).all()
    for j, p in enumerate(names):
        for k, v in (("tau", tau), ("ess", ess), ("rhat", rhat)):
            assert _same(col["%s_%s" % (p, k)][ok], v[ok, j]), (p, k)
    assert _same(col["tau_max"][ok], tau.max(axis=1)[ok]) and _same(col["rhat_max"][ok], rhat.max(axis=1)[ok])
    assert _same(col["window_ok"][ok], wok.min(axis=1)[ok])

    d, dnames = ia.chain_derived(chain, ic, props, N=N)
    assert dnames == labels and d.shape == (S, 32, 16, len(labels))
    dq = _quantiles(d, torch.isnan(d).sum(dim=(1, 2)))
    assert np.isfinite(dq[ok]).any()
    for j, label in enumerate(labels):
        for k, s in enumerate(STATS):
            assert _same(col["%s_%s" % (label, s)][ok], dq[ok, j, k]), (label, s)

    pcols, _ = cat.CatalogPosterior.build_columns(c, ic, N=N, indices=stars)
    r = pv.chain_predictive(chain, lnp, ic, BANDS, pcols, N=N)
    assert _same(col["ppc"][ok], r.ppc.cpu().numpy()[ok]) and np.isfinite(col["ppc"][ok]).all()
    assert _same(col["ppc_nbad"][ok], r.n_bad.cpu().numpy()[ok].astype(float))
    mq = _quantiles(r.mags, r.mag_nan)
    for j, b in enumerate(BANDS):
        for k, s in enumerate(STATS):
            assert _same(col["%s_mag_%s" % (b, s)][ok], mq[ok, j, k]), (b, s)
    term = r.term_chi2.cpu().numpy()
    for j, t in enumerate(pv.term_names(BANDS)):
        assert _same(col["chi2_" + t][ok], term[ok, j]), t
    mp = r.map_pars.cpu().numpy()
    for j, p in enumerate(names):
        assert _same(col["map_" + p][ok], mp[ok, j]), p
    # and the columns every fit has: the chain's own quantiles, its best lnpost
    q = np.percentile(chain.cpu().numpy().reshape(S, -1, D), [50, 16, 84], axis=1)     # [3, S, D]
    for j, p in enumerate(names):
        for k, s in enumerate(STATS):
            assert _same(col["%s_%s" % (p, s)][ok], q[k][ok, j]), (p, s)
    assert _same(col["lnpost_max"][ok], lnp.cpu().numpy().reshape(S, -1).max(axis=1)[ok])
