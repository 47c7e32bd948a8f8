"""The definition of include/isochrones_amd_predict.h in numpy: per-sample values operation by operation in float64 (the
header's order), the means in ``np.longdouble``; the fixtures and the ctypes calls the host-ABI and the GPU tests share."""
import ctypes as C
import functools

import numpy as np

from tests._derived_twin import bracket, interp as interp3, same_bits  # noqa: F401  (the 3-D rule is the derived header's)

ROW_MAJOR, PARAM_MAJOR = 0, 1
NSPEC = 4
BANDS9 = ("V", "J", "K", "B", "H", "G", "BP", "RP", "W1")
#: (S, W, T) of the issue; the kernel takes bands in chunks, not steps, so there is no step-chunk shape to add
#: band counts that take three and four chunks of 8, a last chunk of one, and the launch with more than 60 KB of dynamic LDS
#: (from B = 19 on; B = 32 is the largest)
WIDE_BS = (17, 19, 32)
SHAPES = ((3, 10, 7), (5, 26, 4), (1, 130, 3), (1, 193, 2))


def interp4(bc, axes, xs):
    """bc [nT, ng, nf, nA, B], four float64 arrays of N coordinates -> [N, B]; corner order 0000 .. 1111, the weight
    ((fT * fg) * ff) * fA, value = 0.0 then value + node * weight."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    with np.errstate(invalid="ignore"):
        ok = np.ones(xs[0].shape, dtype=bool)
        for ax, x in zip(axes, xs):
            ok &= ~np.isnan(x) & ~(x < ax[0]) & ~(x > ax[-1])
    it = [bracket(ax, x) for ax, x in zip(axes, xs)]
    f = [(1 - t, t) for _, t in it]
    i = [k for k, _ in it]
    v = np.zeros(xs[0].shape + (bc.shape[4],))
    with np.errstate(invalid="ignore"):
        for k in range(16):
            b = [(k >> 3) & 1, (k >> 2) & 1, (k >> 1) & 1, k & 1]
            w = ((f[0][b[0]] * f[1][b[1]]) * f[2][b[2]]) * f[3][b[3]]
            v = v + bc[i[0] + b[0], i[1] + b[1], i[2] + b[2], i[3] + b[3]] * w[:, None]
    v[~ok] = np.nan
    return v


def predict(tab, chain, lnprob, layout, n_ens, W, comps, i_dist, i_AV, obs_val, obs_unc, ens_begin=0, n_ens_out=None):
    """tab = (cols [n0, n1, nk, 4], axes3, bc [.., B], axes4); chain [T, D, rows] (PARAM_MAJOR) or [T, rows, D]; lnprob
    [T, rows] or None -> dict of the header's outputs for the ensemble range, plus the per-sample ``model`` [C, T, R, 4],
    ``z`` [T, R, B + 4] (float64) and ``good`` [T, R]."""
    cols, axes3, bc, axes4 = tab
    n_out = n_ens - ens_begin if n_ens_out is None else n_ens_out
    x = chain if layout == PARAM_MAJOR else chain.transpose(0, 2, 1)            # [T, D, rows]
    x = x[:, :, ens_begin * W:(ens_begin + n_out) * W]
    T, D, R = x.shape
    B, NT = bc.shape[4], bc.shape[4] + NSPEC
    dist, av = x[:, i_dist].ravel(), x[:, i_AV].ravel()
    with np.errstate(all="ignore"):
        dm = 5 * np.log10(dist / 10.0)
        model = np.empty((len(comps), T * R, 4))
        tot = np.zeros((T * R, B))
        for c, (p0, p1, pk) in enumerate(comps):
            v = interp3(cols, axes3, x[:, p0].ravel(), x[:, p1].ravel(), x[:, pk].ravel())
            model[c] = v
            m = (v[:, 3] + dm)[:, None] - interp4(bc, axes4, [v[:, 0], v[:, 1], v[:, 2], av])
            if len(comps) == 1:
                mags = m
            else:
                tot = tot + np.power(10.0, -0.4 * m)
        if len(comps) > 1:
            mags = -2.5 * np.log10(tot)
        mv = np.concatenate([mags, model[0][:, :3], (1000.0 / dist)[:, None]], axis=1).reshape(T, R, NT)
    out = dict(mags=np.ascontiguousarray(mags.reshape(T, R, B).transpose(0, 2, 1)), model=model.reshape(len(comps), T, R, 4))
    term, ppc = np.full((n_out, NT), np.nan), np.full(n_out, np.nan)
    n_bad = np.zeros(n_out, dtype=np.int32)
    z_all, good_all = np.full((T, R, NT), np.nan), np.zeros((T, R), dtype=bool)
    for e in range(n_out):
        ov, ou = obs_val[ens_begin + e], obs_unc[ens_begin + e]
        present = ~np.isnan(ov)
        m = mv[:, e * W:(e + 1) * W]                                             # [T, W, NT]
        with np.errstate(all="ignore"):
            d = ov - m
            z = (d * d) / (ou * ou)
        good = np.isfinite(m[:, :, present]).all(axis=2)
        z_all[:, e * W:(e + 1) * W], good_all[:, e * W:(e + 1) * W] = z, good
        n_bad[e] = good.size - good.sum()
        if good.any():
            with np.errstate(all="ignore"):
                means = z[good].astype(np.longdouble).sum(axis=0) / np.longdouble(good.sum())
            term[e, present] = means[present].astype(np.float64)
            if present.any():
                ppc[e] = np.float64(means[present].sum() / np.longdouble(present.sum()))
    mag_nan = np.isnan(out["mags"]).reshape(T, B, n_out, W).sum(axis=(0, 3)).T.astype(np.int32)
    out.update(term_chi2=term, ppc=ppc, n_bad=n_bad, z=z_all, good=good_all, mag_nan=mag_nan)
    if lnprob is not None:
        lp = lnprob[:, ens_begin * W:(ens_begin + n_out) * W]
        idx, pars = np.full(n_out, -1, dtype=np.int64), np.full((n_out, D), np.nan)
        for e in range(n_out):
            v = lp[:, e * W:(e + 1) * W].ravel()                                 # s = t * W + w
            if not np.isnan(v).all():
                best = np.max(v[~np.isnan(v)])                                   # a NaN is skipped, -inf is a value
                s = int(np.flatnonzero(v == best)[0])                            # the first of equal maxima
                idx[e] = s
                pars[e] = x[s // W, :, e * W + s % W]
        out.update(map_index=idx, map_pars=pars)
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ichrone(kind):
    """A small synthetic interpolator with nine bands."""
    import isochrones_amd as ia
    eeps = np.arange(200.0, 460.0, 4.0)
    if kind == "track":
        return ia.synthetic_track(bands=BANDS9, fehs=np.array([-1.0, -0.5, 0.0, 0.25, 0.5]),
                                  masses=np.array([0.7, 0.8, 0.9, 1.0, 1.1, 1.3, 1.6, 2.0]), eeps=eeps)
    return ia.synthetic_isochrone(bands=BANDS9, ages=np.array([8.5, 9.0, 9.3, 9.6, 9.9, 10.1]),
                                  fehs=np.array([-1.0, -0.5, 0.0, 0.5]), eeps=eeps)


@functools.lru_cache(maxsize=None)
def tables(kind, B):
    """(cols [n0, n1, nk, 4], axes3, bc [nT, ng, nf, nA, B], axes4) of :func:`ichrone`, read-only.  Beyond nine bands
    (the interpolator has no more) column j is column j mod 9 shifted by 0.01 (j div 9): a table for the C ABI alone."""
    ic = ichrone(kind)
    m, b = ic.model_grid.interp, ic.bc_grid.interp
    cols = np.ascontiguousarray(m.grid[..., list(ic._cols)], dtype=np.float64)
    bc = np.ascontiguousarray(b.grid[..., [int(i) for i in ic._band_cols(list(BANDS9[:min(B, 9)]))]], dtype=np.float64)
    if B > 9:
        bc = np.ascontiguousarray(np.stack([bc[..., j % 9] + 0.01 * (j // 9) for j in range(B)], axis=-1))
    ax3 = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in m.index_columns)
    ax4 = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in b.index_columns)
    for a in (cols, bc):
        a.setflags(write=False)
    return cols, ax3, bc, ax4


def comps_for(Cn):
    """The chain is (k_0 .. k_{C-1}, p0, p1, distance, AV): component c reads (p0, p1, k_c) -> (comps, i_dist, i_AV)."""
    return [(Cn, Cn + 1, c) for c in range(Cn)], Cn + 2, Cn + 3


def _draw(rng, ax, n, lo=None, hi=None):
    """n coordinates over one axis: uniform inside, one in 40 each on a node, above the table, below it, and NaN."""
    v = rng.uniform(ax[0] if lo is None else lo, ax[-1] if hi is None else hi, n)
    k = rng.integers(0, 40, n)
    v = np.where(k == 0, ax[rng.integers(0, ax.size, n)], v)
    v = np.where(k == 1, ax[-1] + 0.5, v)
    v = np.where(k == 2, ax[0] - 0.5, v)
    return np.where(k == 3, np.nan, v)


@functools.lru_cache(maxsize=None)
def chain(kind, S, W, T, Cn, seed=0):
    """Parameter-major storage [T, Cn + 4, S * W] over the tables of :func:`tables`, with a few samples off a table, on
    nodes (the last AV node among them) and NaN; and lnprob [T, S * W].  Read-only."""
    _, ax3, _, ax4 = tables(kind, 1)
    rng = np.random.default_rng(seed + 1000 * S + 10 * W + T + 7 * Cn)
    n = T * S * W
    x = np.empty((T, Cn + 4, S * W))
    for c in range(Cn):
        x[:, c] = _draw(rng, ax3[2], n, 220.0, 420.0).reshape(T, -1)
    x[:, Cn] = _draw(rng, ax3[0], n).reshape(T, -1)
    x[:, Cn + 1] = _draw(rng, ax3[1], n).reshape(T, -1)
    x[:, Cn + 2] = np.where(rng.integers(0, 60, n) == 0, np.nan, rng.uniform(50.0, 500.0, n)).reshape(T, -1)
    x[:, Cn + 3] = _draw(rng, ax4[3], n, 0.0, min(1.0, ax4[3][-1])).reshape(T, -1)
    lp = rng.normal(size=(T, S * W)) * 3 - 10
    x.setflags(write=False)
    lp.setflags(write=False)
    return x, lp


def observations(kind, S, B, seed=0):
    """obs_val, obs_unc [S, B + 4] near what the tables give at a mid-table star; one term in seven absent."""
    rng = np.random.default_rng(seed + S + 31 * B)
    cols, ax3, bc, ax4 = tables(kind, B)
    mid = [np.array([0.5 * (a[0] + a[-1])]) for a in ax3]
    v = interp3(cols, ax3, mid[0], mid[1], np.array([350.0]))[0]
    m = v[3] + 5 * np.log10(200.0 / 10.0) - interp4(bc, ax4, [v[:1], v[1:2], v[2:3], np.array([0.2])])[0]
    centre = np.concatenate([np.where(np.isfinite(m), m, 10.0), [v[0] if np.isfinite(v[0]) else 5800.0, 4.4, 0.0, 5.0]])
    unc = np.concatenate([np.full(B, 0.05), [100.0, 0.1, 0.15, 0.2]])
    val = centre + rng.normal(size=(S, B + 4)) * unc
    val = np.where(rng.integers(0, 7, (S, B + 4)) == 0, np.nan, val)
    return np.ascontiguousarray(val), np.ascontiguousarray(np.broadcast_to(unc, (S, B + 4)).copy())


def oracle_mags(kind, x, comps, i_dist, i_AV, B):
    """The system magnitudes [T, B, rows] by ``orc.OracleIC.interp_mag`` per component plus the addmags formula."""
    from oracle import oracle as orc
    ic = ichrone(kind)
    m, b = ic.model_grid.interp, ic.bc_grid.interp
    oic = orc.OracleIC(ic.kind, orc.OracleTable(m.grid, m.index_columns), orc.OracleTable(b.grid, b.index_columns),
                       ic._cols, ic._prior_cols, ic._astero_cols)
    T, _, R = x.shape
    bcols = ic._band_cols(list(BANDS9[:B]))
    tot, one = np.zeros((T * R, B)), None
    for p0, p1, pk in comps:
        a0, a1, ak = x[:, p0].ravel(), x[:, p1].ravel(), x[:, pk].ravel()
        # the interpolator's own parameter order: track (mass, eep, feh) on axes (feh, mass, eep); iso (eep, age, feh)
        pars = [a1, ak, a0] if kind == "track" else [ak, a0, a1]
        one = oic.interp_mag(np.array(pars + [x[:, i_dist].ravel(), x[:, i_AV].ravel()]), bcols)[3]
        with np.errstate(all="ignore"):
            tot = tot + np.power(10.0, -0.4 * one)
    with np.errstate(all="ignore"):
        mags = one if len(comps) == 1 else -2.5 * np.log10(tot)
    return mags.reshape(T, R, B).transpose(0, 2, 1)


def mags_close(a, b, tol=1e-9):
    """NaN positions identical, |a - b| <= tol * (1 + |b|) elsewhere; returns (ok, largest deviation in that measure)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, np.inf
    fin = np.isfinite(b)
    if not np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]):
        return False, np.inf
    dev = float(np.max(np.abs(a[fin] - b[fin]) / (1 + np.abs(b[fin])))) if fin.any() else 0.0
    return dev <= tol, dev


def rel_close(a, b, rtol=1e-9):
    """NaN positions identical, |a - b| <= rtol * |b| elsewhere; returns (ok, largest relative deviation)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False, np.inf
    fin = np.isfinite(b) & (b != 0)
    rest = ~fin & ~np.isnan(b)
    if not np.array_equal(a[rest], b[rest]):
        return False, np.inf
    dev = float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))) if fin.any() else 0.0
    return dev <= rtol, dev


# ---- the C ABI on numpy arrays ---------------------------------------------------------------------------------------------

def _carr(comps):
    return (C.c_int32 * (3 * len(comps)))(*[i for comp in comps for i in comp])


def host(tab, x, lp, layout, S, W, comps, i_dist, i_AV, obs_val, obs_unc, ens_begin=0, n_out=None, want=None, rc_only=False):
    """iso_predict_chain_host on numpy arrays -> dict of outputs (or the return code with ``rc_only``)."""
    from isochrones_amd import _predict_cabi as pc
    cols, ax3, bc, ax4 = tab
    n_out = S - ens_begin if n_out is None else n_out
    T = x.shape[0]
    ndim = x.shape[1] if layout == PARAM_MAJOR else x.shape[2]
    B = 3 if bc is None else bc.shape[4]
    p = lambda a: None if a is None else a.ctypes.data                          # noqa: E731
    mt = pc.IsoPredictModelTable(p(cols), p(ax3[0]), p(ax3[1]), p(ax3[2]), *([9, 9, 9] if cols is None else cols.shape[:3]), 0)
    bt = pc.IsoPredictBcTable(p(bc), *[p(a) for a in ax4], *([9, 9, 9, 9] if bc is None else bc.shape[:4]), B, 0)
    o = dict(mags=np.full((T, B, max(n_out, 1) * W), -7.0), term_chi2=np.full((max(n_out, 1), B + 4), -7.0),
             ppc=np.full(max(n_out, 1), -7.0), n_bad=np.full(max(n_out, 1), -7, dtype=np.int32),
             map_index=np.full(max(n_out, 1), -7, dtype=np.int64), map_pars=np.full((max(n_out, 1), ndim), -7.0),
             mag_nan=np.full((max(n_out, 1), max(B, 1)), -7, dtype=np.int32))
    names = ("mags", "term_chi2", "ppc", "n_bad", "map_index", "map_pars", "mag_nan")
    out = pc.IsoPredictOut(*[p(o[k]) if want is None or k in want else None for k in names])
    rc = pc.lib().iso_predict_chain_host(C.byref(mt), C.byref(bt), p(x), p(lp), layout, T, S, W, ndim, ens_begin, n_out,
                                         _carr(comps), len(comps), i_dist, i_AV, p(obs_val), p(obs_unc), C.byref(out), None)
    if rc_only:
        return rc
    assert rc == 0, pc.lib().iso_predict_last_error()
    return o


def device(tab, x, lp, layout, S, W, comps, i_dist, i_AV, obs_val, obs_unc, ens_begin=0, n_out=None, want=None):
    """iso_predict_chain on host arrays copied to the device -> dict of numpy outputs; every output starts as -7 and lies in
    front of a stretch of -7 that has to stay so."""
    import torch
    from isochrones_amd import _predict_cabi as pc, device as dev
    cols, ax3, bc, ax4 = tab
    n_out = S - ens_begin if n_out is None else n_out
    T = x.shape[0]
    ndim = x.shape[1] if layout == PARAM_MAJOR else x.shape[2]
    B = bc.shape[4]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")      # noqa: E731
    d_cols, d_bc, d_x, d_val, d_unc = up(cols), up(bc), up(x), up(obs_val), up(obs_unc)
    d_lp = None if lp is None else up(lp)
    d3, d4 = [up(a) for a in ax3], [up(a) for a in ax4]
    mt = pc.IsoPredictModelTable(d_cols.data_ptr(), *[a.data_ptr() for a in d3], *cols.shape[:3], 0)
    bt = pc.IsoPredictBcTable(d_bc.data_ptr(), *[a.data_ptr() for a in d4], *bc.shape[:4], B, 0)
    shapes = dict(mags=((T, B, n_out * W), torch.float64), term_chi2=((n_out, B + 4), torch.float64),
                  ppc=((n_out,), torch.float64), n_bad=((n_out,), torch.int32), map_index=((n_out,), torch.int64),
                  map_pars=((n_out, ndim), torch.float64), mag_nan=((n_out, B), torch.int32))
    flat, view = {}, {}
    for k, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        flat[k] = torch.full((n + 256,), -7, dtype=dt, device="cuda")
        view[k] = flat[k][:n].view(shape)
    out = pc.IsoPredictOut(*[dev.ptr(view[k]) if want is None or k in want else None for k in shapes])
    pc.check(pc.lib().iso_predict_chain(C.byref(mt), C.byref(bt), dev.ptr(d_x), dev.ptr(d_lp), layout, T, S, W, ndim,
                                        ens_begin, n_out, _carr(comps), len(comps), i_dist, i_AV, dev.ptr(d_val),
                                        dev.ptr(d_unc), C.byref(out), dev.stream_ptr(0)))
    torch.cuda.synchronize()
    for k in shapes:
        assert bool((flat[k][view[k].numel():] == -7).all()), "the kernel wrote behind the end of " + k
    return {k: view[k].cpu().numpy() for k in shapes}
