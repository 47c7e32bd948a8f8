#!/usr/bin/env python
"""TEST INFRASTRUCTURE - regenerate tests/golden/cluster/*.npz by running the reference's own StarClusterModel
(isochrones/cluster.py:182-412, cluster_utils.py) on the small synthetic tables of oracle/make_golden.py.

Needs a checkout of the reference (oracle/ref_harness.py: $ISO_REFERENCE_ROOT):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_cluster_golden.py [out_dir]

Nothing under oracle/ is changed; the harness is used as it is, with three additions made here:

* the bare ``isochrones`` package the harness registers lacks ``StarModel`` / ``get_ichrone``, which cluster.py imports
  from it: they are set on the package first (``StarModel`` from the reference's starmodel.py, ``get_ichrone`` a stub);
* ``calc_lnlike_grid`` is called with ``lnlike_prop`` transposed to its documented ``[star, eep]`` layout (the
  reference builds it ``[eep, star]``; under the pure-Python numba shim the unwrapped call raises ``IndexError`` as soon
  as the star and EEP counts differ).  The same wrapper records the per-EEP columns the reference computed;
* ``integrate_over_eeps`` is wrapped to record each row's per-star ``like_tot``.

Each fixture holds the model table, the catalog, ``meta`` (JSON), the parameter rows, what ``lnprior`` / ``lnlike`` /
``lnpost`` returned, flags for rows where the shim raised (``math.log(0)`` at fB = 0 or 1, ``0/0`` at alpha = -1), the
per-star ``like_tot`` and the per-EEP columns of every row (``col_*``, NaN-padded to the EEP range).
"""
from __future__ import annotations

import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh                    # noqa: E402
from oracle import make_golden as mg                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cluster")
EEP_BOUNDS = (151, 196)                                 # strictly inside small_iso()'s EEP axis (150 .. 197)
TRUTH = np.array([9.0, -0.1, 400.0, 0.1, -2.5, 0.3, 0.3])
N_MAX = EEP_BOUNDS[1] - EEP_BOUNDS[0] + 1


def _reference_cluster():
    rh.install_shims()
    pkg = sys.modules["isochrones"]
    if not hasattr(pkg, "StarModel"):
        pkg.StarModel = rh.ref("starmodel").StarModel

        def get_ichrone(*a, **k):
            raise RuntimeError("get_ichrone is not available to the golden generator")
        pkg.get_ichrone = get_ichrone
    return rh.ref("cluster")


class _Recorder:
    """Wraps the reference's two numba kernels inside its cluster module (see the module docstring)."""

    def __init__(self, cl):
        self.cl = cl
        self.grid_fn, self.int_fn = cl.calc_lnlike_grid, cl.integrate_over_eeps
        self.last = None

    def __enter__(self):
        def grid(lnlike_prop, model_mags, Nbands, masses, ln_dm_deeps, eeps, *rest):
            self.last = dict(mags=np.array(model_mags, dtype=float).reshape(len(eeps), Nbands),
                             mass=np.array(masses, dtype=float), lndm=np.array(ln_dm_deeps, dtype=float).reshape(-1),
                             eeps=np.array(eeps, dtype=float))
            return self.grid_fn(np.ascontiguousarray(np.asarray(lnlike_prop).T), model_mags, Nbands, masses,
                                ln_dm_deeps, eeps, *rest)

        def integ(lnlike_grid, eeps, Nstars):
            out = self.int_fn(lnlike_grid, eeps, Nstars)
            self.last["like_tot"] = np.array(out, dtype=float)
            return out

        self.cl.calc_lnlike_grid, self.cl.integrate_over_eeps = grid, integ
        return self

    def __exit__(self, *exc):
        self.cl.calc_lnlike_grid, self.cl.integrate_over_eeps = self.grid_fn, self.int_fn
        return False


def _members(ic, rng, n, bands, props):
    """Member stars drawn from the reference ic itself: EEPs at TRUTH, ~30 % binaries, photometric noise."""
    import pandas as pd
    age, feh, dist, AV = TRUTH[:4]
    pri = rng.uniform(160.0, 192.0, n)
    binary = rng.random(n) < 0.3
    sec = pri - rng.uniform(2.0, 25.0, n)
    sec = np.maximum(sec, float(EEP_BOUNDS[0]))
    _, _, _, mp = ic.interp_mag([pri, np.full(n, age), np.full(n, feh), np.full(n, dist), np.full(n, AV)], list(bands))
    _, _, _, ms = ic.interp_mag([sec, np.full(n, age), np.full(n, feh), np.full(n, dist), np.full(n, AV)], list(bands))
    mp, ms = np.asarray(mp, dtype=float), np.asarray(ms, dtype=float)
    tot = np.where(binary[:, None], -2.5 * np.log10(10 ** (-0.4 * mp) + 10 ** (-0.4 * ms)), mp)
    df = pd.DataFrame()
    for i, b in enumerate(bands):
        unc = rng.uniform(0.02, 0.05, n)
        df[b + "_mag"] = tot[:, i] + unc * rng.standard_normal(n)
        df[b + "_mag_unc"] = unc
    for p in props:
        if p == "parallax":
            df["parallax"] = 1000.0 / dist + 0.1 * rng.standard_normal(n)
            df["parallax_unc"] = 0.1
        else:
            v = np.asarray(ic.interp_value([pri, np.full(n, age), np.full(n, feh)], [p]), dtype=float).reshape(-1)
            df[p] = v + 80.0 * rng.standard_normal(n)
            df[p + "_unc"] = 80.0
    return df


def _rows(rng):
    """~20 parameter rows: a ball around TRUTH, wide draws, off-table / out-of-prior ages and the shim's undefined
    corners (fB = 0, fB = 1, alpha = -1)."""
    width = np.array([0.04, 0.05, 15.0, 0.03, 0.3, 0.08, 0.08])
    ball = TRUTH + width * rng.standard_normal((8, 7))
    ball[:, 6] = np.clip(ball[:, 6], 0.05, 0.6)
    lo = np.array([7.6, -0.9, 150.0, 0.0, -3.9, 0.0, 0.02])
    hi = np.array([10.2, 0.4, 900.0, 1.0, -1.2, 1.0, 0.6])
    wide = rng.uniform(lo, hi, size=(6, 7))
    edge = []
    for col, v in ((0, 7.2), (0, 10.2), (0, 9.75), (6, 0.0), (6, 1.0), (4, -1.0), (2, 60000.0)):
        r = TRUTH.copy()
        r[col] = v
        edge.append(r)
    return np.vstack([ball, wide, np.array(edge)])


def run_case(name, bands, props, nan_cells=(), n_stars=12, seed=0, out=OUT):
    cl = _reference_cluster()
    cat = rh.ref("catalog")
    rng = np.random.default_rng(seed)
    g, ax, cols = mg.small_iso()
    g = g.copy()
    ci = list(cols).index("initial_mass")
    for (a, f, e) in nan_cells:                     # mid-track holes: non-contiguous EEP sets
        g[a, f, e, ci] = np.nan
    bc = mg.small_bc()
    limits = mg.limits_of("iso", ax)
    ic = rh.make_ref_ic("iso", (g, ax, cols), bc, limits, (ax[2][0], ax[2][-1]))
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = _members(ic, rng, n_stars, bands, props)
    stars = cat.StarCatalog(df, bands=list(bands), props=list(props))
    pars = _rows(rng)
    n = pars.shape[0]
    minq = np.full(n, 0.1)
    minq[rng.choice(n - 7, 3, replace=False)] = 0.6      # heavy minq on three ball / wide rows
    lnprior, lnlike, lnpost = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    undefined = np.zeros(n, dtype=bool)
    like_tot = np.full((n, n_stars), np.nan)
    c_n = np.zeros(n, dtype=np.int64)
    c_eep, c_mass, c_lndm = (np.full((n, N_MAX), np.nan) for _ in range(3))
    c_mags = np.full((n, N_MAX, len(bands)), np.nan)
    c_props = np.full((n, N_MAX, len(props)), np.nan)
    models = {}
    for q in sorted(set(minq)):
        models[q] = cl.StarClusterModel(ic, stars, eep_bounds=EEP_BOUNDS, minq=float(q))
    rec = _Recorder(cl)
    with rec, np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(n):
            mod = models[minq[i]]
            p = pars[i]
            lnprior[i] = mod.lnprior(p)
            rec.last = None
            try:
                lnlike[i] = mod.lnlike(p)
                lnpost[i] = lnprior[i] + lnlike[i] if np.isfinite(lnprior[i]) else -np.inf
            except (ValueError, ZeroDivisionError, IndexError):
                undefined[i] = True
                lnlike[i] = np.nan
                lnpost[i] = -np.inf if not np.isfinite(lnprior[i]) else np.nan
            if not undefined[i]:
                lp = mod.lnpost(p)                      # the reference's own lnpost (starmodel.py:538-542)
                assert (lp == lnpost[i]) or (np.isnan(lp) and np.isnan(lnpost[i])), (name, i, lp, lnpost[i])
            r = rec.last
            if r is not None and not undefined[i]:
                k = r["eeps"].size
                c_n[i] = k
                c_eep[i, :k], c_mass[i, :k], c_lndm[i, :k], c_mags[i, :k] = r["eeps"], r["mass"], r["lndm"], r["mags"]
                for j, q in enumerate(props):
                    if q == "parallax":
                        c_props[i, :k, j] = 1000.0 / p[2]
                    elif k:
                        c_props[i, :k, j] = np.asarray(ic.interp_value([r["eeps"], p[0], p[1]], [q]), dtype=float).reshape(-1)
                like_tot[i] = r["like_tot"]
    meta = dict(bands=list(bands), props=list(props), eep_bounds=list(EEP_BOUNDS), limits={k: list(map(float, v)) for k, v in limits.items()},
                model_columns=list(cols), mass_bounds=[float(limits["mass"][0]), float(limits["mass"][1])],
                nan_cells=[list(map(int, c)) for c in nan_cells], truth=TRUTH.tolist(), halo_fraction=0.5, max_AV=1.0,
                max_distance=50000.0, param_names=list(cl.StarClusterModel.param_names))
    cat_arrays = {}
    for b in bands:
        cat_arrays["mag_" + b] = df[b + "_mag"].to_numpy(float)
        cat_arrays["unc_" + b] = df[b + "_mag_unc"].to_numpy(float)
    for q in props:
        cat_arrays["prop_" + q] = df[q].to_numpy(float)
        cat_arrays["propunc_" + q] = df[q + "_unc"].to_numpy(float)
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, name + ".npz"), meta=json.dumps(meta, sort_keys=True), model_grid=g,
                        model_ax0=ax[0], model_ax1=ax[1], model_ax2=ax[2], bc_grid=bc[0],
                        **{"bc_ax%d" % i: np.asarray(a, float) for i, a in enumerate(bc[1])}, bc_columns=np.array(bc[2]),
                        pars=pars, minq=minq, lnprior=lnprior, lnlike=lnlike, lnpost=lnpost, undefined=undefined,
                        like_tot=like_tot, col_n=c_n, col_eep=c_eep, col_mass=c_mass, col_lndm=c_lndm, col_mags=c_mags,
                        col_props=c_props, **cat_arrays)
    print("%-22s rows=%d finite lnlike=%d -inf=%d undefined=%d" % (
        name, n, np.isfinite(lnlike).sum(), np.isneginf(lnlike).sum(), undefined.sum()))


def main(out=OUT):
    run_case("cluster_jhk", ("J", "H", "K"), (), seed=11, out=out)
    run_case("cluster_props", ("J", "H", "K"), ("parallax", "Teff"), seed=12, out=out)
    # holes at ages 9.0 / 9.5 (index 3, 4), feh -0.5 / 0.0 (index 1, 2), EEP nodes 170 / 171 / 180 (index 20, 21, 30)
    holes = [(a, f, e) for a in (3, 4) for f in (1, 2) for e in (20, 21, 30)]
    run_case("cluster_holes_phot6", ("J", "H", "K", "G", "BP", "RP"), (), nan_cells=holes, seed=13, out=out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
