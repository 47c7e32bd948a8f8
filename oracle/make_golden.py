#!/usr/bin/env python
"""TEST INFRASTRUCTURE — regenerate tests/golden/*.npz by running the *reference* itself.

Run in the authoring container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py

Each fixture is pure data: small synthetic tables (isochrones_amd.grids recipe), seeded
sample points, and what the reference's own functions return for them —
``DFInterpolator.__call__``, ``ModelGridInterpolator.interp_value / interp_mag`` and
``Single/Binary/TripleStarModel.lnprior / lnlike / lnpost`` (isochrones/interp.py,
models.py, mags.py, likelihood.py, priors.py, starmodel.py).  No reference source is stored.
"""
from __future__ import annotations

import itertools
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import user_priors                # noqa: E402
from isochrones_amd import grids as G         # noqa: E402

OUT = os.environ.get("ISO_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")     # (override: tests/test_goldens_reproducible.py)
BANDS = ("J", "H", "K", "G", "BP", "RP", "V")


def small_bc():
    teff, logg, feh, av = G.bc_axes()
    axes = (teff[0:24:6].tolist() + [teff[19]], logg[15:20], np.array([-1.25, -1.0, -0.5, 0.0, 0.5, 0.75]),
            np.array([0.0, 0.1, 0.4, 1.0]))
    axes = (np.sort(np.array(axes[0])),) + axes[1:]
    return G.synthetic_bc_grid(BANDS, axes)


def small_track():
    fehs = np.array([-1.0, -0.5, -0.25, 0.0, 0.5])
    masses = np.array([0.3, 0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0, 4.0, 8.0])
    eeps = np.arange(420.0, 468.0)
    return G.synthetic_track_grid(fehs, masses, eeps)


def small_iso():
    ages = np.array([7.5, 8.0, 8.5, 9.0, 9.5, 9.75, 10.0, 10.25])
    fehs = np.array([-1.0, -0.5, 0.0, 0.5])
    eeps = np.arange(150.0, 198.0)
    return G.synthetic_iso_grid(ages, fehs, eeps)


def limits_of(kind, axes):
    if kind == "track":
        f, m, e = axes
        return dict(mass=(m[0], m[-1]), feh=(f[0], f[-1]), age=(5.0, 8.6), eep=(e[0], e[-1]))
    a, f, e = axes
    return dict(mass=(0.1, 300.0), feh=(f[0], f[-1]), age=(a[0], a[-1]), eep=(e[0], e[-1]))


def sample_pars(rng, kind, n_stars, axes, n_wide, n_ball):
    """[n, n_params] rows: wide uniform (5% beyond the table so some are out of grid), a
    posterior-like ball, and hand-picked edge cases."""
    if kind == "track":
        f, m, e = axes
        lo = np.array([m[0], e[0], f[0], 1.0, 0.0])
        hi = np.array([m[-1], e[-1], f[-1], 250.0, 1.0])
        centre = np.array([1.02, 440.3, -0.1, 100.0, 0.2])
        width = np.array([0.08, 6.0, 0.12, 8.0, 0.08])
    else:
        a, f, e = axes
        lo = np.array([e[0]] * n_stars + [a[0], f[0], 1.0, 0.0])
        hi = np.array([e[-1]] * n_stars + [a[-1], f[-1], 600.0, 1.0])
        centre = np.array([185.0, 178.0, 171.0][:n_stars] + [9.4, -0.1, 400.0, 0.2])
        width = np.array([4.0] * n_stars + [0.15, 0.12, 20.0, 0.08])
    span = hi - lo
    wide = rng.uniform(lo - 0.05 * span, hi + 0.05 * span, size=(n_wide, lo.size))
    inside = rng.uniform(lo, hi, size=(n_wide, lo.size))
    ball = centre + width * rng.standard_normal((n_ball, lo.size))
    if kind == "iso" and n_stars > 1:   # mostly ordered eeps, some deliberately not
        k = n_stars
        for arr in (inside, ball):
            half = arr.shape[0] // 4 * 3
            arr[:half, :k] = -np.sort(-arr[:half, :k], axis=1)
    edge = []
    c = centre.copy()
    edge.append(c.copy())
    for j in range(lo.size):                       # NaN in each slot
        r = c.copy(); r[j] = np.nan; edge.append(r)
    # exact interior node hits on every table axis, and exact lower edges
    if kind == "track":
        r = c.copy(); r[0] = m[4]; edge.append(r)
        r = c.copy(); r[1] = e[10]; edge.append(r)
        r = c.copy(); r[2] = f[2]; edge.append(r)
        r = c.copy(); r[0], r[1], r[2] = m[3], e[7], f[1]; edge.append(r)
        r = c.copy(); r[0] = m[0]; edge.append(r)
        r = c.copy(); r[1] = e[0]; edge.append(r)
        r = c.copy(); r[2] = f[0]; edge.append(r)
        r = c.copy(); r[0] = 0.55; r[1] = 453.5; edge.append(r)    # next to the NaN tail
        r = c.copy(); r[0] = 0.55; r[1] = 454.0; edge.append(r)    # zero weight on a NaN corner
        r = c.copy(); r[0] = 0.4; r[1] = 460.0; edge.append(r)     # inside the NaN tail
        r = c.copy(); r[0] = 6.0; edge.append(r)                   # too hot for the BC table
    else:
        k = n_stars
        r = c.copy(); r[0] = e[20]; edge.append(r)
        r = c.copy(); r[k] = a[3]; edge.append(r)
        r = c.copy(); r[k + 1] = f[1]; edge.append(r)
        r = c.copy(); r[0] = e[0]; r[k] = a[0]; r[k + 1] = f[0]; edge.append(r)
        r = c.copy(); r[k] = 9.9; r[0] = 156.0; edge.append(r)     # near the missing pre-MS points
        r = c.copy(); r[k] = 10.1; r[0] = 152.0; edge.append(r)    # inside them
        if k >= 2:
            r = c.copy(); r[0], r[1] = 170.0, 180.0; edge.append(r)          # wrong order
            r = c.copy(); r[0], r[1] = 180.0, 180.0; edge.append(r)          # equal
        if k == 3:
            r = c.copy(); r[0], r[1], r[2] = 170.0, 180.0, 175.0; edge.append(r)
            r = c.copy(); r[0], r[1], r[2] = 170.0, 180.0, 185.0; edge.append(r)
            r = c.copy(); r[0], r[1], r[2] = 190.0, 180.0, 185.0; edge.append(r)
    for j in (lo.size - 2, lo.size - 1):           # distance / AV at and beyond their bounds
        for v in (0.0, -1.0, 1e5 if j == lo.size - 2 else 1.5):
            r = c.copy(); r[j] = v; edge.append(r)
    return np.vstack([wide, inside, ball, np.array(edge)])


OBS = {
    "spec_phot_plx": dict(Teff=(5770, 100), logg=(4.5, 0.1), feh=(0.0, 0.15), V=(10.0, 0.05), parallax=(10.0, 0.1)),
    "phot6_plx": dict(J=(9.3, 0.02), H=(9.0, 0.02), K=(8.95, 0.02), BP=(10.7, 0.002), RP=(9.8, 0.002),
                      G=(10.3, 0.001), parallax=(2.5, 0.05)),
    "spec_only": dict(Teff=(5800, 100), logg=(4.5, 0.1), parallax=(10.0, 0.1)),
    "phot_only": dict(J=(9.3, 0.05), K=(8.9, 0.05)),
    "astero": dict(Teff=(5770, 100), V=(10.0, 0.05), nu_max=(2800.0, 60.0), delta_nu=(130.0, 2.0)),
}


def _ref_prior(spec):
    """("Gaussian", mean, sigma, lo, hi) etc. -> a prior object of the REFERENCE (isochrones/priors.py)."""
    pr = rh.ref("priors")
    fam, args = spec[0], list(spec[1:])
    if fam == "Gaussian":
        return pr.GaussianPrior(args[0], args[1], bounds=tuple(args[2:4]) if len(args) == 4 else None)
    if fam == "LogNormal":
        return pr.LogNormalPrior(args[0], args[1])
    if fam == "Flat":
        return pr.FlatPrior(tuple(args))
    if fam == "FlatLog":
        return pr.FlatLogPrior(tuple(args))
    if fam == "PowerLaw":
        return pr.PowerLawPrior(args[0], tuple(args[1:3]))
    if fam == "Chabrier":          # ("Chabrier", lo, hi): the reference's class takes nothing but bounds
        return pr.ChabrierPrior(bounds=tuple(args[0:2]))
    if fam == "Broken":            # ("Broken", mu, sigma, alpha, pl_lo, pl_hi, breakpoint, lo, hi)
        return pr.BrokenPrior([pr.LogNormalPrior(args[0], args[1]), pr.PowerLawPrior(args[2], tuple(args[3:5]))],
                              [args[5]], bounds=tuple(args[6:8]))
    if fam == "Feh":               # ("Feh", halo_fraction, local, lo, hi)
        p = pr.FehPrior(halo_fraction=args[0], local=bool(args[1]))
        p.bounds = tuple(args[2:4])
        return p
    if fam == "User":              # ("User", class name, ...): oracle/user_priors.py on the reference's base classes
        return user_priors.build(pr, spec)
    raise ValueError(fam)


def edge_rows(centre, column, values):
    """The centre row with one coordinate replaced, once per value."""
    rows = np.repeat(np.asarray(centre, dtype=float)[None, :], len(values), axis=0)
    rows[:, column] = values
    return rows


def _ulp_edges(prior, lo, hi, inner=()):
    """(value, where, the reference must say) for a prior with bounds (lo, hi): on them, one ulp outside them, and
    ``inner``, further (value, where, expectation) triples."""
    return [(lo, "lo", "finite"), (hi, "hi", "finite"), (float(np.nextafter(lo, -np.inf)), "below lo", "-inf"),
            (float(np.nextafter(hi, np.inf)), "above hi", "-inf")] + list(inner)


def run_model_case(name, kind, n_stars, obs_key, model_table, bc_table, rng, n_wide, n_ball, extra_kw=None,
                   priors=None, eep_orig_prior=None, edges=None, check=None):
    """``edges`` (the prior-edge cases only): {parameter: [(value, where, expectation)]} - rows appended to the sampled
    ones, the centre row with that one parameter replaced; ``check(arrays)``: further assertions of the generator."""
    sm = rh.ref("starmodel")
    limits = limits_of(kind, model_table[1])
    axes = model_table[1]
    eep_bounds = (axes[2][0], axes[2][-1])
    ic = rh.make_ref_ic(kind, model_table, bc_table, limits, eep_bounds)
    cls = {1: sm.SingleStarModel, 2: sm.BinaryStarModel, 3: sm.TripleStarModel}[n_stars]
    obs = dict(OBS[obs_key])
    kw = dict(extra_kw or {})
    mod = cls(ic, **obs, **kw)
    if priors:                     # StarModel.set_prior (starmodel.py:629-632)
        mod.set_prior(**{k: _ref_prior(v) for k, v in priors.items()})
    if eep_orig_prior:             # the prior the EEP term transforms (priors.py:409-429) is an attribute
        mod._priors["eep"].orig_prior = _ref_prior(eep_orig_prior)
    pars = sample_pars(rng, kind, n_stars, axes, n_wide, n_ball)
    edge_meta = []
    if edges is not None:
        centre = pars[2 * n_wide + n_ball]             # sample_pars' first hand-picked row
        for par, triples in edges.items():
            col = list(mod.param_names).index(par)
            for v, where, expect in triples:
                edge_meta.append(dict(row=int(pars.shape[0]), column=col, par=par, where=where, expect=expect))
                pars = np.vstack([pars, edge_rows(centre, col, [v])])
    n = pars.shape[0]
    lnprior, lnlike, lnpost = np.empty(n), np.empty(n), np.empty(n)
    # math.log10(distance <= 0) raises under the pure-Python numba shim where compiled numba
    # follows libm (-inf / NaN); such direct lnlike calls are flagged and not compared.
    lnlike_undefined = np.zeros(n, dtype=bool)
    lnpost_undefined = np.zeros(n, dtype=bool)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            for i in range(n):
                p = pars[i]
                lnprior[i] = mod.lnprior(p)
                try:
                    lnlike[i] = mod.lnlike(p)
                except ValueError:
                    lnlike[i] = np.nan
                    lnlike_undefined[i] = True
                if edges is None:
                    lnpost[i] = mod.lnpost(p)
                    continue
                try:                                   # a prior that admits distance <= 0 lets lnpost reach that logarithm
                    lnpost[i] = mod.lnpost(p)
                except ValueError:
                    lnpost[i] = np.nan
                    lnpost_undefined[i] = True
    # the primary's interp_value / interp_mag at the same points
    prim = np.column_stack([pars[:, 0]] + [pars[:, n_stars + j] for j in range(4)])
    pcols = ["Teff", "logg", "feh", "Mbol"] + (["age", "dt_deep"] if kind == "track" else ["mass", "dm_deep"]) \
        + ["nu_max", "delta_nu"]
    with np.errstate(all="ignore"):
        vals = ic.interp_value([prim[:, 0], prim[:, 1], prim[:, 2]], pcols)
        good = prim[:, 3] > 0      # log10(distance <= 0): see lnlike_undefined above
        Teff, logg, feh = (np.full(n, np.nan) for _ in range(3))
        mags = np.full((n, len(BANDS)), np.nan)
        Teff[good], logg[good], feh[good], mags[good] = ic.interp_mag(
            [prim[good, j] for j in range(5)], list(BANDS))
    cube = rng.random((16, n_stars + 4))
    cube_out = cube.copy()
    with np.errstate(all="ignore"):
        for row in cube_out:
            mod.mnest_prior(row, None, None)
    custom = bool(priors or eep_orig_prior)
    meta = dict(priors=priors or {}, eep_orig_prior=eep_orig_prior, kind=kind, n_stars=n_stars, obs={k: list(map(float, v)) for k, v in obs.items()}, kwargs=kw,
                limits={k: list(map(float, v)) for k, v in limits.items()}, eep_bounds=list(map(float, eep_bounds)),
                bands=list(BANDS), model_columns=list(model_table[2]), interp_value_cols=pcols,
                param_names=list(mod.param_names),
                mass_norms=[] if custom else list(map(float, mod._priors["mass"].norms)),
                feh_norm=float("nan") if custom else float(mod._priors["feh"]._norm),
                distance_bounds=list(map(float, mod.bounds("distance"))), AV_bounds=list(map(float, mod.bounds("AV"))))
    out = dict(meta=json.dumps(meta), pars=pars, lnprior=lnprior, lnlike=lnlike, lnpost=lnpost,
               interp_value=np.asarray(vals), Teff=Teff, logg=logg, feh=feh, mags=mags,
               cube_in=cube, cube_out=cube_out, lnlike_undefined=lnlike_undefined,
               mag_defined=good)
    if edges is not None:
        c = 2 * n_wide + n_ball
        assert np.isfinite(lnpost[c]) and not lnpost_undefined[c], "%s: the centre row is not finite" % name
        for e in edge_meta:
            i = e["row"]
            if e["expect"] == "finite":                # on or inside the prior's bounds: never flagged, never excluded
                assert not (lnlike_undefined[i] or lnpost_undefined[i]), (name, e)
                assert np.isfinite(lnprior[i]) and np.isfinite(lnpost[i]), (name, e, lnprior[i], lnpost[i])
            elif e["expect"] == "-inf":
                assert lnprior[i] == -np.inf and lnpost[i] == -np.inf, (name, e, lnprior[i], lnpost[i])
        if check is not None:
            check(dict(pars=pars, lnprior=lnprior, lnpost=lnpost, interp_value=np.asarray(vals), cols=pcols))
        meta["edges"] = edge_meta
        out["meta"] = json.dumps(meta)
        out["lnpost_undefined"] = lnpost_undefined
        # what the reference's base classes make of a user's prior, term by term: lnpdf(x), and prior(x) where it has one
        for par, spec in (priors or {}).items():
            if spec[0] != "User":
                continue
            pr, x = mod._priors[par], pars[:, list(mod.param_names).index(par)]
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                out["user_%s_lnpdf" % par] = np.array([pr.lnpdf(float(v)) for v in x], dtype=float)
                if callable(pr):
                    out["user_%s_call" % par] = np.array([pr(float(v)) for v in x], dtype=float)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print("%-28s n=%d  finite lnpost=%d  -inf=%d  nan=%d" % (
        name, n, np.isfinite(lnpost).sum(), np.isneginf(lnpost).sum(), np.isnan(lnpost).sum()))


def run_interp_kats(rng):
    """The reference's data-free tests: isochrones/tests/test_interp.py:11-46 (3-D) and the
    recorded answers of docs/interpolate.ipynb cells 3, 5, 12, 14 (2-D, incl. a ragged table)."""
    import pandas as pd
    interp = rh.ref("interp")
    out = {}
    # -- 3-D (tests/test_interp.py) --
    xx, yy, zz = [np.arange(10 + np.log10(n)) * n for n in [1, 10, 100]]
    func = lambda x, y, z: x ** 2 * np.cos(y / 10) + z
    df = pd.DataFrame([(x, y, z, func(x, y, z)) for x, y, z in itertools.product(xx, yy, zz)],
                      columns=["x", "y", "z", "val"]).set_index(["x", "y", "z"])
    dfi = interp.DFInterpolator(df)
    pts = rng.random(size=(200, 3)) * 9
    pts[:, 1] *= 10
    pts[:, 2] *= 100
    pts[0] = [6.0, 50.0, 200.0]       # exact node (test_interp.py:27,31)
    pts[1] = [3.1, 44.0, 503.0]       # test_interp.py:28,35
    out["t3_axes0"], out["t3_axes1"], out["t3_axes2"] = xx, yy, zz
    out["t3_grid"] = dfi.grid
    out["t3_pts"] = pts
    out["t3_vals"] = dfi([pts[:, 0], pts[:, 1], pts[:, 2]], ["val"])
    out["t3_scalar"] = np.array([dfi([6.0, 50.0, 200.0], ["val"])[0], dfi([3.1, 44.0, 503.0], ["val"])[0]])
    # -- 2-D (docs/interpolate.ipynb) --
    x = np.arange(1, 4)
    y = np.arange(1, 6)
    index = pd.MultiIndex.from_product((x, y), names=["x", "y"])
    df2 = pd.DataFrame(index=index)
    df2["sum"] = [a + b for a, b in itertools.product(x, y)]
    df2["product"] = [a * b for a, b in itertools.product(x, y)]
    df2["power"] = [a ** b for a, b in itertools.product(x, y)]
    d2 = interp.DFInterpolator(df2)
    d2m = interp.DFInterpolator(df2.drop([(3, 3), (3, 4)]))
    out["t2_axes0"], out["t2_axes1"] = x.astype(float), y.astype(float)
    out["t2_grid"] = d2.grid
    out["t2_grid_missing"] = d2m.grid
    q = np.array([[1.4, 2.1], [2.2, 4.6], [1.3, 2.2], [2.3, 3.0]])
    out["t2_pts"] = q
    out["t2_vals"] = np.array([d2([a, b]) for a, b in q])
    out["t2_vals_missing"] = np.array([d2m([a, b]) for a, b in q])
    # recorded notebook answers, as printed there
    out["t2_doc_cell3"] = np.array([3.5, 2.94, 2.36])          # interp([1.4, 2.1])
    out["t2_doc_cell5"] = np.array([10.12])                    # interp([2.2, 4.6], ['product'])
    out["t2_doc_cell12"] = np.array([3.5, 2.86, 2.14])         # interp_missing([1.3, 2.2])
    out["t2_doc_cell14"] = np.array([np.nan, np.nan, np.nan])  # interp_missing([2.3, 3])
    # -- 4-D random table, generic columns --
    ax4 = [np.sort(rng.uniform(0, 10, n)) for n in (5, 6, 4, 7)]
    g4 = rng.standard_normal((5, 6, 4, 7, 3))
    d4 = rh.make_ref_dfinterp(g4, ax4, ["a", "b", "c"])
    p4 = np.column_stack([rng.uniform(a[0] - 0.2, a[-1] + 0.2, 300) for a in ax4])
    p4[0] = [a[2] for a in ax4]
    p4[1] = [a[0] for a in ax4]
    with np.errstate(all="ignore"):
        v4 = d4([p4[:, 0], p4[:, 1], p4[:, 2], p4[:, 3]], ["c", "a"])
    for i, a in enumerate(ax4):
        out["t4_axes%d" % i] = a
    out["t4_grid"], out["t4_pts"], out["t4_vals"] = g4, p4, v4
    np.savez_compressed(os.path.join(OUT, "interp_kats.npz"), **out)
    print("interp_kats: 3d max|err vs func-free check skipped; %d + %d + %d points" % (len(pts), len(q), len(p4)))


def run_interp_edges():
    """The reference's DFInterpolator on the uniform-step tables of tests/_interp_twin.edge_tables() (U2, U3, U4: axes i*step
    with a step that is no power of two, NaN nodes next to the probes where an O(1) index guess is off by one) at their node
    and next-to-node probes.  Probes with a coordinate at the last node of an axis are left
    out: the reference reads past the table there.  Only the probes and the answers are stored; the tables come from the
    twin's fixed seeds."""
    # the tables are made in one place, the test package's twin: this import needs the repository root on sys.path, which the
    # head of this script puts there (also when tests/test_goldens_reproducible.py runs it in a subprocess)
    from tests import _interp_twin as tw
    out = {}
    for name, t in tw.edge_tables(list(tw.UNIFORM)).items():
        keep = np.ones(t.probes.shape[0], dtype=bool)
        for d, a in enumerate(t.axes):
            keep &= ~(t.probes[:, d] == a[-1])
        pts = t.probes[keep]
        dfi = rh.make_ref_dfinterp(t.grid, t.axes, t.columns)
        with np.errstate(all="ignore"):
            vals = dfi([pts[:, d] for d in range(t.nd)], t.columns)
        out[name + "_pts"], out[name + "_vals"] = pts, np.asarray(vals, dtype=float)
        print("interp_edges %s: %d points, %d finite values" % (name, pts.shape[0], np.isfinite(vals).sum()))
    np.savez_compressed(os.path.join(OUT, "interp_edges.npz"), **out)


def run_eep_case():
    """interp_eeps of the reference (isochrones/interp.py:488-558) on ragged age arrays built
    from a small synthetic track table whose EEP axis starts at 1 (the reference's assumption)."""
    from isochrones_amd.interp import DFInterpolator
    from isochrones_amd.ingest import ragged_age_arrays
    interp = rh.ref("interp")
    rng = np.random.default_rng(424242)
    fehs = np.array([-1.0, -0.5, 0.0, 0.5])
    masses = np.array([0.5, 0.58, 0.62, 0.8, 1.0, 1.2, 2.0, 5.0, 7.0])
    eeps = np.arange(1.0, 481.0)
    g, ax, cols = G.synthetic_track_grid(fehs, masses, eeps)          # ragged: m<0.6 stops at 454
    # make the raggedness richer: cut a few more tracks short
    for (i, j, last) in [(0, 3, 300), (1, 4, 120), (2, 6, 77), (3, 8, 410), (2, 2, 5)]:
        g[i, j, last:, :] = np.nan
    dfi = DFInterpolator.from_arrays(g, ax, cols)
    ages, lengths = ragged_age_arrays(dfi, "age")
    dt = np.full_like(ages, 1.0)
    n = 4000
    x1 = rng.uniform(0.45, 7.3, n)                                    # mass (some out of range)
    x0 = rng.uniform(-1.1, 0.55, n)                                   # feh
    x = rng.uniform(4.8, 11.0, n)                                     # log age (some beyond every track)
    x[:5] = np.nan
    x0[5:8] = np.nan
    x0[8], x1[8] = fehs[1], masses[4]                                 # exact nodes
    x0[9], x1[9] = fehs[0], masses[0]
    x[10] = ages[4 + 9 * 2, 100]                                      # exact age hit on a track
    x0[10], x1[10] = fehs[2], masses[4]
    with np.errstate(all="ignore"):
        want = interp.interp_eeps(x, x0, x1, fehs, masses, len(masses), ages, dt, lengths)
    np.savez_compressed(os.path.join(OUT, "interp_eep.npz"), fehs=fehs, masses=masses, ages=ages, lengths=lengths,
                        age=x, feh=x0, mass=x1, eep=want)
    print("interp_eep: n=%d finite=%d nan=%d" % (n, np.isfinite(want).sum(), np.isnan(want).sum()))
    # second fixture: repeated ages inside tracks and many exact hits.  The reference's searchsorted returns the
    # index of the equal element its bisection lands on (interp.py:26-29), which inside a run of equal ages is
    # neither the first nor the last of the run - the probe sequence itself is part of the behaviour.
    ages2 = ages.copy()
    for t in rng.choice(ages2.shape[0], 24, replace=False):
        L = int(lengths[t])
        for _ in range(6):
            if L > 12:
                a0 = int(rng.integers(1, L - 8))
                ages2[t, a0:a0 + int(rng.integers(2, 8))] = ages2[t, a0]
    n = 6000
    x1 = rng.uniform(0.5, 7.0, n)
    x0 = rng.uniform(-1.0, 0.5, n)
    x = rng.uniform(4.8, 11.0, n)
    fin = ages2[np.isfinite(ages2)]
    x[:3000] = rng.choice(fin, 3000)                                  # ages that are in the table
    for k in range(3000, 3600):                                       # ... queried on the very track they come from
        i, j = int(rng.integers(0, fehs.size - 1)), int(rng.integers(0, masses.size - 1))    # (the upper edge is undefined in the reference)
        L = int(lengths[i * masses.size + j])
        if L:
            x[k], x0[k], x1[k] = ages2[i * masses.size + j, int(rng.integers(0, L))], fehs[i], masses[j]
    with np.errstate(all="ignore"):
        want2 = interp.interp_eeps(x, x0, x1, fehs, masses, len(masses), ages2, dt, lengths)
    np.savez_compressed(os.path.join(OUT, "interp_eep_plateaus.npz"), fehs=fehs, masses=masses, ages=ages2,
                        lengths=lengths, age=x, feh=x0, mass=x1, eep=want2)
    print("interp_eep_plateaus: n=%d finite=%d nan=%d" % (n, np.isfinite(want2).sum(), np.isnan(want2).sum()))


def _tree_cases(obs_mod, ic):
    """(name, reference tree builder kwargs) — the configurations of docs/multiple.ipynb cells 21-36
    plus the keyword form used by tests/test_likelihood.py."""
    def build(name):
        obs = obs_mod.ObservationTree(name=name)
        for band, m in zip("JHK", (12.11, 11.74, 11.68)):
            o = obs_mod.Observation("2MASS", band, 4)
            o.add_source(obs_mod.Source(m, 0.02))
            obs.add_observation(o)
        o = obs_mod.Observation("AO", "K", 0.1)
        o.add_source(obs_mod.Source(0.0, 0.02, separation=0, pa=0, relative=True, is_reference=True))
        o.add_source(obs_mod.Source(2.43, 0.02, separation=0.2, pa=100, relative=True, is_reference=False))
        obs.add_observation(o)
        return obs
    spec = dict(parallax=(2.0, 0.05), Teff=(5834.0, 100), logg=(4.43, 0.15), feh=(-0.01, 0.1))
    return [
        ("tree_resolved", build, dict(spec)),
        ("tree_resolved_unassoc", build, dict(spec, index=[0, 1])),
        ("tree_triple1", build, dict(N=[2, 1], index=[0, 0], parallax=(2.0, 0.05))),
        ("tree_triple2", build, dict(N=[1, 2], index=[0, 1], Teff=(5834.0, 100))),
        ("tree_double_binary", build, dict(N=2, index=[0, 1], AV=(0.2, 0.1))),
        ("tree_kwargs_single", None, dict(Teff=(5800, 100), logg=(4.5, 0.1), J=(13.3, 0.05), K=(12.9, 0.05),
                                          parallax=(2.0, 0.1))),
        ("tree_kwargs_binary", None, dict(J=(13.3, 0.05), K=(12.9, 0.05), parallax=(2.0, 0.1), N=2)),
        ("tree_kwargs_triple", None, dict(Teff=(5800, 100), J=(13.3, 0.05), K=(12.9, 0.05), N=3, maxAV=0.6)),
        # the tree meets system 1 (one star) before system 0 (two stars): prior_transform / mnest_prior walk
        # obs.Nstars.items() (starmodel.py:618,646) while the parameter vector is laid out by ascending system index
        # (observation.py:1116-1130), so the reference scales some slots with other parameters' bounds here
        ("tree_out_of_order", build, dict(N=[1, 2], index=[1, 0], parallax=(2.0, 0.05))),
    ]


def run_tree_cases():
    """Generic StarModel + ObservationTree of the reference (starmodel.py:63-661,
    observation.py) on the small synthetic isochrone table."""
    sm = rh.ref("starmodel")
    obs_mod = rh.ref("observation")
    rng = np.random.default_rng(777)
    iso, bc = small_iso(), small_bc()
    axes = iso[1]
    limits = limits_of("iso", axes)
    for name, build, kw in _tree_cases(obs_mod, None):
        ic = rh.make_ref_ic("iso", iso, bc, limits, (axes[2][0], axes[2][-1]))
        kw = dict(kw)
        obs = build(name) if build is not None else None
        mod = sm.StarModel(ic, obs=obs, **kw)
        _emit_tree_case(name, mod, kw, build is not None, rng, axes, limits, obs_mod)


def _emit_tree_case(name, mod, kw, built, rng, axes, limits, obs_mod, extra_meta=None, edges=None, n_rows=400):
    if True:
        names = list(mod.param_names)
        N = mod.obs.Nstars
        # parameter samples: per system descending eeps near the table's middle, some violations
        n = n_rows
        cols = []
        for s in mod.obs.systems:
            e = rng.uniform(axes[2][0] - 2, axes[2][-1] + 2, size=(n, N[s]))
            e[: int(0.85 * n)] = -np.sort(-e[: int(0.85 * n)], axis=1)
            cols.append(e)
            cols.append(rng.uniform(axes[0][0] - 0.05, axes[0][-1] + 0.05, (n, 1)))       # age
            cols.append(rng.uniform(axes[1][0] - 0.05, axes[1][-1] + 0.05, (n, 1)))       # feh
            cols.append(rng.uniform(100.0, 900.0, (n, 1)))                                # distance
            cols.append(rng.uniform(-0.02, 1.02, (n, 1)))                                 # AV
        pars = np.hstack(cols)
        pars[0, 0] = np.nan
        if edges is not None:                          # (centre row, {parameter: [(value, where, expectation)]})
            centre, per_par = edges
            edge_meta = []
            pars = np.vstack([pars[:n_rows - 1], np.asarray(centre, dtype=float)[None, :]])
            for par, triples in per_par.items():
                col = names.index(par)
                for v, where, expect in triples:
                    edge_meta.append(dict(row=int(pars.shape[0]), column=col, par=par, where=where, expect=expect))
                    pars = np.vstack([pars, edge_rows(centre, col, [v])])
            n = pars.shape[0]
        lnprior, lnlike, lnpost = np.empty(n), np.empty(n), np.empty(n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with np.errstate(all="ignore"):
                for i in range(n):
                    lnprior[i] = mod.lnprior(pars[i])
                    lnlike[i] = mod.lnlike(pars[i])
                    lnpost[i] = mod.lnpost(pars[i])
        # the tree's structure as plain data
        labels = mod.obs.leaf_labels
        nodes = []
        for nd in mod.obs:
            if isinstance(nd, obs_mod.ObsNode) and not isinstance(nd, obs_mod.DummyObsNode):
                nodes.append(dict(band=nd.band, relative=bool(nd.relative), mag=nd.value[0], unc=nd.value[1],
                                  leaves=[l.label for l in nd.leaves],
                                  ref_leaves=[l.label for l in nd.reference.leaves] if nd.reference is not None else None))
        cube = rng.random((8, len(names)))
        meta = dict(param_names=names, leaf_labels=labels, nodes=nodes, kwargs={k: (list(v) if isinstance(v, (tuple, list)) else v)
                                                                               for k, v in kw.items()},
                    limits={k: list(map(float, v)) for k, v in limits.items()}, eep_bounds=[float(axes[2][0]), float(axes[2][-1])],
                    bands=list(BANDS), built=built, systems=[int(s) for s in mod.obs.systems],
                    Nstars={str(k): int(v) for k, v in N.items()})
        meta.update(extra_meta or {})
        if edges is not None:
            c = n_rows - 1
            assert np.isfinite(lnpost[c]), "%s: the centre row is not finite" % name
            for e in edge_meta:
                i = e["row"]
                if e["expect"] == "finite":
                    assert np.isfinite(lnprior[i]) and np.isfinite(lnpost[i]), (name, e, lnprior[i], lnpost[i])
                else:
                    assert lnprior[i] == -np.inf and lnpost[i] == -np.inf, (name, e, lnprior[i], lnpost[i])
            meta["edges"] = edge_meta
        # StarModel.mnest_prior (starmodel.py:644-656) on non-degenerate cubes: unlike prior_transform it sorts every
        # system's EEPs in descending order.  Own generator, so the arrays above keep their values.
        import zlib
        mcube = np.random.default_rng(zlib.crc32(name.encode())).random((32, len(names)))
        mnest = mcube.copy()
        for row in mnest:
            mod.mnest_prior(row, len(names), len(names))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), pars=pars, lnprior=lnprior,
                            lnlike=lnlike, lnpost=lnpost, cube_in=cube,
                            cube_out=np.array([mod.prior_transform(c) for c in cube]), mnest_in=mcube, mnest_out=mnest)
        print("%-24s n=%d npar=%d finite lnpost=%d -inf=%d nan=%d leaves=%s" % (
            name, n, len(names), np.isfinite(lnpost).sum(), np.isneginf(lnpost).sum(), np.isnan(lnpost).sum(), labels))


# The photometry rows of tests/golden/ini/<case>/star.ini, written out the way the reference's
# StarModel.from_ini assembles them (starmodel.py:336-424: per section, per band, the tagged companions
# in order, then the (0, 0.01) reference row of a relative section) before ObservationTree.from_df.
# (from_ini itself needs configobj, which is not installed, so the rows are spelled out here and the
# reference takes over from from_df on.)
def _rows(instrument, resolution, relative, bands):
    out = []
    for band, entries in bands:
        for sep, pa, mag, e in entries:
            out.append(dict(name=instrument, band=band, resolution=resolution, relative=relative, separation=sep,
                            pa=pa, mag=mag, e_mag=e))
        if relative:
            out.append(dict(name=instrument, band=band, resolution=resolution, relative=relative, separation=0.0,
                            pa=0.0, mag=0.0, e_mag=0.01))
    return out


INI_CASES = {
    "single": dict(
        kwargs=dict(Teff=(5750, 98.0), feh=(-0.06, 0.16), logg=(4.41, 0.1)),
        rows=_rows("2MASS", 4.0, False, [("J", [(0, 0, 13.413, 0.02)]), ("H", [(0, 0, 13.045, 0.02)]),
                                         ("K", [(0, 0, 12.993, 0.02)])])
        + _rows("GaiaDR3", 4.0, False, [("G", [(0, 0, 14.6, 0.05)]), ("RP", [(0, 0, 14.1, 0.05)])]),
        variants={"": {}}),
    "binary": dict(
        kwargs={},
        rows=_rows("GaiaDR3", 4.0, False, [("G", [(10, 100, 15.9, 0.02), (0, 0, 14.7, 0.02)]),
                                           ("BP", [(10, 100, 16.4, 0.02), (0, 0, 15.1, 0.02)]),
                                           ("RP", [(10, 100, 15.3, 0.02), (0, 0, 14.2, 0.02)])])
        + _rows("2MASS", 4.0, False, [("J", [(10, 100, 14.513, 0.02), (0, 0, 13.513, 0.02)]),
                                      ("H", [(10, 100, 14.045, 0.02), (0, 0, 13.145, 0.02)]),
                                      ("K", [(10, 100, 13.993, 0.02), (0, 0, 13.093, 0.02)])]),
        variants={"": {}, "_unassoc": dict(index=[0, 1])}),
    "triple": dict(
        kwargs=dict(maxAV=0.9, Teff=(5700, 98.0), feh=(-0.1, 0.16), logg=(4.45, 0.1)),
        rows=_rows("2MASS", 4.0, False, [("J", [(0, 0, 13.313, 0.02)]), ("H", [(0, 0, 12.945, 0.02)]),
                                         ("K", [(0, 0, 12.893, 0.02)])])
        + _rows("KeckAO", 0.1, True, [("K", [(0.6, 100, 1.66, 0.05), (1.2, 200, 2.1, 0.1)]),
                                      ("H", [(0.6, 100, 1.77, 0.03), (1.2, 200, 2.2, 0.1)]),
                                      ("J", [(0.6, 100, 1.84, 0.05), (1.2, 200, 2.35, 0.1)])]),
        variants={"": {}, "_unassoc1": dict(index=[0, 0, 1]), "_unassoc2": dict(index=[0, 1, 1])}),
    "triple_b": dict(
        kwargs=dict(maxAV=0.7, Teff=(5810, 90), feh=(0.05, 0.12), logg=(4.40, 0.09)),
        rows=_rows("2MASS", 4.0, False, [("J", [(0, 0, 13.31, 0.02)]), ("H", [(0, 0, 12.96, 0.02)]),
                                         ("K", [(0, 0, 12.91, 0.015)])])
        + _rows("ShaneAO", 0.5, True, [("H", [(2.95, 41.5, 1.41, 0.01), (9.4, 230.0, 2.55, 0.01)]),
                                       ("K", [(2.95, 41.5, 1.36, 0.05)])]),
        variants={"": {}, "_unassoc2": dict(index=[0, 1, 1])}),
    "flat": dict(
        kwargs=dict(J=(13.3, 0.05), H=(12.95, 0.05), K=(12.9, 0.05), Teff=(5800, 150), parallax=(2.0, 0.1)),
        rows=None, variants={"": {}, "_N2": dict(N=2)}),
}


class _stable_argsort:
    """The reference picks a new node's parent with ``np.argsort(distances)`` (observation.py:1260) and takes
    the first candidate; coincident sources tie at distance 0.  numpy's default sort is not stable (the
    AVX-512 kernels of numpy 2 reorder ties even in 8-element arrays), which makes the reference's tree depend
    on the numpy build — on this machine the two-star, six-band file even yields a tree it then cannot
    evaluate.  The goldens are generated with ties kept in iteration order (the result of the reference on any
    numpy whose small-array sort is insertion sort), which is also what isochrones_amd.observation does."""

    def __enter__(self):
        self._orig = np.argsort
        orig = self._orig

        def argsort(a, *args, **kw):
            if not args and "kind" not in kw:
                kw["kind"] = "stable"
            return orig(a, *args, **kw)
        np.argsort = argsort

    def __exit__(self, *exc):
        np.argsort = self._orig


def run_ini_cases():
    """The star.ini fixtures (tests/golden/ini/) as the reference's generic StarModel sees them."""
    import pandas as pd
    sm = rh.ref("starmodel")
    obs_mod = rh.ref("observation")
    rng = np.random.default_rng(4242)
    iso, bc = small_iso(), small_bc()
    axes = iso[1]
    limits = limits_of("iso", axes)
    for case, spec in INI_CASES.items():
        for suffix, extra in spec["variants"].items():
            ic = rh.make_ref_ic("iso", iso, bc, limits, (axes[2][0], axes[2][-1]))
            obs = None
            kw = dict(spec["kwargs"], **extra)
            with _stable_argsort():
                if spec["rows"] is not None:
                    df = pd.DataFrame(spec["rows"], columns=["name", "band", "resolution", "relative", "separation",
                                                             "pa", "mag", "e_mag"])
                    obs = obs_mod.ObservationTree.from_df(df)
                mod = sm.StarModel(ic, obs=obs, **kw)
            _emit_tree_case("ini_" + case + suffix, mod, kw, False, rng, axes, limits, obs_mod,
                            extra_meta=dict(ini=case, from_ini_kwargs=extra))


def run_isotrack_case():
    """IsoTrackModel of the reference (starmodel.py:2010-2104) on a small isochrone table and a
    small track table that share their EEP range."""
    sm = rh.ref("starmodel")
    rng = np.random.default_rng(99)
    trk, bc = small_track(), small_bc()
    iso = G.synthetic_iso_grid(np.array([7.5, 8.0, 8.5, 9.0, 9.5, 9.75, 10.0, 10.25]), np.array([-1.0, -0.5, 0.0, 0.5]),
                               np.arange(420.0, 468.0))
    lim_t, lim_i = limits_of("track", trk[1]), limits_of("iso", iso[1])
    eb = (420.0, 467.0)
    ic_t = rh.make_ref_ic("track", trk, bc, lim_t, eb)
    ic_i = rh.make_ref_ic("iso", iso, bc, lim_i, eb)
    obs = dict(Teff=(5770, 100), logg=(4.5, 0.1), V=(10.0, 0.05), J=(9.2, 0.03), parallax=(10.0, 0.1))
    mod = sm.IsoTrackModel(ic_i, ic_t, **obs)
    n = 600
    pars = np.column_stack([rng.uniform(418, 469, n), rng.uniform(0.28, 8.2, n), rng.uniform(7.4, 8.7, n),
                            rng.uniform(-1.05, 0.55, n), rng.uniform(20, 210, n), rng.uniform(-0.02, 1.02, n)])
    ball = np.array([440.0, 1.0, 8.2, -0.1, 100.0, 0.2]) + np.array([5, 0.05, 0.1, 0.1, 5, 0.05]) * rng.standard_normal((300, 6))
    pars = np.vstack([pars, ball])
    pars[0, 2] = np.nan
    n = pars.shape[0]
    lnprior, lnlike, lnpost = np.empty(n), np.empty(n), np.empty(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            for i in range(n):
                lnprior[i] = mod.lnprior(pars[i])
                lnlike[i] = mod.lnlike(pars[i])
                lnpost[i] = mod.lnpost(pars[i])
    meta = dict(obs={k: list(map(float, v)) for k, v in obs.items()}, limits_track={k: list(map(float, v)) for k, v in lim_t.items()},
                limits_iso={k: list(map(float, v)) for k, v in lim_i.items()}, eep_bounds=list(eb), bands=list(BANDS),
                iso_columns=list(iso[2]))
    np.savez_compressed(os.path.join(OUT, "isotrack.npz"), meta=json.dumps(meta), pars=pars, lnprior=lnprior, lnlike=lnlike,
                        lnpost=lnpost, iso_grid=iso[0], iso_ax0=iso[1][0], iso_ax1=iso[1][1], iso_ax2=iso[1][2])
    print("isotrack: n=%d finite=%d -inf=%d nan=%d" % (n, np.isfinite(lnpost).sum(), np.isneginf(lnpost).sum(),
                                                       np.isnan(lnpost).sum()))


def run_prior_cases(rng=None):
    """Non-default prior families through set_prior (every family the device evaluates), including the
    reference's quirk that set_prior on the parameter EEP replaces does NOT reach the EEP term (EEP_prior
    keeps the object it was built with, starmodel.py:1447 + :629-632), and the explicit re-assignment of
    EEP_prior.orig_prior that does."""
    rng = rng or np.random.default_rng(20240808)
    trk, iso, bc = small_track(), small_iso(), small_bc()
    run_model_case("track_single_custom_priors", "track", 1, "spec_phot_plx", trk, bc, rng, 250, 250,
                   priors=dict(mass=("LogNormal", float(np.log(1.0)), 0.4), age=("Gaussian", 9.6, 0.3, 8.0, 10.1),
                               feh=("Flat", -1.5, 0.4), distance=("Gaussian", 150.0, 60.0, 1.0, 600.0),
                               AV=("PowerLaw", 0.5, 0.0, 1.0)))
    run_model_case("track_single_eep_orig_prior", "track", 1, "phot_only", trk, bc, rng, 150, 150,
                   priors=dict(mass=("PowerLaw", -2.35, 0.1, 10.0), AV=("Gaussian", 0.2, 0.1, 0.0, 1.0)),
                   eep_orig_prior=("Gaussian", 9.6, 0.3, 8.0, 10.1))
    run_model_case("iso_binary_custom_priors", "iso", 2, "phot6_plx", iso, bc, rng, 250, 250,
                   priors=dict(mass=("PowerLaw", -2.35, 0.1, 10.0), age=("Flat", 8.5, 10.1),
                               feh=("Gaussian", -0.2, 0.3, -1.0, 0.5), distance=("LogNormal", float(np.log(300.0)), 0.5),
                               AV=("Gaussian", 0.2, 0.1, 0.0, 1.0)),
                   eep_orig_prior=("LogNormal", float(np.log(0.9)), 0.5))
    run_model_case("iso_single_flatlog_age", "iso", 1, "spec_only", iso, bc, rng, 100, 100,
                   priors=dict(age=("FlatLog", 8.0, 10.0), distance=("PowerLaw", 2.0, 0.0, 500.0)))


def _case_rng(name):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode()))      # per case: the older fixtures keep their draws


def run_prior_edge_cases():
    """Every route a prior takes, pinned on its branch points.  Device families with parameters the records must carry
    (a broken prior = the device's Chabrier family with its own mu, sigma, alpha and breakpoint; FehPrior with a
    halo fraction, disk and bounds of its own), the same families behind the EEP term (the ``prior(x)`` form), and priors
    a user wrote (oracle/user_priors.py), which the reference itself normalises and evaluates here.  Besides a few hundred
    sampled rows every case has the centre row with one parameter put ON each bound of its prior, one ulp outside it,
    and for a broken prior on its breakpoint, one ulp below it and around the power law's own bounds.

    One bound is open in the reference: ``BrokenPrior._lnpdf`` (priors.py:209-211) has no bounds test, so below its lower
    bound ``lnpdf`` is the log-normal's value (the upper bound is closed by the power law's own test when both end there,
    as here).  That row is recorded with the expectation "open" and compared like any other."""
    trk, iso, bc = small_track(), small_iso(), small_bc()
    inf = float("inf")
    # --- device families ---
    mu, sg, al, plo, phi, bp, lo, hi = float(np.log(0.3)), 0.5, -1.8, 0.6, 3.5, 0.9, 0.45, 3.5
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    mass_edges = [(lo, "lo", "finite"), (hi, "hi", "finite"), (dn(lo), "below lo", "open"), (up(hi), "above hi", "-inf"),
                  (bp, "breakpoint", "finite"), (float(np.nextafter(bp, 0)), "below breakpoint", "finite"),
                  (plo, "power law lo", "finite"), (dn(plo), "below power law lo", "finite"),
                  (up(plo), "above power law lo", "finite"), (dn(phi), "below power law hi", "finite")]
    run_model_case("track_single_chabrier_feh", "track", 1, "phot_only", trk, bc, _case_rng("track_single_chabrier_feh"),
                   100, 100,
                   priors=dict(mass=("Broken", mu, sg, al, plo, phi, bp, lo, hi), feh=("Feh", 0.2, False, -0.8, 0.35),
                               AV=("Gaussian", 0.3, 0.2, 0.05, 0.9)),
                   # (the reference cannot CALL a Gaussian without bounds, priors.py:54-56 on bounds = None: infinite ones)
                   eep_orig_prior=("Gaussian", 9.6, 0.3, -inf, inf),
                   edges=dict(mass=mass_edges, feh=_ulp_edges("feh", -0.8, 0.35), AV=_ulp_edges("AV", 0.05, 0.9)))

    obp = 0.215                    # (the synthetic isochrones put 0.17 - 0.35 solar masses at these EEPs)

    def both_sides(a):
        m = a["interp_value"][:, a["cols"].index("mass")]
        fin = np.isfinite(a["lnprior"])
        assert (fin & (m < obp)).sum() > 10 and (fin & (m >= obp)).sum() > 10, ((fin & (m < obp)).sum(), (fin & (m >= obp)).sum())
        assert (np.isneginf(a["lnprior"]) & np.isfinite(m) & ((m < 0.18) | (m > 0.31))).sum() > 0    # outside its bounds

    run_model_case("iso_binary_chabrier_orig", "iso", 2, "phot6_plx", iso, bc, _case_rng("iso_binary_chabrier_orig"), 100, 100,
                   priors=dict(age=("Flat", 8.2, 9.7), feh=("Feh", 0.05, True, -0.7, 0.3)),
                   eep_orig_prior=("Broken", float(np.log(0.2)), 0.3, -2.7, 0.19, 0.31, obp, 0.18, 0.31),
                   edges=dict(age=_ulp_edges("age", 8.2, 9.7), feh=_ulp_edges("feh", -0.7, 0.3)), check=both_sides)
    # --- a user's priors ---
    tri_feh, far = ("User", "Triangle", -0.6, 0.4), ("User", "ForeignExp", 300.0, 5.0, 240.0)
    run_model_case("track_single_user_priors", "track", 1, "spec_phot_plx", trk, bc, _case_rng("track_single_user_priors"),
                   100, 100, priors=dict(feh=tri_feh, distance=far),
                   edges=dict(feh=_ulp_edges("feh", -0.6, 0.4), distance=_ulp_edges("distance", 5.0, 240.0)))
    run_model_case("iso_binary_user_priors", "iso", 2, "phot6_plx", iso, bc, _case_rng("iso_binary_user_priors"), 100, 100,
                   priors=dict(AV=("User", "Triangle", 0.05, 0.8)), edges=dict(AV=_ulp_edges("AV", 0.05, 0.8)))
    run_model_case("track_single_overriding_subclasses", "track", 1, "spec_phot_plx", trk, bc,
                   _case_rng("track_single_overriding_subclasses"), 100, 100,
                   priors=dict(feh=("User", "Skew", -0.1, 0.25, -0.7, 0.4), AV=("User", "Tilt", 0.02, 0.9),
                               distance=("User", "Over", 2.0, 5.0, 240.0)),
                   edges=dict(feh=_ulp_edges("feh", -0.7, 0.4), AV=_ulp_edges("AV", 0.02, 0.9),
                              distance=_ulp_edges("distance", 5.0, 240.0)))
    # --- the resolved binary of run_tree_cases with a user's AV prior (the generic model tests the bounds itself) ---
    sm, obs_mod = rh.ref("starmodel"), rh.ref("observation")
    axes = iso[1]
    limits = limits_of("iso", axes)
    name, build, kw = _tree_cases(obs_mod, None)[0]
    assert name == "tree_resolved"
    ic = rh.make_ref_ic("iso", iso, bc, limits, (axes[2][0], axes[2][-1]))
    mod = sm.StarModel(ic, obs=build(name), **dict(kw))
    spec = ("User", "Triangle", 0.05, 0.8)
    mod.set_prior(AV=_ref_prior(spec))
    _emit_tree_case("tree_resolved_user_av", mod, dict(kw), True, _case_rng("tree_resolved_user_av"), axes, limits, obs_mod,
                    extra_meta=dict(priors=dict(AV=list(spec))), n_rows=200,
                    edges=([185.0, 170.0, 9.4, -0.1, 500.0, 0.2], dict(AV_0=_ulp_edges("AV", 0.05, 0.8))))


# ------------------------------------------------------------------------------------------------
# table ingest ("next" row f1): the reference's own grid classes on small synthetic raw frames
# ------------------------------------------------------------------------------------------------

def _raw_mist_rows(rng, keys, key_names, eep_counts):
    """Raw MIST-like rows (the column names of the .eep / .iso files the reference parses, mist/models.py:23-33)
    for every key tuple; row counts differ, so the product grid is ragged."""
    import pandas as pd
    frames = []
    for key, n in zip(keys, eep_counts):
        eep = np.arange(1, n + 1, dtype=float)
        m0 = key[key_names.index("initial_mass")] if "initial_mass" in key_names else 0.5 + 0.02 * eep + 0.1 * rng.random()
        feh = key[0] if key_names[0] == "initial_feh" else key[1]
        d = dict(zip(key_names, [np.full(n, k) for k in key]))
        d["EEP"] = eep
        d["initial_mass"] = m0 * np.ones(n)
        d["star_mass"] = d["initial_mass"] * (1.0 - 2e-3 * eep / n)
        d["star_age"] = 1e6 * 10 ** (3.4 * (eep / 40.0) ** 0.7) / np.mean(d["initial_mass"]) ** 2.5 * (1 + 0.01 * rng.random(n))
        d["log_Teff"] = 3.76 + 0.12 * np.log10(d["initial_mass"]) - 1.5e-3 * eep + 0.002 * feh
        d["log_g"] = 4.45 - 0.03 * eep
        d["log_L"] = 3.5 * np.log10(d["initial_mass"]) + 0.012 * eep
        d["log_R"] = 0.8 * np.log10(d["initial_mass"]) + 6e-3 * eep
        d["log_surf_z"] = np.log10(0.0142 * 10.0 ** feh) - 1e-4 * eep
        d["surface_h1"] = 0.715 - 2e-4 * eep
        d["delta_nu"] = 135.0 * np.sqrt(d["initial_mass"]) / (1 + 0.02 * eep)
        d["nu_max"] = 3090.0 * d["initial_mass"] / (1 + 0.04 * eep)
        d["phase"] = np.floor(eep / 12.0)
        d["interpolated"] = np.zeros(n)
        frames.append(pd.DataFrame(d))
    return pd.concat(frames, ignore_index=True)


def run_ingest_cases(seed=4242, save=True):
    """MISTEvolutionTrackGrid / MISTIsochroneGrid / MISTBolometricCorrectionGrid of the reference on synthetic raw
    frames: column standardisation + derived columns (models.py:102-109, mist/models.py:81-85,219-223), dt_deep
    (mist/models.py:403-435), dm_deep (models.py:126-153), the ragged age arrays (models.py:171-203), the
    NaN-padded dense grids (interp.py:590-614), and the BC frame -> band columns -> Rv slice -> dense 4-D table
    (bc.py:99-118, mist/bc.py:161-233).  Inputs and outputs are stored as plain arrays."""
    import tempfile
    import pandas as pd
    mm = rh.ref("mist.models")
    mbc = rh.ref("mist.bc")
    rng = np.random.default_rng(seed)
    out = {}
    # the committed fixture is seed 4242 with the table shapes below; any other seed (tests/test_ingest_golden.py's
    # container-only sweep) also draws the shapes
    vary = np.random.default_rng(seed + 1) if seed != 4242 else None

    def axis(default, lo, hi, step):
        if vary is None:
            return np.array(default)
        n = int(vary.integers(2, 6))
        return np.sort(vary.choice(np.arange(lo, hi, step), n, replace=False)).round(6)
    with tempfile.TemporaryDirectory() as tmp, rh.memory_hdf() as hdf, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # ---- evolution tracks ----
        fehs = axis([-0.5, 0.0, 0.25], -2.0, 0.6, 0.25)
        masses = axis([0.8, 1.0, 1.2, 1.5], 0.3, 3.0, 0.1)
        keys = list(itertools.product(fehs, masses))
        counts = [int(c) for c in rng.integers(18, 36, len(keys))]
        raw_t = _raw_mist_rows(rng, keys, ("initial_feh", "initial_mass"), counts)

        class Tracks(mm.MISTEvolutionTrackGrid):
            n_eep = max(counts)
            datadir = os.path.join(tmp, "tracks")

            def df_all(self):
                df = raw_t.copy().sort_values(by=list(self.index_cols))
                df.index = [df[c] for c in self.index_cols]
                return df

        Tracks.fehs = fehs
        os.makedirs(Tracks.datadir)
        g = Tracks()
        df = g.df
        age, dt, lengths = g.get_array_grids()
        out.update(track_raw=raw_t.values, track_raw_columns=np.array(list(raw_t.columns)),
                   track_columns=np.array(list(df.columns)), track_values=df.values,
                   track_index=np.array([list(t) for t in df.index.values], dtype=float),
                   track_grid=g.interp.grid, track_axes0=g.interp.index_columns[0], track_axes1=g.interp.index_columns[1],
                   track_axes2=g.interp.index_columns[2], track_age_arrays=age, track_dt_deep_arrays=dt,
                   track_lengths=lengths)
        print("ingest tracks: %d rows, grid %s, %d NaN cells" % (len(df), g.interp.grid.shape,
                                                                  int(np.isnan(g.interp.grid[..., 0]).sum())))
        # ---- isochrones ----
        ages = axis([8.5, 9.0, 9.5, 10.0], 7.0, 10.3, 0.05)
        ifehs = axis([-1.0, 0.0, 0.5], -2.0, 0.6, 0.25)
        keys = list(itertools.product(ages, ifehs))
        counts = [int(c) for c in rng.integers(15, 30, len(keys))]
        raw_i = _raw_mist_rows(rng, keys, ("log10_isochrone_age_yr", "feh"), counts)
        # an isochrone's rows: initial mass grows along EEP (what dm_deep differentiates)
        raw_i["initial_mass"] = 0.3 + 0.03 * raw_i["EEP"] ** 1.1 + 0.02 * raw_i["feh"]
        raw_i["star_mass"] = raw_i["initial_mass"] * 0.999

        class Isos(mm.MISTIsochroneGrid):
            datadir = os.path.join(tmp, "isos")

            def df_all(self):
                df = raw_i.copy().sort_values(by=list(self.index_cols))
                df.index = [df[c] for c in self.index_cols]
                return df

        os.makedirs(Isos.datadir)
        gi = Isos()
        dfi = gi.df
        out.update(iso_raw=raw_i.values, iso_raw_columns=np.array(list(raw_i.columns)),
                   iso_columns=np.array(list(dfi.columns)), iso_values=dfi.values,
                   iso_index=np.array([list(t) for t in dfi.index.values], dtype=float),
                   iso_grid=gi.interp.grid, iso_axes0=gi.interp.index_columns[0], iso_axes1=gi.interp.index_columns[1],
                   iso_axes2=gi.interp.index_columns[2])
        print("ingest isochrones: %d rows, grid %s" % (len(dfi), gi.interp.grid.shape))
        # ---- bolometric corrections: two photometric systems, five index levels incl. Rv ----
        lv = (np.array([3500.0, 5000.0, 6500.0, 8000.0]), np.array([3.0, 4.0, 5.0]), np.array([-1.0, 0.0, 0.5]),
              np.array([0.0, 0.5, 1.0]), np.array([2.5, 3.1, 4.0]))
        idx = pd.MultiIndex.from_product(lv, names=["Teff", "logg", "[Fe/H]", "Av", "Rv"])
        bcdir = os.path.join(tmp, "BC", "mist")
        os.makedirs(bcdir)

        class BC(mbc.MISTBolometricCorrectionGrid):
            datadir = bcdir

        frames = {}
        for phot, cols in (("UBVRIplus", ["Bessell_B", "Bessell_V", "2MASS_J", "2MASS_Ks", "Gaia_G_DR2Rev", "TESS",
                                          "Kepler_Kp"]),
                           ("WISE", ["WISE_W1", "WISE_W2"])):
            frames[phot] = pd.DataFrame(rng.normal(size=(len(idx), len(cols))), index=idx, columns=cols)
            hdf.preload(os.path.join(bcdir, "%s.h5" % phot), "df", frames[phot])
        bands = ["J", "K", "G", "W1", "V", "Kepler", "TESS"]
        gb = BC(bands=bands)
        dfb = gb.df
        out.update(bc_index=np.array([list(t) for t in idx.values], dtype=float), bc_bands=np.array(bands),
                   bc_columns=np.array(list(dfb.columns)), bc_grid=gb.interp.grid,
                   **{"bc_axes%d" % k: gb.interp.index_columns[k] for k in range(4)})
        for phot, fr in frames.items():
            out["bc_%s_values" % phot] = fr.values
            out["bc_%s_columns" % phot] = np.array(list(fr.columns))
        print("ingest BC: frame %s -> grid %s, columns %s" % (dfb.shape, gb.interp.grid.shape, list(dfb.columns)))
        # band-name resolution (mist/bc.py:165-233)
        names = ["J", "H", "K", "Ks", "G", "BP", "RP", "Bp", "Rp", "U", "B", "V", "R", "I", "u", "g", "r", "i", "z", "W1", "W2",
                 "W3", "W4", "Kepler", "kep", "Kp", "TESS", "Tycho_B", "Hipparcos_Hp", "WFPC2_F555W", "UKIRT_K", "UK_J",
                 "HST_WFPC2_F555W", "Gaia_G_MAW", "UBVRIplus_Bessell_V"]
        names += ["nonsense", "PanSTARRS_g", "SDSS_g"]

        def resolve(b):
            try:
                return BC.get_band(b)
            except ValueError:
                return ("!unresolved", "!unresolved")

        got = [resolve(b) for b in names]
        out.update(band_names=np.array(names), band_phot=np.array([p for p, _ in got]), band_column=np.array([c for _, c in got]))
    # the reference orders the track columns through a set() and joins the BC frames in set order, both of which depend on
    # the interpreter's string hash seed: store every table with its columns sorted by name, so that regenerating this
    # file gives the same bytes
    for pre, grid_keys in (("track", ("track_values", "track_grid")), ("iso", ("iso_values", "iso_grid")), ("bc", ("bc_grid",))):
        names = [str(c) for c in out[pre + "_columns"]]
        order = np.argsort(names)
        out[pre + "_columns"] = np.array([names[k] for k in order])
        for key in grid_keys:
            out[key] = np.ascontiguousarray(out[key][..., order])
    if save:
        np.savez_compressed(os.path.join(OUT, "ingest.npz"), **out)
    return out



# ------------------------------------------------------------------------------------------------
# the reference's data directory ($ISOCHRONES) as its own classes lay it out, on small synthetic frames
# ------------------------------------------------------------------------------------------------

def run_datadir_case(seed=777):
    """A small ``$ISOCHRONES`` tree written by the reference's own code - ``MISTEvolutionTrackGrid().interp`` /
    ``MISTIsochroneGrid().interp`` save ``full_grid<tag>.npz`` through ``DFInterpolator(df, filename=...)``
    (grid.py:132-137, interp.py:590-614, models.py:163-165), ``get_array_grids()`` saves ``array_grid<tag>.npz``
    (models.py:171-203) - plus what a user exports once where pytables exists: the BC frames
    (``ingest.export_frame_npz`` of the frames behind ``BC/mist/<phot>.h5``) and the axis vectors of each model grid
    (``mist.export_axes`` of the frame's index levels; the real MIST grids do not need them).  And, in
    ``datadir.npz``, what the reference's MIST interpolators / star models built on these very grids return at seeded
    sample points: ``interp_value``, ``interp_mag``, ``SingleStarModel.lnprior / lnlike / lnpost``.
    tests/golden/isochrones_tree/ is then what ``get_ichrone('mist')`` of this build must load."""
    import shutil
    import pandas as pd
    from isochrones_amd import ingest, mist as our_mist
    mm = rh.ref("mist.models")
    mbc = rh.ref("mist.bc")
    miso = rh.ref("mist.isochrone")
    sm = rh.ref("starmodel")
    rng = np.random.default_rng(seed)
    tree = os.path.join(OUT, "isochrones_tree")
    shutil.rmtree(tree, ignore_errors=True)
    tdir, idir, bcdir = os.path.join(tree, "mist", "tracks"), os.path.join(tree, "mist"), os.path.join(tree, "BC", "mist")
    for d in (tdir, bcdir):
        os.makedirs(d)
    bands = ["J", "K", "G", "W1", "V"]
    with rh.memory_hdf() as hdf, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fehs, masses = np.array([-0.5, 0.0, 0.25]), np.array([0.8, 1.0, 1.2, 1.5])
        keys = list(itertools.product(fehs, masses))
        counts = [int(c) for c in rng.integers(20, 34, len(keys))]
        counts[5] = 34                                        # one track reaches the last EEP node
        raw_t = _raw_mist_rows(rng, keys, ("initial_feh", "initial_mass"), counts)

        class Tracks(mm.MISTEvolutionTrackGrid):
            n_eep = max(counts)
            datadir = tdir

            def df_all(self):
                df = raw_t.copy().sort_values(by=list(self.index_cols))
                df.index = [df[c] for c in self.index_cols]
                return df

        Tracks.fehs = fehs
        ages, ifehs = np.array([8.5, 9.0, 9.5, 10.0]), np.array([-0.5, 0.0, 0.25])
        keys = list(itertools.product(ages, ifehs))
        icounts = [int(c) for c in rng.integers(18, 30, len(keys))]
        icounts[4] = 30
        raw_i = _raw_mist_rows(rng, keys, ("log10_isochrone_age_yr", "feh"), icounts)
        raw_i["initial_mass"] = 0.3 + 0.03 * raw_i["EEP"] ** 1.1 + 0.02 * raw_i["feh"]
        raw_i["star_mass"] = raw_i["initial_mass"] * 0.999

        class Isos(mm.MISTIsochroneGrid):
            datadir = idir

            def df_all(self):
                df = raw_i.copy().sort_values(by=list(self.index_cols))
                df.index = [df[c] for c in self.index_cols]
                return df

        lv = (np.array([3500.0, 5000.0, 6500.0, 8000.0]), np.array([2.5, 3.5, 4.0, 5.0]), np.array([-1.0, 0.0, 0.5]),
              np.array([0.0, 0.5, 1.0]), np.array([2.5, 3.1, 4.0]))
        idx = pd.MultiIndex.from_product(lv, names=["Teff", "logg", "[Fe/H]", "Av", "Rv"])

        class BC(mbc.MISTBolometricCorrectionGrid):
            datadir = bcdir

        frames = {}
        for phot, cols in (("UBVRIplus", ["Bessell_B", "Bessell_V", "2MASS_J", "2MASS_Ks", "Gaia_G_DR2Rev", "TESS", "Kepler_Kp"]),
                           ("WISE", ["WISE_W1", "WISE_W2"])):
            # smooth in (Teff, logg, feh, Av), so that magnitudes stay in a sane range
            T, g, f, A, R = (idx.get_level_values(k).to_numpy(float) for k in range(5))
            vals = np.column_stack([0.3 * j - 2.0 * np.log10(T / 5772.0) * (1 + 0.1 * j) + 0.02 * (g - 4.4) + 0.03 * f
                                    - A * (0.3 + 0.1 * j) * (R / 3.1) ** 0.2 + 0.01 * rng.normal(size=len(idx))
                                    for j in range(len(cols))])
            frames[phot] = pd.DataFrame(vals, index=idx, columns=cols)
            hdf.preload(os.path.join(bcdir, "%s.h5" % phot), "df", frames[phot])

        class TrackIC(miso.MIST_EvolutionTrack):
            grid_type, bc_type = Tracks, BC
            eep_bounds = (1, max(counts))

        class IsoIC(miso.MIST_Isochrone):
            grid_type, bc_type = Isos, BC
            eep_bounds = (1, max(icounts))

        out = {}
        for kind, ic_cls in (("track", TrackIC), ("iso", IsoIC)):
            ic = ic_cls(bands=list(bands))
            mg = ic.model_grid
            interp = mg.interp                                 # the reference writes full_grid<tag>.npz here
            if kind == "track":
                age, dt, lengths = mg.get_array_grids()        # ... and array_grid<tag>.npz here
                out.update(track_age_arrays=age, track_dt_deep_arrays=dt, track_lengths=lengths)
            our_mist.export_axes(mg.df, os.path.join(mg.datadir, "full_grid%s_axes.npz" % mg.kwarg_tag))
            n = 400
            if kind == "track":
                pars = np.column_stack([rng.uniform(0.75, 1.55, n), rng.uniform(0.5, 35.0, n), rng.uniform(-0.55, 0.3, n),
                                        rng.uniform(50, 400, n), rng.uniform(-0.05, 1.05, n)])
                pcols = ["Teff", "logg", "feh", "Mbol", "age", "dt_deep", "radius", "nu_max"]
            else:
                pars = np.column_stack([rng.uniform(0.5, 31.0, n), rng.uniform(8.4, 10.05, n), rng.uniform(-0.55, 0.3, n),
                                        rng.uniform(50, 400, n), rng.uniform(-0.05, 1.05, n)])
                pcols = ["Teff", "logg", "feh", "Mbol", "mass", "dm_deep", "radius", "nu_max"]
            mod = sm.SingleStarModel(ic, Teff=(5600, 120), logg=(4.1, 0.2), J=(9.0, 0.05), K=(8.6, 0.05), G=(10.2, 0.02),
                                     parallax=(5.0, 0.2))
            lnprior, lnlike, lnpost = np.empty(n), np.empty(n), np.empty(n)
            with np.errstate(all="ignore"):
                vals = np.asarray(ic.interp_value([pars[:, 0], pars[:, 1], pars[:, 2]], pcols))
                Teff, logg, feh, mags = ic.interp_mag([pars[:, j] for j in range(5)], list(bands))
                for i in range(n):
                    lnprior[i], lnlike[i], lnpost[i] = mod.lnprior(pars[i]), mod.lnlike(pars[i]), mod.lnpost(pars[i])
            cols = [str(c) for c in interp.columns]
            out.update({kind + "_pars": pars, kind + "_interp_value": vals, kind + "_Teff": Teff, kind + "_logg": logg,
                        kind + "_feh": feh, kind + "_mags": mags, kind + "_lnprior": lnprior, kind + "_lnlike": lnlike,
                        kind + "_lnpost": lnpost, kind + "_grid_shape": np.array(interp.grid.shape),
                        kind + "_columns": np.array(cols), kind + "_interp_value_cols": np.array(pcols),
                        kind + "_axis0": interp.index_columns[0], kind + "_axis1": interp.index_columns[1],
                        kind + "_axis2": interp.index_columns[2]})
            print("datadir %s: grid %s, finite lnpost %d / %d" % (kind, interp.grid.shape, np.isfinite(lnpost).sum(), n))
        out["meta"] = json.dumps(dict(bands=bands, obs=dict(Teff=[5600, 120], logg=[4.1, 0.2], J=[9.0, 0.05], K=[8.6, 0.05],
                                                               G=[10.2, 0.02], parallax=[5.0, 0.2]),
                                      track_eep_bounds=[1, max(counts)], iso_eep_bounds=[1, max(icounts)]))
        for phot, fr in frames.items():
            ingest.export_frame_npz(fr, os.path.join(bcdir, phot + ".npz"))
    # the HDF5 stand-in only touched empty placeholder files: they are not part of the fixture
    for dirpath, _, files in os.walk(tree):
        for f in files:
            if not f.endswith(".npz"):
                os.remove(os.path.join(dirpath, f))
    np.savez_compressed(os.path.join(OUT, "datadir.npz"), **out)


def main():
    if "--only-priors" in sys.argv:
        run_prior_cases()
        return
    if "--only-prior-edges" in sys.argv:
        run_prior_edge_cases()
        return
    if "--only-isotrack" in sys.argv:
        run_isotrack_case()
        return
    if "--only-tree" in sys.argv:
        run_tree_cases()
        return
    if "--only-ini" in sys.argv:
        run_ini_cases()
        return
    if "--only-interp-edges" in sys.argv:
        run_interp_edges()
        return
    if "--only-eep" in sys.argv:
        run_eep_case()
        return
    if "--only-ingest" in sys.argv:
        run_ingest_cases()
        return
    if "--only-datadir" in sys.argv:
        run_datadir_case()
        return
    if not rh.reference_available():
        sys.exit("reference tree not found; goldens can only be regenerated in the authoring container")
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240807)
    run_interp_kats(rng)
    trk, iso, bc = small_track(), small_iso(), small_bc()
    np.savez_compressed(os.path.join(OUT, "tables.npz"),
                        track_grid=trk[0], track_ax0=trk[1][0], track_ax1=trk[1][1], track_ax2=trk[1][2],
                        track_columns=np.array(trk[2]),
                        iso_grid=iso[0], iso_ax0=iso[1][0], iso_ax1=iso[1][1], iso_ax2=iso[1][2],
                        iso_columns=np.array(iso[2]),
                        bc_grid=bc[0], bc_ax0=bc[1][0], bc_ax1=bc[1][1], bc_ax2=bc[1][2], bc_ax3=bc[1][3],
                        bc_columns=np.array(bc[2]))
    run_model_case("track_single_spec_phot", "track", 1, "spec_phot_plx", trk, bc, rng, 500, 400)
    run_model_case("track_single_astero", "track", 1, "astero", trk, bc, rng, 150, 150)
    run_model_case("track_single_maxav", "track", 1, "phot_only", trk, bc, rng, 100, 100,
                   extra_kw=dict(maxAV=0.5, max_distance=500.0, halo_fraction=0.05))
    run_model_case("iso_single_spec_phot", "iso", 1, "spec_phot_plx", iso, bc, rng, 400, 300)
    run_model_case("iso_single_spec_only", "iso", 1, "spec_only", iso, bc, rng, 100, 100)
    run_model_case("iso_binary_phot6", "iso", 2, "phot6_plx", iso, bc, rng, 400, 400)
    run_model_case("iso_triple_phot6", "iso", 3, "phot6_plx", iso, bc, rng, 250, 250)
    run_eep_case()
    run_tree_cases()
    run_ini_cases()
    run_isotrack_case()
    run_prior_cases()
    run_ingest_cases()
    run_datadir_case()
    run_prior_edge_cases()
    run_interp_edges()


if __name__ == "__main__":
    main()
