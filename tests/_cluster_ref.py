"""numpy restatement of the star-cluster likelihood, written from its description ("Star clusters"), and
helpers that rebuild the cluster fixtures of tests/golden/cluster/.  The restatement is the yardstick of the GPU tests at
shapes too large for fixtures; tests/test_cluster_cpu.py pins it to the reference's own numbers."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")
CASES = ("cluster_jhk", "cluster_props", "cluster_holes_phot6")


def _powerlaw_lnpdf(x, a, lo, hi):
    a1 = a + 1.0
    with np.errstate(all="ignore"):
        return np.log(a1 / (hi ** a1 - lo ** a1)) + a * np.log(x)


def _logaddexp(a, b):
    hi = np.where(b > a, b, a)
    with np.errstate(all="ignore"):
        return hi + np.log(np.exp(a - hi) + np.exp(b - hi))


def like_per_star(eeps, mass, ln_dm, mags, prop_model, star_mag, star_unc, star_prop, star_prop_unc, alpha, gamma, fB,
                  mass_lo, mass_hi, minq):
    """like_s of every star for one parameter row.

    eeps, mass, ln_dm [n]: the kept EEPs and their initial mass, ln|dm/dEEP|; mags [n, Nb]; prop_model [n, Np];
    star_mag / star_unc [Ns, Nb]; star_prop / star_prop_unc [Ns, Np]."""
    n, ns = len(eeps), star_mag.shape[0]
    if n < 2:
        return np.zeros(ns)
    with np.errstate(all="ignore"):
        q = mass[None, :] / mass[:, None]                                   # [j, k] = m_k / m_j
        keep = (np.arange(n)[None, :] <= np.arange(n)[:, None]) & ~(q < minq)
        mass_term = _powerlaw_lnpdf(mass, alpha, mass_lo, mass_hi) + ln_dm     # [j]
        ratio = _powerlaw_lnpdf(q, gamma, minq, 1.0)                         # [j, k]
        flux = 10 ** (-0.4 * mags)
        binary = -2.5 * np.log10(flux[:, None, :] + flux[None, :, :])        # [j, k, b]
        ln_fb, ln_1mfb = np.log(fB), np.log(1.0 - fB)
        d = np.diff(eeps)
        out = np.empty(ns)
        for s in range(ns):
            w = 1.0 / star_unc[s] ** 2
            single = ln_1mfb + -0.5 * (mags - star_mag[s]) ** 2 * w            # [j, b]
            lb = ln_fb + -0.5 * (binary - star_mag[s]) ** 2 * w                # [j, k, b]
            phot = np.zeros((n, n))
            for b in range(mags.shape[1]):
                phot = phot + _logaddexp(lb[:, :, b], single[:, None, b])
            prop = np.zeros(n)
            for p in range(prop_model.shape[1]):
                prop = prop + -0.5 * (star_prop[s, p] - prop_model[:, p]) ** 2 / star_prop_unc[s, p] ** 2
            L = phot + mass_term[:, None] + ratio + prop[:, None]
            e = np.where(keep, np.exp(np.where(keep, L, 0.0)), 0.0)
            inner = np.concatenate([[0.0], [np.sum(0.5 * (e[j, :j] + e[j, 1:j + 1]) * d[:j]) for j in range(1, n)]])
            out[s] = np.sum(0.5 * (inner[:-1] + inner[1:]) * d)
        return out


def lnlike_from_likes(like):
    if np.any(like == 0):
        return -np.inf
    with np.errstate(all="ignore"):
        return float(np.sum(np.log(like)))


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    out = {k: d[k] for k in d.files}
    out["meta"] = json.loads(str(out["meta"]))
    return out


def catalog_frame(fx):
    import pandas as pd
    meta = fx["meta"]
    df = pd.DataFrame()
    for b in meta["bands"]:
        df[b + "_mag"] = fx["mag_" + b]
        df[b + "_mag_unc"] = fx["unc_" + b]
    for q in meta["props"]:
        df[q] = fx["prop_" + q]
        df[q + "_unc"] = fx["propunc_" + q]
    return df


def star_arrays(fx):
    meta = fx["meta"]
    mag = np.column_stack([fx["mag_" + b] for b in meta["bands"]])
    unc = np.column_stack([fx["unc_" + b] for b in meta["bands"]])
    ns = mag.shape[0]
    prop = np.column_stack([fx["prop_" + q] for q in meta["props"]]) if meta["props"] else np.zeros((ns, 0))
    punc = np.column_stack([fx["propunc_" + q] for q in meta["props"]]) if meta["props"] else np.zeros((ns, 0))
    return mag, unc, prop, punc


def make_ic(fx):
    """This package's isochrone interpolator over the fixture's tables."""
    from isochrones_amd.interp import DFInterpolator
    from isochrones_amd.models import BolometricCorrectionGrid, IsochroneGrid, IsochroneInterpolator
    meta = fx["meta"]
    bands = [str(b) for b in fx["bc_columns"]]
    bcg = BolometricCorrectionGrid(DFInterpolator.from_arrays(fx["bc_grid"], [fx["bc_ax%d" % i] for i in range(4)], bands),
                                   bands=bands)
    mg = IsochroneGrid(DFInterpolator.from_arrays(fx["model_grid"], [fx["model_ax%d" % i] for i in range(3)],
                                                  meta["model_columns"]),
                       limits={k: tuple(v) for k, v in meta["limits"].items()})
    ax2 = fx["model_ax2"]
    return IsochroneInterpolator(mg, bcg, bands=bands, eep_bounds=(float(ax2[0]), float(ax2[-1])))


def make_model(fx, minq, ic=None, **kw):
    import isochrones_amd as ia
    meta = fx["meta"]
    return ia.StarClusterModel(ic or make_ic(fx), catalog_frame(fx), eep_bounds=tuple(meta["eep_bounds"]), minq=float(minq),
                               bands=meta["bands"], props=meta["props"], **kw)
