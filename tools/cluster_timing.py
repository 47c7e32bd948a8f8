#!/usr/bin/env python
"""Timing of StarClusterModel on one device: JSON lines with the shape (stars, bands, valid EEPs, rows), the kernels' time
(HIP events around iso_cluster_lnlike), the end-to-end lnpost time, star-pairs per second and the ratio to an f64
issue-bound estimate.

The estimate: ~50 f64 VALU operations per star-pair and band (residual, Gaussian term, logaddexp with one exp and one log,
the binary magnitude amortised over the star tile) plus the exp of the cell, against 4e13 f64 vector operations per
second for the whole MI355X (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz x ~2.5).  ``ratio`` = estimate / measured kernel
time: 1 would be issue-bound at that rate.

    python tools/cluster_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_PAIR_BAND = 50.0
F64_OPS_PER_S = 4e13
NOTEBOOK = [8.84, -0.2, 500.0, 0.03, -3.0, 0.3, 0.3]


def _model(n_stars, seed, bands="gri", minq=0.5):
    import isochrones_amd as ia
    ic = ia.synthetic_isochrone(bands=tuple(bands))
    cat = ia.simulate_cluster(n_stars, *NOTEBOOK, bands=bands, ic=ic, seed=seed)
    cols = ["%s_mag" % b for b in bands]
    df = cat.df[np.isfinite(cat.df[cols].to_numpy()).all(axis=1)]
    return ia.StarClusterModel(ic, df, bands=list(bands), props=["parallax"], eep_bounds=(200, 700), minq=minq)


def _valid_eeps(mod, rows):
    lo, hi = mod.bounds("eep")
    E = np.arange(lo, hi + 1).astype(float)
    out = []
    for p in rows:
        m = np.asarray(mod.ic.interp_value([E, p[0] * np.ones(E.size), p[1] * np.ones(E.size)], ["initial_mass"]),
                       dtype=float).reshape(-1)
        out.append(int(np.isfinite(m).sum()))
    return out


def time_case(name, mod, rows, reps):
    import torch
    rows = np.asarray(rows, dtype=float)
    single = rows.shape[0] == 1
    arg = rows[0] if single else rows
    mod.lnpost(arg)                                   # warm-up: uploads, tables, first launches
    torch.cuda.synchronize()
    wall = []
    kern = []
    for _ in range(reps):
        mod._kernel_events = []
        t0 = time.perf_counter()
        mod.lnpost(arg)                               # returns host values: synchronised
        wall.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        kern.append(sum(a.elapsed_time(b) for a, b in mod._kernel_events) * 1e-3)
    mod._kernel_events = None
    nv = _valid_eeps(mod, rows[:min(len(rows), 8)])
    n_valid = float(np.mean(nv))
    ns, nb = len(mod.stars), len(mod.bands)
    pairs = ns * n_valid * (n_valid + 1) / 2 * rows.shape[0]
    k = float(np.median(kern))
    est = pairs * (OPS_PER_PAIR_BAND * nb + 20.0) / F64_OPS_PER_S
    return dict(case=name, stars=ns, bands=nb, valid_eeps=n_valid, rows=int(rows.shape[0]), reps=reps,
                kernel_s=k, lnpost_s=float(np.median(wall)), lnpost_min_s=float(np.min(wall)),
                star_pairs=pairs, star_pairs_per_s=pairs / k, estimate_s=est, ratio_estimate_over_kernel=est / k,
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, no fit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else sys.stdout
    reps = 3 if a.quick else 20
    rng = np.random.default_rng(0)
    nb = _model(50, seed=1)
    for name, rows in (("notebook_1row", np.array([NOTEBOOK])),
                       ("notebook_1024rows", np.array(NOTEBOOK) + np.array([0.02, 0.03, 5.0, 0.01, 0.2, 0.05, 0.05])
                        * rng.standard_normal((1024, 7)))):
        out.write(json.dumps(time_case(name, nb, rows, reps if rows.shape[0] == 1 else max(3, reps // 4))) + "\n")
        out.flush()
    big = _model(500, seed=2)
    rows = np.array(NOTEBOOK) + np.array([0.02, 0.03, 5.0, 0.01, 0.2, 0.05, 0.05]) * rng.standard_normal((256, 7))
    out.write(json.dumps(time_case("stars500_256rows", big, rows, 3)) + "\n")
    out.flush()
    if not a.quick:
        import isochrones_amd as ia
        truth = [9.0, 0.0, 500.0, 0.1, -2.5, 0.3, 0.3]
        ic = ia.synthetic_isochrone(bands=("J", "H", "K"))
        cat = ia.simulate_cluster(30, *truth, bands="JHK", mass_range=(0.4, 1.1), ic=ic, seed=7)   # EEPs ~300-680 at 1 Gyr
        df = cat.df[np.isfinite(cat.df[["J_mag", "H_mag", "K_mag"]].to_numpy()).all(axis=1)]
        mod = ia.StarClusterModel(ic, df, bands=["J", "H", "K"], props=["parallax"], eep_bounds=(200, 700),
                                  max_distance=2000)
        t0 = time.perf_counter()
        res = mod.fit_multinest(n_live_points=300, seed=3)
        dt = time.perf_counter() - t0
        s = mod.samples
        q = {k: [float(v) for v in np.quantile(s[k], [0.025, 0.5, 0.975])] for k in ("age", "feh", "distance")}
        out.write(json.dumps(dict(case="fit_multinest_30stars", stars=len(df), bands=3, n_live_points=300, seconds=dt,
                                  lnpost_evaluations=int(res.ncall), niter=int(res.niter), logz=float(res.logz),
                                  truth=truth, quantiles_2p5_50_97p5=q, device=torch.cuda.get_device_name(0))) + "\n")
        out.flush()


if __name__ == "__main__":
    main()
