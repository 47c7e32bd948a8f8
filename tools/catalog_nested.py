"""Timing driver of the catalog nested sampler: seconds and stars/s of fit_stars_nested_gpu by phase, the proposal efficiency
over the catalog, and the yardstick - the per-star host loop catalog.model(i, ic).fit_multinest(...) - in the same session.

    python tools/catalog_nested.py [--stars 1250 10000] [--live 400 1000] [--passes 5] [--yardstick 100] [--out FILE]

Appends one JSON line per (stars, live points) to profiles/nested/catalog_nested.jsonl (or --out).  Phases are the ones
fit_stars_nested_gpu's ``timings`` separate with a device synchronisation: build (per-star blocks), sampling (the ONE kernel
launch: fill and macro-steps are inside it and are not timed apart) and copy-out.  A last line lists registers / scratch /
waves of every kernel of the library from the build's resources JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, nargs="+", default=[1250, 10000])
    ap.add_argument("--live", type=int, nargs="+", default=[400, 1000])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--yardstick", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nested",
                                                  "catalog_nested.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd.catalog import fit_stars_nested_gpu, nested_result_columns
    from isochrones_amd.csrc.libraries import NESTED
    bands = ["G", "BP", "RP"]
    ic = ia.synthetic_track(bands=bands)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    table = NESTED.resource_table()
    res = table["k_catalog_nested<0, 1, 3>"]
    cols = nested_result_columns(ic.param_names)
    i_ncall, i_niter, i_err = cols.index("ncall"), cols.index("niter"), cols.index("lnZ_err")
    for live in a.live:
        yard = None
        for n in a.stars:
            cat, _ = ia.synthetic_catalog(ic, n, bands=bands, seed=0, mag_unc=0.02, with_parallax=True)
            idx = np.arange(n)
            fit_stars_nested_gpu(cat, ic, idx, n_live_points=live, seed=0)          # warm-up pass
            total, phases, rows = [], [], None
            for _ in range(a.passes):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = fit_stars_nested_gpu(cat, ic, idx, n_live_points=live, seed=0, timings=tm)
                torch.cuda.synchronize()
                total.append(time.perf_counter() - t0)
                phases.append(tm)
            if yard is None and a.yardstick:
                m = min(a.yardstick, n)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(m):
                    cat.model(i, ic).fit_multinest(n_live_points=live)
                yard = m / (time.perf_counter() - t0)
            ok = rows[:, -1] == 1
            eff = rows[ok, i_ncall] / np.maximum(rows[ok, i_niter], 1)
            sec = float(np.median(total))
            line = dict(stars=n, n_live_points=live, passes=a.passes, seconds=sec, stars_per_s=n / sec,
                        phases_s={k: float(np.median([p.get(k, 0.0) for p in phases])) for k in ("build_posteriors", "sampling", "summaries")},
                        ok_fraction=float(ok.mean()), ncall_per_niter=dict(zip(("p05", "p50", "p95", "max"), map(float, list(np.percentile(eff, [5, 50, 95])) + [eff.max()]))),
                        niter_median=float(np.median(rows[ok, i_niter])), lnZ_err_median=float(np.median(rows[ok, i_err])),
                        yardstick_fit_multinest_stars_per_s=yard, speedup=(n / sec) / yard if yard else None,
                        kernel="k_catalog_nested<0, 1, 3>", resources=res, device=torch.cuda.get_device_name(0))
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    with open(a.out, "a") as f:
        f.write(json.dumps(dict(resources_of_every_kernel=table)) + "\n")


if __name__ == "__main__":
    main()
