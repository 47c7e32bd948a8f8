#!/usr/bin/env python
"""Timing of the batched on-device EM fit of a binned population and of the bootstrap built on it, JSON lines appended to
profiles/emfit/emfit.jsonl:

* ``iso_emfit_run`` (libiso_emfit.so: k_emfit_run) alone: the C entry on prepared device tables, weights and outputs,
  ``K`` steps with ``tol = -inf`` (``K + 1`` evaluations of all stars), between HIP events, median of ``--reps`` passes
  after warm-up, rotating over distinct tables and weight sets: S = 10^4 and 10^6 stars, B = 8 and 64 cells, R = 1, 64 and
  256 replicates.  Every row carries the seconds per (replicate, evaluation), the bytes of table and weights the
  evaluations read (the table twice: two passes) and what they come to per second: an estimate of what binds the kernel
  from times and counts, not a counter reading.  One replicate is one workgroup, so R = 1 uses one CU of the device;
* alternating with it in the same process, on the same tables, the E-step of the only route there was before:
  ``binfit.moments`` (what ``maximize`` calls once per step: the upload of the row, ``iso_binfit_moments``, the download of
  N), wall clock per call.  ``maximize`` adds ``cell_table``, the M-step on the host and an ``lnlike`` call to every step;
* on the 10^4 x 32 x 100 catalog of tools/binned_timing.py (the 8-bin age histogram and the 8 x 8 grid): ``maximize`` per
  step, wall clock, measured here again, next to ``em_masses`` per (replicate, step) and ``bootstrap`` end to end.

    python tools/emfit_timing.py [--quick] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from binfit_timing import make_table  # noqa: E402  (the tables are that tool's)
from binned_timing import NAMES, grids, interim_priors, timed  # noqa: E402
from hier_timing import make_chain  # noqa: E402

STARS = (10 ** 4, 10 ** 6)
CELLS = (8, 64)
REPLICATES = (1, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 10^3 and 10^5 stars, a short bootstrap")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emfit", "emfit.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _chain, _emfit_cabi as ec, binfit, device as dev, emfit
    if not torch.cuda.is_available():
        raise SystemExit("emfit_timing needs a GPU: a CPU run says nothing about these paths")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a")
    reps = 5 if a.quick else 30
    name = torch.cuda.get_device_name(0)
    device = torch.device("cuda", 0)

    def emit(**row):
        row["device"] = name
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row), flush=True)

    lib = ec.lib()
    stream = dev.stream_ptr(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    for S in STARS:
        if a.quick:
            S //= 10
        big = S >= 10 ** 5
        K = 2 if big else 8
        n_tables, n_sets = (2, 2) if (big or a.quick) else (8, 4)
        for B in CELLS:
            torch.cuda.empty_cache()
            tables = [make_table(S, B, 10 + i) for i in range(n_tables)]
            scale = torch.ones(B, **f64)
            g0 = torch.full((B,), 1.0 / B, **f64)
            lnh = np.zeros((1, B))
            # the earlier route's E-step on the same tables: one call per EM step
            binfit.moments(tables[0], lnh, None, False, device=device)
            walls = []
            for i in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                binfit.moments(tables[i % n_tables], lnh, None, False, device=device)
                walls.append(time.perf_counter() - t0)
            moments_s = float(np.median(walls))
            for R in REPLICATES:
                sets = []
                for k in range(n_sets):
                    w = torch.empty(R, S, **f64)
                    ec.check(lib.iso_emfit_weights(ec.POISSON, 100 + k, 0, R, S, dev.ptr(w), stream))
                    sets.append(w)
                g, obj, wsum = torch.empty(R, B, **f64), torch.empty(R, **f64), torch.empty(R, **f64)
                n_iter, status, live = (torch.empty(R, **i32) for _ in range(3))

                def run(i):
                    ec.check(lib.iso_emfit_run(dev.ptr(tables[i % n_tables]), B, S, dev.ptr(scale), dev.ptr(sets[i % n_sets]), R,
                                               None, dev.ptr(g0), 0, K, float("-inf"), 0, dev.ptr(g), dev.ptr(obj),
                                               dev.ptr(n_iter), dev.ptr(status), dev.ptr(live), dev.ptr(wsum), stream))
                med, best = timed(run, n_tables * n_sets, reps, 2)
                evals = R * (K + 1)
                table_bytes, weight_bytes = 2 * B * S * 8 * evals, S * 8 * evals
                ops = evals * S * (5 * B + 4)                           # two multiplies and an add, a multiply and an add per cell
                emit(path="iso_emfit_run", S=S, B=B, R=R, steps=K, evaluations_per_replicate=K + 1, reps=reps,
                     rotating_tables=n_tables, rotating_weight_sets=n_sets, median_s=med, min_s=best,
                     s_per_replicate_evaluation=med / evals, s_per_batch_evaluation=med / (K + 1),
                     table_bytes=table_bytes, weight_bytes=weight_bytes, bytes_per_s=(table_bytes + weight_bytes) / med,
                     float64_ops=ops, float64_ops_per_s=ops / med, workgroups=R,
                     steps_done=int(n_iter.min().item()), estimate="from times and counts, not a counter reading",
                     binfit_moments_call_s=moments_s, ratio_moments_call_to_replicate_evaluation=moments_s / (med / evals))
                del sets
            del tables

    # -- on the catalog of tools/binned_timing.py -----------------------------------------------------------------------
    S, W, T = (10 ** 3 if a.quick else 10 ** 4), 32, 100
    x = make_chain(S, W, T, 100)
    models = grids()
    for gname in ("age 8", "age 8 x feh 8"):
        model = models[gname]
        pp = ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim_priors())
        pp.bin_tables()
        pp.maximize(max_iter=3, errors=False)                       # warm-up: the libraries, the allocator
        steps = 20 if a.quick else 100
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pp.maximize(max_iter=steps, tol=-np.inf, errors=False)
        torch.cuda.synchronize()
        per_step = (time.perf_counter() - t0) / max(1, fit.n_iter)
        row = dict(path="PopulationPosterior.bootstrap", grid=gname, S=S, W=W, T=T, B=model.n_cells,
                   maximize_steps_timed=int(fit.n_iter), maximize_s_per_step=per_step)
        pp.em_masses(max_iter=3)
        for R in REPLICATES:
            w = emfit.star_weights("poisson", 5, 0, R, S, device).cpu().numpy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, n_it, _, _ = pp.em_masses(weights=w, max_iter=steps, tol=-np.inf)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            row["em_masses_R%d_wall_s" % R] = wall
            row["em_masses_R%d_s_per_replicate_step" % R] = wall / (R * max(1, int(n_it.max())))
        n_boot = 20 if a.quick else 200
        walls, bs = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bs = pp.bootstrap(n_boot=n_boot, seed=1)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        total_steps = int(bs.n_iter.sum())
        row.update(n_boot=n_boot, bootstrap_wall_s=float(np.median(walls)), bootstrap_steps_all_replicates=total_steps,
                   bootstrap_steps_longest_replicate=int(bs.n_iter.max()), bootstrap_s_per_replicate_step=float(np.median(walls)) / max(1, total_steps),
                   same_steps_through_maximize_s=per_step * total_steps,
                   ratio_maximize_route_to_bootstrap=per_step * total_steps / float(np.median(walls)),
                   converged=int((bs.status == ec.CONVERGED).sum()), largest_mass_sd=float(np.nanmax(bs.mass_sd)), reps=3)
        emit(**row)
    out.close()


if __name__ == "__main__":
    main()
