#!/usr/bin/env python
"""Timing of the (mass, age, [Fe/H]) -> EEP paths on one device, JSON lines into profiles/solve/eep_solve.jsonl:

* ``solve_eep`` (libiso_solve.so, exact) on 10^4, 10^5 and 10^6 random triples, on the MIST-shaped synthetic track and
  isochrone tables, device tensors in and out;
* the fast ``get_eep`` estimate on the same batches (track table: the only parametrisation that has one);
* ``get_eep(host_array, accurate=True)`` - one Nelder-Mead per star, the only earlier way to these numbers - on 256 of
  the same triples, in the same process.

Device paths: warm-up passes, then HIP events around each of ``--reps`` passes, median and minimum reported.  The
per-star loop is timed once with a host clock (it returns host values, so it has waited for the device).

    python tools/eep_solve_timing.py [--quick] [--out FILE]
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

SIZES = (10 ** 4, 10 ** 5, 10 ** 6)
LOOP_STARS = 256


def triples(kind, n, rng):
    """(mass, age, feh) with a solution on most rows: stars between 0.7 and 3 solar masses, 0.1 to 6 Gyr for the track
    table; for the isochrone table the mass is read off an isochrone so that it lies on it."""
    feh = rng.uniform(-1.0, 0.4, n)
    if kind == "track":
        return rng.uniform(0.7, 3.0, n), rng.uniform(8.0, 9.8, n), feh
    age = rng.uniform(8.0, 10.0, n)
    return rng.uniform(0.3, 1.0, n), age, feh


def device_time(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e-3, float(np.min(ms)) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, 32 stars in the per-star loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve", "eep_solve.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    if not torch.cuda.is_available():
        raise SystemExit("eep_solve_timing needs a GPU: a CPU run says nothing about these paths")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")
    reps = 5 if a.quick else 30
    name = torch.cuda.get_device_name(0)

    def emit(**row):
        row["device"] = name
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row))

    rng = np.random.default_rng(2024)
    ics = dict(track=ia.synthetic_track(bands=("J", "H", "K")), iso=ia.synthetic_isochrone(bands=("J", "H", "K")))
    for kind, ic in ics.items():
        for n in SIZES:
            m, g, f = triples(kind, n, rng)
            tm, tg, tf = (torch.as_tensor(v, device="cuda") for v in (m, g, f))
            res = ic.solve_eep(tm, tg, tf)
            solved = int(torch.isfinite(res).sum().item())
            med, best = device_time(lambda: ic.solve_eep(tm, tg, tf), reps)
            emit(path="solve_eep", table=kind, n=n, reps=reps, solved=solved, median_s=med, min_s=best,
                 triples_per_s=n / med)
            if kind == "track":
                med, best = device_time(lambda: ic.get_eep(tm, tg, tf), reps)
                emit(path="get_eep_fast", table=kind, n=n, reps=reps, median_s=med, min_s=best, triples_per_s=n / med)
            if n == SIZES[0] and kind == "track":
                k = 32 if a.quick else LOOP_STARS
                ic.get_eep(m[:2], g[:2], f[:2], accurate=True, return_nan=True)          # warm-up
                t0 = time.perf_counter()
                loop = ic.get_eep(m[:k], g[:k], f[:k], accurate=True, return_nan=True)
                dt = time.perf_counter() - t0
                exact = res[:k].cpu().numpy()
                both = np.isfinite(loop) & np.isfinite(exact)
                emit(path="get_eep_accurate_loop", table=kind, n=k, seconds=dt, s_per_star=dt / k,
                     converged=int(np.isfinite(loop).sum()),
                     max_abs_eep_difference_to_solve=float(np.max(np.abs(loop[both] - exact[both]))) if both.any() else None)
    out.close()


if __name__ == "__main__":
    main()
