#!/usr/bin/env python
"""Timing of the draws on one device, JSON lines into profiles/draw/draw.jsonl:

* ``iso_draw_systems`` alone (the C entry on a preallocated tensor; the seven columns of
  ``StarPopulation.generate(rng="philox")``) and ``plan.draw`` around it at N = 10^4, 10^5 and 10^6, between HIP events;
* ``StarPopulation.generate(N, as_tensors=True)`` by part - draws, EEP estimate, evaluation - for ``rng="numpy"`` (the draws
  on the host with their upload) and ``rng="philox"`` at N = 10^3, 10^5 and 10^6, and whole (one round, ``exact_N=False``);
* ``InjectionSet.draw`` at 10^6 (``--quick``: 10^5), both ways;
* the largest device-against-host-entry difference of the seven columns at N = 10^5.

Everything runs in one process; the two ways alternate pass by pass, ``--reps`` passes each (default 30), median and minimum
reported.  The kernel is timed between HIP events, the legs with a host clock after a synchronise.

    python tools/draw_timing.py [--quick] [--out FILE]
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

BANDS7 = ("J", "H", "K", "G", "BP", "RP", "V")


def population(ic):
    """The population of tools/population_timing.py (the reference's own test, AV within the BC table)."""
    import isochrones_amd as ia
    from isochrones_amd import priors
    return ia.StarPopulation(ic, imf=priors.SalpeterPrior(bounds=(0.4, 10)), fB=0.4, gamma=0.3, sfh=ia.StarFormationHistory(),
                             feh=priors.GaussianPrior(-0.2, 0.2), distance=priors.DistancePrior(max_distance=3000),
                             AV=priors.AVPrior(bounds=(0, 1)))


def alternate(fns, reps, clock):
    """``{name: (median, minimum)}`` of the passes of every ``fns[name](k)``, taken in turn pass by pass."""
    for k in range(3):
        for fn in fns.values():
            fn(k)
    seen = {name: [] for name in fns}
    for k in range(reps):
        for name, fn in fns.items():
            seen[name].append(clock(fn, k))
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in seen.items()}


def event_clock(fn, k):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def wall_clock(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, nothing at 10^6 but the kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw", "draw.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _draw_cabi as dc, device as dev, populations as pp, priors as P
    if not torch.cuda.is_available():
        raise SystemExit("draw_timing needs a GPU: a CPU run says nothing about these paths")
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

    ic = ia.synthetic_track(bands=BANDS7)
    pop = population(ic)
    plan = pop.draw_plan()
    bk = pp._DeviceBackend(0)
    C_ = len(plan.device_columns)

    lib = dc.lib()
    for n in (10 ** 4, 10 ** 5, 10 ** 6):
        x = torch.empty((C_, n), dtype=torch.float64, device="cuda")

        def entry(k, n=n, x=x):                                  # the C entry alone, on a tensor that exists
            dc.check(lib.iso_draw_systems(plan.records.ctypes.data, C_, plan.order.ctypes.data, None, 0, 100 + k % 8, 0, 0, None, n,
                                          dev.ptr(x), dev.stream_ptr(0)))

        t = alternate({"entry": entry, "plan": lambda k, n=n: plan.draw(n, 100 + k % 8, device=0)}, reps, event_clock)
        for path, key in (("iso_draw_systems", "entry"), ("plan.draw", "plan")):
            emit(path=path, n=n, columns=C_, reps=reps, median_s=t[key][0], min_s=t[key][1], systems_per_s=n / t[key][0],
                 bytes_written=C_ * n * 8, gb_per_s=C_ * n * 8 / t[key][0] * 1e-9,
                 note="the C entry on a preallocated tensor" if key == "entry" else "the output tensor's allocation and the Python call included")
        del x

    host = plan.draw(10 ** 5, 3)
    got = plan.draw(10 ** 5, 3, device=0)
    worst = max(float(np.max(np.abs(got[c].cpu().numpy() - host[c]) / np.maximum(1.0, np.abs(host[c])))) for c in plan.device_columns)
    emit(path="device_against_host_entry", n=10 ** 5, columns=C_, max_relative_difference=worst)

    up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")      # noqa: E731

    def numpy_draws(k, n):
        return [up(v) for v in pop.draw(n, np.random.default_rng(7 + k))]

    def philox_draws(k, n):
        d = plan.draw(n, 7 + k, device=0)
        return [d["mass"], d["q"] * d["mass"] * (d["binary"] < pop.fB), d["age"], d["feh"], d["distance"], d["AV"]]

    for n in (10 ** 3, 10 ** 5) + (() if a.quick else (10 ** 6,)):
        legs = alternate({"numpy": lambda k, n=n: numpy_draws(k, n), "philox": lambda k, n=n: philox_draws(k, n)}, reps, wall_clock)
        tA, tB, tg, tf, td, ta = philox_draws(0, n)
        m2, g2, f2 = torch.cat([tA, tB]), torch.cat([tg, tg]), torch.cat([tf, tf])
        eep = alternate({"eep": lambda k: ic.get_eep(m2, g2, f2)}, reps, event_clock)["eep"]
        e = ic.get_eep(m2, g2, f2)
        eeps = (e[:n].contiguous(), e[n:].contiguous())
        ev = alternate({"ev": lambda k: pp._evaluate(ic, tA, tB, tg, tf, td, ta, None, "all", False, eeps, bk)}, reps, event_clock)["ev"]
        whole = alternate({"numpy": lambda k, n=n: pop.generate(n, seed=7 + k, exact_N=False, as_tensors=True),
                           "philox": lambda k, n=n: pop.generate(n, seed=7 + k, exact_N=False, as_tensors=True, rng="philox")},
                          reps, wall_clock)
        emit(path="generate", n=n, bands=7, reps=reps, draws_numpy_s=legs["numpy"][0], draws_philox_s=legs["philox"][0],
             draws_ratio=legs["numpy"][0] / legs["philox"][0], eep_s=eep[0], evaluate_s=ev[0],
             generate_numpy_s=whole["numpy"][0], generate_philox_s=whole["philox"][0],
             generate_ratio=whole["numpy"][0] / whole["philox"][0])

    n = 10 ** 5 if a.quick else 10 ** 6
    draw = {"mass": P.SalpeterPrior(bounds=(0.4, 10)), "age": P.AgePrior((8.0, 10.0)), "feh": P.GaussianPrior(-0.2, 0.2),
            "distance": P.DistancePrior(3000), "AV": P.AVPrior((0, 1))}
    limits = {"V": (14.0, 0.2)}
    inj = alternate({"numpy": lambda k: ia.InjectionSet.draw(ic, draw, n, limits, seed=k, accurate=False),
                     "philox": lambda k: ia.InjectionSet.draw(ic, draw, n, limits, seed=k, accurate=False, rng="philox")},
                    reps, wall_clock)
    emit(path="InjectionSet.draw", n=n, reps=reps, numpy_s=inj["numpy"][0], philox_s=inj["philox"][0], ratio=inj["numpy"][0] / inj["philox"][0])
    out.close()


if __name__ == "__main__":
    main()
