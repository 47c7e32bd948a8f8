#!/usr/bin/env python
"""Timing of the population paths on one device, JSON lines into profiles/population/population.jsonl:

* the kernel alone (``iso_population_eval``, every output asked for, binaries) at N = 10^4 and 10^6 systems with 3 and 7
  bands, on the MIST-shaped synthetic track table (18 columns);
* ``evaluate_binaries`` end to end on device tensors (EEP estimate, the launch, the columns gathered into one matrix);
* ``StarPopulation.generate(N)`` split into its parts - draws on the host, EEP estimate, evaluation, DataFrame - and whole;
* beside them, in the same process on the same draws, the only earlier route to these numbers:
  ``ic.generate_binary(..., all_As=True)`` at N = 10^3 and 10^5 (host arrays through pandas, two ``interp_value`` and four
  ``interp_mag`` launches), which does not give the system extinctions.

Device paths: warm-up passes, then HIP events around each of ``--reps`` passes (default 30) that rotate over 8 distinct
input sets, median and minimum reported.  Host-side parts (draws, the frame, ``generate_binary``, ``generate``) are timed
with a host clock after a synchronise; they return host values.

    python tools/population_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = 8
BANDS7 = ("J", "H", "K", "G", "BP", "RP", "V")


def device_time(fn, reps, warmup=3):
    """``fn(k)`` is pass k; it picks input set k mod SETS."""
    import torch
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    ms = []
    for k in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(k)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e-3, float(np.min(ms)) * 1e-3


def host_time(fn, reps):
    import torch
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return float(np.median(s)), float(np.min(s))


def population(ic):
    """The population of the reference's own test (isochrones/tests/test_populations.py), AV within the BC table."""
    import isochrones_amd as ia
    from isochrones_amd import priors
    return ia.StarPopulation(ic, imf=priors.SalpeterPrior(bounds=(0.4, 10)), fB=0.4, gamma=0.3, sfh=ia.StarFormationHistory(),
                             feh=priors.GaussianPrior(-0.2, 0.2), distance=priors.DistancePrior(max_distance=3000),
                             AV=priors.AVPrior(bounds=(0, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, no 10^6 frame")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population", "population.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _population_cabi as pc, device as dev, populations as pp
    if not torch.cuda.is_available():
        raise SystemExit("population_timing needs a GPU: a CPU run says nothing about these paths")
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
    bk = pp._DeviceBackend(0)
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")      # noqa: E731
    cols, packed = pp._packed_columns(ic, "all")

    for n in (10 ** 4, 10 ** 6):
        draws = [pop.draw(n, np.random.default_rng(100 + k)) for k in range(SETS)]
        sets = []
        for mA, mB, age, feh, dist, av in draws:
            tA, tB, tg, tf = up(mA), up(mB), up(age), up(feh)
            e = ic.get_eep(torch.cat([tA, tB]), torch.cat([tg, tg]), torch.cat([tf, tf]))
            sets.append(dict(mA=tA, mB=tB, age=tg, feh=tf, dist=up(dist), av=up(av),
                             coords=torch.stack([tf, tA, e[:n], tf, tB, e[n:]]).contiguous()))
        on_grid = float(torch.isfinite(sets[0]["coords"][2]).double().mean().item())
        for bands in (BANDS7[:3], BANDS7):
            tb = pp.population_tables(ic, packed, bands, bk)
            Q, B = tb.Q, tb.B
            o = [dev.empty_f64(s, 0) for s in ((2, Q, n), (2, B, n), (2, B, n), (B, n), (B, n))]
            po = pc.IsoPopulationOut(*[dev.ptr(t) for t in o])
            fn = pc.lib().iso_population_eval

            def kernel(k, tb=tb, po=po):
                s = sets[k % SETS]
                pc.check(fn(C.byref(tb.model), C.byref(tb.bct), dev.ptr(s["coords"]), dev.ptr(s["dist"]), dev.ptr(s["av"]), n, 2,
                            C.byref(po), dev.stream_ptr(0)))

            med, best = device_time(kernel, reps)
            emit(path="kernel", n=n, bands=B, columns=Q, reps=reps, median_s=med, min_s=best, systems_per_s=n / med,
                 primaries_on_grid=on_grid, bytes_written=(2 * Q + 6 * B) * n * 8)

            def end_to_end(k, bands=bands):
                s = sets[k % SETS]
                return ia.evaluate_binaries(ic, s["mA"], s["mB"], s["age"], s["feh"], s["dist"], s["av"], bands=bands)

            med, best = device_time(end_to_end, reps)
            emit(path="evaluate_binaries", n=n, bands=B, columns=Q, reps=reps, median_s=med, min_s=best, systems_per_s=n / med)
        del sets, o
        torch.cuda.empty_cache()

    # generate(N), part by part on one round of draws, and whole; generate_binary on the same draws
    host_reps = 3 if a.quick else 7
    for n in (10 ** 3, 10 ** 5) + (() if a.quick else (10 ** 6,)):
        d_s, _ = host_time(lambda: pop.draw(n, np.random.default_rng(7)), host_reps)
        mA, mB, age, feh, dist, av = pop.draw(n, np.random.default_rng(7))
        tA, tB, tg, tf, td, ta = (up(v) for v in (mA, mB, age, feh, dist, av))
        m2, g2, f2 = torch.cat([tA, tB]), torch.cat([tg, tg]), torch.cat([tf, tf])
        eep_s, _ = device_time(lambda k: ic.get_eep(m2, g2, f2), reps)
        e = ic.get_eep(m2, g2, f2)
        eeps = (e[:n].contiguous(), e[n:].contiguous())
        ev_s, _ = device_time(lambda k: pp._evaluate(ic, tA, tB, tg, tf, td, ta, None, "all", False, eeps, bk), reps)
        res = pp._evaluate(ic, tA, tB, tg, tf, td, ta, None, "all", False, eeps, bk)
        fr_s, _ = host_time(res.frame, host_reps)
        whole_s, _ = host_time(lambda: pop.generate(n, seed=7), host_reps)
        loose_s, _ = host_time(lambda: pop.generate(n, seed=7, exact_N=False), host_reps)
        emit(path="generate", n=n, bands=7, draws_s=d_s, eep_s=eep_s, evaluate_s=ev_s, frame_s=fr_s, generate_exact_n_s=whole_s,
             generate_one_round_s=loose_s, reference_documented_s_per_1000=1.24)
        if n <= 10 ** 5:
            old_s, _ = host_time(lambda: ic.generate_binary(mA, mB, age, feh, distance=dist, AV=av, all_As=True), host_reps)
            emit(path="generate_binary_all_As", n=n, bands=7, seconds=old_s, new_route_s=eep_s + ev_s + fr_s,
                 ratio=old_s / (eep_s + ev_s + fr_s), note="same draws; the earlier route has no system A_<band>")
    out.close()


if __name__ == "__main__":
    main()
