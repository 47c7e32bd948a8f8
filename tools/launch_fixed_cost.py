#!/usr/bin/env python
"""The fixed part of one launch of the headline kernel (cfg 2: k_lnpost_fast<0, 1, 1, false, false>).

Times the kernel on rotating `prior_valid` batches of several sizes through iso_time_lnpost_rotating (HIP events on the
launch stream, as bench.py does) and fits t = a + b n over the sizes: the slope b is what a sample costs in bytes moved,
the intercept a is what a launch costs besides - axis staging and first parameter loads before any table byte is asked
for, the drain of the last waves, the gap between two launches of the stream.  The sizes are visited in turn, `--rounds`
times, so that clock and thermal drift hit all of them alike.

    python tools/launch_fixed_cost.py [--label parent] [--out profiles/launch_ends/parent.jsonl]

Batch b of size n is the first n rows of bench.make_samples(default_rng(12345 + b), max n, "prior_valid"): at n = 10^6
exactly bench.py's batches.  One JSON line on stdout (appended to --out when given)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (250_000, 500_000, 1_000_000, 2_000_000, 4_000_000)


def fit_line(ns, ts):
    """Least squares t = a + b n; returns (a, b, largest residual)."""
    A = np.column_stack([np.ones(len(ns)), np.asarray(ns, dtype=float)])
    (a, b), *_ = np.linalg.lstsq(A, np.asarray(ts, dtype=float), rcond=None)
    return float(a), float(b), float(np.max(np.abs(A @ np.array([a, b]) - ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200, help="launches per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings per size")
    ap.add_argument("--warmup", type=int, default=40)
    args = ap.parse_args()
    sizes = sorted(int(s) for s in args.sizes.split(","))

    import torch
    import bench
    from isochrones_amd import device as dev
    ic, mod = bench.build_model()
    full = [bench.make_samples(np.random.default_rng(12345 + b), sizes[-1], "prior_valid") for b in range(args.batches)]
    mod.lnpost(full[0][:4096])                           # packs the tables outside the timed launches
    rots = {n: bench.Rotation(mod.handle(0), [f[:n] for f in full], dev.stream_ptr(0)) for n in sizes}
    del full
    for n in sizes:
        rots[n].run(args.warmup)
    us = {n: [] for n in sizes}
    for _ in range(args.rounds):
        for n in sizes:
            us[n].append(rots[n].run(args.reps) * 1e3)
    med = [float(np.median(us[n])) for n in sizes]
    a, b, resid = fit_line(sizes, med)
    # the same line through the lowest timing of every size: what the launch costs when nothing disturbs it
    a_min, b_min, _ = fit_line(sizes, [min(us[n]) for n in sizes])
    rec = {"label": args.label, "kernel": "k_lnpost_fast<0, 1, 1, false, false>", "workload": "prior_valid",
           "device": torch.cuda.get_device_name(0), "batches": args.batches, "reps": args.reps, "rounds": args.rounds,
           "sizes": sizes, "us_per_launch": {str(n): us[n] for n in sizes}, "us_median": dict(zip(map(str, sizes), med)),
           "intercept_us": a, "slope_ns_per_sample": b * 1e3, "slope_bytes_per_sample_at_8TBs": b * 1e-6 * 8e12,
           "largest_residual_us": resid, "intercept_us_of_minima": a_min, "slope_ns_per_sample_of_minima": b_min * 1e3}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
