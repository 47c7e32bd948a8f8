#!/usr/bin/env python
"""Timing of the derived stellar properties on one device, JSON lines appended to profiles/derived/derived.jsonl:

* the ``iso_derived_chain`` kernel alone (libiso_derived.so) and ``FusedEnsembleSampler.derived_quantiles`` end to end
  (derived chain + quantile kernel), between HIP events, median of ``--reps`` passes after warm-up, at (S, W, T) =
  (10^4, 32, 100) and (10^4, 300, 100) with the 4 columns radius, Teff, logg, age of the full-size synthetic track table.
  The passes rotate over 8 distinct chains, so that no launch re-reads what the last one left in a cache.  A star's
  walkers are scattered about the star's own point of the table, as a fit leaves them.  The kernel's time is set against
  the bytes it has to move: 3 parameter rows in, 4 derived rows out, 8 bytes each per sample;
* in the same process, on the same chains, the only earlier route to the same numbers: ``ic.interp_value`` on a permuted
  copy of the chain as one device batch, then the framework sort of ``fit_stars_gpu``'s non-fused branch (in slices of
  stars where the whole would not fit);
* ``fit_catalog(derived=True)`` at 10^4 stars beside the same fit without the switch: ``phases["derived_s"]`` and the
  fit's total, at ``fit_stars_gpu``'s default 32 x (150 + 100) and, with ``--fits 32,300``, at the reference's
  300 x (200 + 100).

    python tools/derived_timing.py [--quick] [--skip-kernels] [--fits 32[,300]] [--out FILE]
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

SHAPES = ((10 ** 4, 32, 100), (10 ** 4, 300, 100))
PROPS = ("radius", "Teff", "logg", "age")
ROTATE = 8
PEAK_HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s HBM3E
FITS = {32: dict(nwalkers=32, nburn=150, niter=100), 300: dict(nwalkers=300, nburn=200, niter=100)}


def make_chain(ic, S, W, T, seed):
    """Parameter-major storage [T, 5, S * W] of (mass, eep, feh, distance, AV) on the device: every star has a point of
    its own inside the table and its samples scatter about it by a few percent of an axis."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    fehs, masses, _ = ic.model_grid.interp.index_columns

    def col(lo, hi, width):
        centre = lo + (hi - lo) * (0.1 + 0.8 * torch.rand(S, 1, dtype=torch.float64, device="cuda", generator=g))
        x = centre + width * (hi - lo) * torch.randn(T, S, W, dtype=torch.float64, device="cuda", generator=g)
        return x.clamp_(lo, hi).view(T, S * W)
    x = torch.empty(T, 5, S * W, dtype=torch.float64, device="cuda")
    x[:, 0] = col(0.6, 2.0, 0.01)
    x[:, 1] = col(220.0, 450.0, 0.02)
    x[:, 2] = col(float(fehs[3]), float(fehs[-1]), 0.02)
    x[:, 3] = 100.0
    x[:, 4] = 0.1
    return x


def earlier_route(ic, x, S, W, step):
    """interp_value on the permuted chain as one device batch, then the sort of fit_stars_gpu's non-fused branch."""
    import torch
    T = x.shape[0]
    out = []
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        p = x[:, :3, s0 * W:(s0 + n) * W].permute(1, 0, 2).contiguous().view(3, -1)                  # the permuted copy
        v = ic.interp_value([p[0], p[1], p[2]], list(PROPS))                                         # [T * n * W, Q]
        flat = v.view(T, n, W, len(PROPS)).permute(1, 3, 0, 2).reshape(n, len(PROPS), T * W).contiguous()
        srt = torch.sort(flat, dim=2).values
        m = srt.shape[2]
        pick = torch.tensor([0.5, 0.16, 0.84], dtype=torch.float64, device=flat.device) * (m - 1)
        i0 = pick.floor().long()
        i1 = torch.clamp(i0 + 1, max=m - 1)
        frac = pick - i0.to(torch.float64)
        out.append(srt[:, :, i0] * (1 - frac) + srt[:, :, i1] * frac)
    return torch.cat(out, dim=0)


def device_time(fns, reps, warmup=3):
    """Median and minimum seconds of one call, the calls rotating over ``fns``."""
    import torch
    for i in range(max(warmup, len(fns))):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fns[i % len(fns)]()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e-3, float(np.min(ms)) * 1e-3


class _Holder:
    """What derived_quantiles reads of a sampler, around a chain that no sampler made."""

    def __init__(self, storage, S, W):
        self._chain, self.n_ensembles, self.nwalkers, self._stacked = storage, S, W, True
        self.device, self.device_index = storage.device, storage.device.index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars")
    ap.add_argument("--skip-kernels", action="store_true", help="only the catalog fits")
    ap.add_argument("--fits", default="32", help="walker counts of the catalog fits, of 32 and 300 (empty: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived", "derived.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd.derived import derive_storage
    from isochrones_amd.sampler import FusedEnsembleSampler
    if not torch.cuda.is_available():
        raise SystemExit("derived_timing needs a GPU: a CPU run says nothing about these paths")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a")
    reps, rotate = (5, 2) if a.quick else (30, ROTATE)
    name = torch.cuda.get_device_name(0)

    def emit(**row):
        row["device"] = name
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row), flush=True)

    ic = ia.synthetic_track(bands=("G", "BP", "RP"))
    for S, W, T in (() if a.skip_kernels else SHAPES):
        if a.quick:
            S = 10 ** 3
        chains = [make_chain(ic, S, W, T, 100 + i) for i in range(rotate)]
        n = S * W * T
        nbytes = n * 8 * (3 + len(PROPS))
        shape = dict(S=S, W=W, T=T, columns=list(PROPS), samples=n, rotating_chains=rotate, reps=reps)
        d, nc = derive_storage(chains[0], S, W, ic, PROPS)
        nan_share = float((nc > 0).double().mean().item())
        del d
        med, best = device_time([lambda x=x: derive_storage(x, S, W, ic, PROPS) for x in chains], reps)
        least = nbytes / PEAK_HBM_BYTES_PER_S
        emit(path="iso_derived_chain", median_s=med, min_s=best, samples_per_s=n / med, streamed_bytes=nbytes,
             bytes_per_s=nbytes / med, least_time_bytes_s=least, share_of_hbm_peak=least / med,
             star_columns_with_a_nan=nan_share, **shape)
        holders = [_Holder(x, S, W) for x in chains]
        dq = FusedEnsembleSampler.derived_quantiles
        q_new = dq(holders[0], ic, PROPS)[0]
        med_q, best_q = device_time([lambda h=h: dq(h, ic, PROPS) for h in holders], reps)
        emit(path="derived_quantiles", median_s=med_q, min_s=best_q, stars_per_s=S / med_q, **shape)
        step = max(1, min(S, (1 << 27) // (W * T)))
        q_old = earlier_route(ic, chains[0], S, W, step)
        fin = torch.isfinite(q_old) & torch.isfinite(q_new)
        rel = ((q_old - q_new).abs() / (1 + q_new.abs()))[fin]
        r_old = max(3, reps // 3)
        med_o, best_o = device_time([lambda x=x: earlier_route(ic, x, S, W, step) for x in chains], r_old, warmup=1)
        emit(path="interp_value_and_torch_sort", median_s=med_o, min_s=best_o, stars_per_s=S / med_o, stars_per_slice=step,
             max_scaled_difference_to_derived_quantiles=float(rel.max().item()) if rel.numel() else None,
             same_nan_positions=bool(torch.equal(torch.isnan(q_old), torch.isnan(q_new))),
             speedup_of_derived_quantiles=med_o / med_q, **dict(shape, reps=r_old))
        del chains, holders, q_new, q_old
        torch.cuda.empty_cache()

    # the catalog fit with and without the switch
    n = 1000 if a.quick else 10 ** 4
    fits = [FITS[int(w)] for w in a.fits.split(",") if w]
    if fits:
        cat, _ = ia.synthetic_catalog(ic, n, bands=["G", "BP", "RP"], seed=7, mag_unc=0.01)
    for kw in fits:
        for _ in range(2):                                               # the first pass is the warm-up
            rows = {}
            for flag in (False, True):
                t0 = time.perf_counter()
                df = ia.fit_catalog(cat, ic, derived=flag, **kw)
                torch.cuda.synchronize()
                rows[flag] = (time.perf_counter() - t0, df)
        off, on = rows[False], rows[True]
        ph = on[1].attrs["timings"]["phases"]
        new = [c for c in on[1].columns if c not in off[1].columns]
        emit(path="fit_catalog", stars=n, wall_s_without=off[0], wall_s_with=on[0],
             fit_s_without=off[1].attrs["timings"]["fit_s"], fit_s_with=on[1].attrs["timings"]["fit_s"],
             derived_s=ph["derived_s"], phases_with=ph, phases_without=off[1].attrs["timings"]["phases"],
             derived_columns=new, ok_share=float(on[1]["ok"].mean()),
             finite_share_of_derived_where_ok=float(np.isfinite(on[1].loc[on[1]["ok"] > 0, new].values).mean()), **kw)
    out.close()


if __name__ == "__main__":
    main()
