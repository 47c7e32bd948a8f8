#!/usr/bin/env python
"""Timing of the posterior-predictive check on one device, JSON lines appended to profiles/predictive/predictive.jsonl:

* the ``iso_predict_chain`` kernel alone (libiso_predict.so) and ``FusedEnsembleSampler.predictive`` end to end (kernel +
  quantile kernel on the magnitude chain), between HIP events, median of ``--reps`` passes after warm-up, at (S, W, T) =
  (10^4, 32, 100) and (10^4, 300, 100) with the 3 bands G, BP, RP of the full-size synthetic track table.  The passes rotate
  over 8 distinct chains, so that no launch re-reads what the last one left in a cache.  A star's walkers are scattered
  about the star's own point of the table, as a fit leaves them.  The kernel's time is set against the bytes it has to
  stream: 5 parameter rows and 1 lnprob row in, 3 magnitude rows out, 8 bytes each per sample;
* in the same process, on the same chains, the only earlier route to the same numbers: the chain permuted to rows, through
  ``ic.interp_mag`` as one device batch, then framework ops for the residuals, the means, the argmax and the sort (in slices
  of stars where the whole would not fit);
* ``fit_catalog(predictive=True)`` at 10^4 stars beside the same fit without the switch: ``phases["predictive_s"]`` and the
  fit's total, at ``fit_stars_gpu``'s default 32 x (150 + 100) and, with ``--fits 32,300``, at the reference's
  300 x (200 + 100).

    python tools/predictive_timing.py [--quick] [--skip-kernels] [--fits 32[,300]] [--out FILE]
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
BANDS = ("G", "BP", "RP")
ROTATE = 8
PEAK_HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s HBM3E
FITS = {32: dict(nwalkers=32, nburn=150, niter=100), 300: dict(nwalkers=300, nburn=200, niter=100)}


def make_chain(ic, S, W, T, seed):
    """Parameter-major storage [T, 5, S * W] of (mass, eep, feh, distance, AV) and lnprob [T, S * W] on the device: every
    star has a point of its own inside the table and its samples scatter about it by a few percent of an axis."""
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
    x[:, 3] = col(80.0, 400.0, 0.01)
    x[:, 4] = col(0.0, 0.5, 0.02)
    lnp = -0.5 * torch.randn(T, S * W, dtype=torch.float64, device="cuda", generator=g) ** 2
    return x, lnp


def make_obs(S, seed=5):
    """Observations [S, B + 4] of plausible size (the timing does not depend on their values); Teff and parallax present."""
    rng = np.random.default_rng(seed)
    B = len(BANDS)
    val = np.full((S, B + 4), np.nan)
    unc = np.full((S, B + 4), np.nan)
    val[:, :B], unc[:, :B] = rng.uniform(8.0, 14.0, (S, B)), 0.02
    val[:, B], unc[:, B] = rng.uniform(4500.0, 6500.0, S), 100.0
    val[:, B + 3], unc[:, B + 3] = rng.uniform(2.0, 12.0, S), 0.1
    return val, unc


def earlier_route(ic, x, lnp, val, unc, S, W, step):
    """The chain permuted to rows, interp_mag as one device batch, then framework ops: residuals and their means per term,
    their mean over the terms, the argmax of lnprob with its parameters, and the sort for the magnitude quantiles."""
    import torch
    T, B = x.shape[0], len(BANDS)
    ppc, quant, mpars = [], [], []
    pick_q = torch.tensor([0.5, 0.16, 0.84], dtype=torch.float64, device=x.device)
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        p = x[:, :, s0 * W:(s0 + n) * W].permute(1, 0, 2).contiguous().view(5, -1)                   # the permuted copy
        teff, logg, feh, mags = ic.interp_mag_device(p, list(BANDS))                                 # [N], [N, B]
        model = torch.cat([mags, teff[:, None], logg[:, None], feh[:, None], (1000.0 / p[3])[:, None]], dim=1)
        model = model.view(T, n, W, B + 4)
        v, u = val[s0:s0 + n, None, :], unc[s0:s0 + n, None, :]
        z = (v - model) ** 2 / u ** 2                                                                # [T, n, W, B + 4]
        present = ~torch.isnan(val[s0:s0 + n])
        good = torch.isfinite(torch.where(present[None, :, None, :], model, torch.zeros_like(model))).all(dim=3)
        zg = torch.where(good[..., None], z, torch.zeros_like(z))
        means = zg.sum(dim=(0, 2)) / good.sum(dim=(0, 2))[:, None].to(torch.float64)                 # [n, B + 4]
        means = torch.where(present, means, torch.full_like(means, float("nan")))
        ppc.append(torch.nansum(means, dim=1) / present.sum(dim=1))
        lp = lnp[:, s0 * W:(s0 + n) * W].view(T, n, W).permute(1, 0, 2).reshape(n, T * W)
        best = torch.argmax(torch.nan_to_num(lp, nan=float("-inf")), dim=1)
        rows = x[:, :, s0 * W:(s0 + n) * W].view(T, 5, n, W).permute(2, 0, 3, 1).reshape(n, T * W, 5)
        mpars.append(rows[torch.arange(n, device=x.device), best])
        flat = mags.view(T, n, W, B).permute(1, 3, 0, 2).reshape(n, B, T * W).contiguous()
        srt = torch.sort(flat, dim=2).values
        m = srt.shape[2]
        pick = pick_q * (m - 1)
        i0 = pick.floor().long()
        i1 = torch.clamp(i0 + 1, max=m - 1)
        frac = pick - i0.to(torch.float64)
        quant.append(srt[:, :, i0] * (1 - frac) + srt[:, :, i1] * frac)
    return torch.cat(ppc), torch.cat(quant), torch.cat(mpars)


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
    """What FusedEnsembleSampler.predictive reads of a sampler, around a chain that no sampler made."""

    def __init__(self, storage, lnp, S, W):
        self._chain, self._lnprob, self.n_ensembles, self.nwalkers, self._stacked = storage, lnp, S, W, True
        self.ndim = int(storage.shape[1])
        self.device, self.device_index = storage.device, storage.device.index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars")
    ap.add_argument("--skip-kernels", action="store_true", help="only the catalog fits")
    ap.add_argument("--fits", default="32", help="walker counts of the catalog fits, of 32 and 300 (empty: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive", "predictive.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import predictive as pv
    from isochrones_amd.sampler import FusedEnsembleSampler
    if not torch.cuda.is_available():
        raise SystemExit("predictive_timing needs a GPU: a CPU run says nothing about these paths")
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

    ic = ia.synthetic_track(bands=BANDS)
    B = len(BANDS)
    for S, W, T in (() if a.skip_kernels else SHAPES):
        if a.quick:
            S = 10 ** 3
        chains = [make_chain(ic, S, W, T, 100 + i) for i in range(rotate)]
        hval, hunc = make_obs(S)
        dobs = pv.DeviceObs(hval, hunc, 0)
        n = S * W * T
        nbytes = n * 8 * (5 + 1 + B)
        shape = dict(S=S, W=W, T=T, bands=list(BANDS), samples=n, rotating_chains=rotate, reps=reps)
        r0 = pv.predict_storage(chains[0][0], chains[0][1], S, W, ic, BANDS, dobs)
        bad_share = float(r0.n_bad.double().sum().item()) / n
        del r0
        med, best = device_time([lambda c=c: pv.predict_storage(c[0], c[1], S, W, ic, BANDS, dobs) for c in chains], reps)
        least = nbytes / PEAK_HBM_BYTES_PER_S
        emit(path="iso_predict_chain", median_s=med, min_s=best, samples_per_s=n / med, streamed_bytes=nbytes,
             bytes_per_s=nbytes / med, least_time_bytes_s=least, share_of_hbm_peak=least / med, bad_sample_share=bad_share,
             **shape)
        holders = [_Holder(c[0], c[1], S, W) for c in chains]
        sp = FusedEnsembleSampler.predictive
        new = sp(holders[0], ic, dobs, bands=BANDS)
        med_q, best_q = device_time([lambda h=h: sp(h, ic, dobs, bands=BANDS) for h in holders], reps)
        emit(path="sampler.predictive", median_s=med_q, min_s=best_q, stars_per_s=S / med_q, samples_per_s=n / med_q, **shape)
        step = max(1, min(S, (1 << 26) // (W * T)))
        ppc_o, q_o, mp_o = earlier_route(ic, chains[0][0], chains[0][1], dobs.val, dobs.unc, S, W, step)
        fin = torch.isfinite(ppc_o) & torch.isfinite(new["ppc"])
        rel = ((ppc_o - new["ppc"]).abs() / new["ppc"].abs())[fin]
        finq = torch.isfinite(q_o) & torch.isfinite(new["mag_quantiles"])
        relq = ((q_o - new["mag_quantiles"]).abs() / (1 + new["mag_quantiles"].abs()))[finq]
        r_old = max(3, reps // 3)
        med_o, best_o = device_time([lambda c=c: earlier_route(ic, c[0], c[1], dobs.val, dobs.unc, S, W, step) for c in chains],
                                    r_old, warmup=1)
        emit(path="interp_mag_and_framework_ops", median_s=med_o, min_s=best_o, stars_per_s=S / med_o, stars_per_slice=step,
             max_relative_difference_of_ppc=float(rel.max().item()) if rel.numel() else None,
             max_scaled_difference_of_mag_quantiles=float(relq.max().item()) if relq.numel() else None,
             same_map_pars=bool(torch.equal(mp_o, new["map_pars"])),
             speedup_of_sampler_predictive=med_o / med_q, **dict(shape, reps=r_old))
        del chains, holders, new, ppc_o, q_o, mp_o
        torch.cuda.empty_cache()

    # the catalog fit with and without the switch
    n = 1000 if a.quick else 10 ** 4
    fits = [FITS[int(w)] for w in a.fits.split(",") if w]
    if fits:
        cat, _ = ia.synthetic_catalog(ic, n, bands=list(BANDS), seed=7, mag_unc=0.01)
    for kw in fits:
        for _ in range(2):                                               # the first pass is the warm-up
            rows = {}
            for flag in (False, True):
                t0 = time.perf_counter()
                df = ia.fit_catalog(cat, ic, predictive=flag, **kw)
                torch.cuda.synchronize()
                rows[flag] = (time.perf_counter() - t0, df)
        off, on = rows[False], rows[True]
        ph = on[1].attrs["timings"]["phases"]
        new = [c for c in on[1].columns if c not in off[1].columns]
        emit(path="fit_catalog", stars=n, wall_s_without=off[0], wall_s_with=on[0],
             fit_s_without=off[1].attrs["timings"]["fit_s"], fit_s_with=on[1].attrs["timings"]["fit_s"],
             predictive_s=ph["predictive_s"], phases_with=ph, phases_without=off[1].attrs["timings"]["phases"],
             predictive_columns=new, ok_share=float(on[1]["ok"].mean()),
             median_ppc_where_ok=float(np.nanmedian(on[1].loc[on[1]["ok"] > 0, "ppc"].values)), **kw)
    out.close()


if __name__ == "__main__":
    main()
