#!/usr/bin/env python
"""Timing of the per-star chain diagnostics on one device, JSON lines appended to
profiles/diagnostics/chain_diagnostics.jsonl:

* the ``iso_diag_chain`` kernel alone (libiso_diag.so) between HIP events, median of ``--reps`` passes after warm-up, at
  (S, W, T, D) = (10^4, 300, 100, 5), (1 250, 300, 100, 5), (10^4, 32, 100, 5) and (1, 256, 5000, 5), max_lag = 1024.
  The passes rotate over 8 distinct chains, so that no launch re-reads what the last one left in a cache.  Each row
  sets the time against the chain's bytes and against the S D W sum_k (T - k) float64 multiply-adds of the definition;
* in the same process, the same statistics from framework ops on the device (``torch.fft`` autocovariances plus
  reductions), on the same chains;
* the numpy twin (tests/_diag_twin.py) on 16 of the stars, host clock;
* ``fit_catalog(diagnostics=True)`` at 10^4 stars beside the same fit without the switch: ``phases["diag_s"]`` and the
  fit's total, at ``fit_stars_gpu``'s default 32 x (150 + 100) and at the reference's 300 x (200 + 100).

    python tools/chain_diagnostics_timing.py [--quick] [--skip-kernels] [--out FILE]
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

SHAPES = ((10 ** 4, 300, 100, 5), (1250, 300, 100, 5), (10 ** 4, 32, 100, 5), (1, 256, 5000, 5))
MAX_LAG = 1024
ROTATE = 8
TWIN_STARS = 16
PEAK_HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s HBM3E
PEAK_F64_FMA_PER_S = 78.6e12 / 2       # MI355X: 78.6 TFLOP/s float64 vector = 39.3e12 multiply-adds per second


def make_chain(S, W, T, D, seed):
    """Parameter-major storage [T, D, S * W] on the device: AR(1) series, a different coefficient per parameter."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    phi = torch.tensor([0.3, 0.6, 0.8, 0.0, 0.5], dtype=torch.float64, device="cuda")[:D].view(D, 1)
    x = torch.empty(T, D, S * W, dtype=torch.float64, device="cuda")
    x[0] = torch.randn(D, S * W, dtype=torch.float64, device="cuda", generator=g)
    amp = torch.sqrt(1 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + amp * torch.randn(D, S * W, dtype=torch.float64, device="cuda", generator=g)
    return x


def torch_diagnostics(x, S, W, c=5.0, max_lag=MAX_LAG):
    """The same five numbers from framework ops: FFT autocovariances pooled over walkers, a cumulative sum, reductions."""
    import torch
    T, D = x.shape[0], x.shape[1]
    K = min(T - 1, max_lag)
    v = x.view(T, D, S, W)
    y = v - v.mean(dim=0, keepdim=True)
    f = torch.fft.rfft(y, n=2 * T, dim=0)
    A = torch.fft.irfft(f.real * f.real + f.imag * f.imag, n=2 * T, dim=0)[: K + 1].sum(dim=3)          # [K + 1, D, S]
    rho = A / A[0]
    tau_m = 1 + 2 * (torch.cumsum(rho, dim=0) - rho[0])
    hit = torch.arange(K + 1, device=x.device, dtype=torch.float64).view(-1, 1, 1) >= c * tau_m
    ok = hit.any(dim=0)
    m = torch.where(ok, hit.to(torch.int8).argmax(dim=0), torch.full_like(ok, K, dtype=torch.int64))
    tau = tau_m.gather(0, m[None])[0]
    n = T // 2
    ch = torch.cat([v[:n], v[T - n:]], dim=3)                                                          # [n, D, S, 2 W]
    mu = ch.mean(dim=0)
    Wv = ch.var(dim=0, unbiased=True).mean(dim=2)
    B = n * mu.var(dim=2, unbiased=True)
    rhat = torch.sqrt(((n - 1) / n * Wv + B / n) / Wv)
    return torch.stack([tau, m.to(torch.float64), ok.to(torch.float64), W * T / tau, rhat], dim=-1).permute(1, 0, 2)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars in the catalog fit")
    ap.add_argument("--skip-kernels", action="store_true", help="only the catalog fits")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics", "chain_diagnostics.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd.diagnostics import diag_storage
    from tests import _diag_twin as tw
    if not torch.cuda.is_available():
        raise SystemExit("chain_diagnostics_timing needs a GPU: a CPU run says nothing about these paths")
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

    for S, W, T, D in (() if a.skip_kernels else SHAPES):
        chains = [make_chain(S, W, T, D, 100 + i) for i in range(rotate)]
        K = min(T - 1, MAX_LAG)
        nbytes = S * W * T * D * 8
        fma = S * D * W * sum(T - k for k in range(K + 1))
        shape = dict(S=S, W=W, T=T, D=D, max_lag=MAX_LAG, chain_bytes=nbytes, f64_multiply_adds=fma,
                     rotating_chains=rotate, reps=reps)
        res = diag_storage(chains[0], S, W, 5.0, MAX_LAG)
        med, best = device_time([lambda x=x: diag_storage(x, S, W, 5.0, MAX_LAG) for x in chains], reps)
        t_bytes, t_fma = nbytes / PEAK_HBM_BYTES_PER_S, fma / PEAK_F64_FMA_PER_S
        emit(path="iso_diag_chain", median_s=med, min_s=best, pairs_per_s=S * D / med, bytes_per_s=nbytes / med,
             f64_multiply_adds_per_s=fma / med, least_time_bytes_s=t_bytes, least_time_multiply_adds_s=t_fma,
             bound="multiply-adds" if t_fma > t_bytes else "bytes", share_of_bound=max(t_bytes, t_fma) / med,
             window_ok_share=float(res[..., 2].mean().item()), **shape)
        # framework ops on the same chains; the FFT workspace is several times the chain, so the largest shape runs in
        # slices of stars that are timed together
        step = max(1, min(S, (1 << 28) // (W * T * D)))

        def torch_pass(x):
            v = x.view(T, D, S, W)
            return [torch_diagnostics(v[:, :, s0:s0 + step].reshape(T, D, -1), min(step, S - s0), W)
                    for s0 in range(0, S, step)]
        ref = torch.cat(torch_pass(chains[0]), dim=0)
        same = (ref[..., 1] == res[..., 1])
        rel = ((ref[..., 0] - res[..., 0]).abs() / res[..., 0].abs())[same]
        med_t, best_t = device_time([lambda x=x: torch_pass(x) for x in chains], max(3, reps // 3), warmup=1)
        emit(path="torch_ops", median_s=med_t, min_s=best_t, pairs_per_s=S * D / med_t, stars_per_slice=step,
             same_window_share=float(same.double().mean().item()),
             max_rel_tau_difference_where_same_window=float(rel.max().item()) if rel.numel() else None,
             **dict(shape, reps=max(3, reps // 3)))
        k = min(S, TWIN_STARS)
        host = chains[0].view(T, D, S, W)[:, :, :k].reshape(T, D, k * W).cpu().numpy()
        t0 = time.perf_counter()
        twin = tw.storage_diagnostics(host, k, W, 5.0, MAX_LAG)
        dt = time.perf_counter() - t0
        got = res[:k].cpu().numpy()
        emit(path="numpy_twin", stars=k, seconds=dt, s_per_pair=dt / (k * D), pairs_per_s=k * D / dt,
             max_rel_tau_difference_to_kernel=float(np.nanmax(np.abs(got[..., 0] - twin[..., 0]) / np.abs(twin[..., 0]))),
             windows_equal=bool(np.array_equal(got[..., 1], twin[..., 1])), **shape)
        del chains, res, ref
        torch.cuda.empty_cache()

    # the catalog fit with and without the switch
    n = 1000 if a.quick else 10 ** 4
    ic = ia.synthetic_track(bands=("G", "BP", "RP"))
    cat, _ = ia.synthetic_catalog(ic, n, bands=["G", "BP", "RP"], seed=7, mag_unc=0.01)
    for kw in (dict(nwalkers=32, nburn=150, niter=100), dict(nwalkers=300, nburn=200, niter=100)):
        for _ in range(2):                                               # the first pass is the warm-up
            rows = {}
            for flag in (False, True):
                t0 = time.perf_counter()
                df = ia.fit_catalog(cat, ic, diagnostics=flag, **kw)
                torch.cuda.synchronize()
                rows[flag] = (time.perf_counter() - t0, df)
        off, on = rows[False], rows[True]
        ph = on[1].attrs["timings"]["phases"]
        emit(path="fit_catalog", stars=n, wall_s_without=off[0], wall_s_with=on[0],
             fit_s_without=off[1].attrs["timings"]["fit_s"], fit_s_with=on[1].attrs["timings"]["fit_s"], diag_s=ph["diag_s"],
             phases_with=ph, phases_without=off[1].attrs["timings"]["phases"],
             window_ok_share=float(np.nanmean(on[1]["window_ok"])), median_tau_max=float(np.nanmedian(on[1]["tau_max"])),
             median_rhat_max=float(np.nanmedian(on[1]["rhat_max"])), **kw)
    out.close()


if __name__ == "__main__":
    main()
