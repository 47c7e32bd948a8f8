#!/usr/bin/env python
"""Timing of the maximum-likelihood fit of a binned population on one device, JSON lines appended to
profiles/binfit/binfit.jsonl:

* ``iso_binfit_moments`` (libiso_binfit.so: k_binfit_partial + k_binfit_total) alone: the C entry on prepared device tables,
  rows, outputs and workspace, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct
  tables: S = 10^4 and 10^6 stars, B = 8 and 64 cells, H = 1 and 64 hyper rows, with and without the pair sums.  Every row
  carries the bytes of table the call reads and the multiplies and adds of its owner walks, and what they come to per
  second: an estimate of what binds k_binfit_partial from times and counts, not a counter reading;
* alternating with it pass by pass in the same process, on the same tables, the only route to the first moment there was
  before: per hyper row ``iso_binned_lnlike`` for the row's ``ell``, ``iso_shrink_cells`` for the stars' cell probabilities,
  and their sum over the stars through a framework op (what ``star_bin_probabilities(theta[h:h + 1])`` runs), 10
  alternating passes (3 with ``--quick``), fewer than the 30 of the entry alone: the rows say so in ``reps``;
* ``PopulationPosterior.maximize`` end to end on the 10^4 x 32 x 100 catalog of tools/binned_timing.py: the 8-bin age
  histogram, next to ``fit_mcmc`` at its defaults on the same posterior, and the 8 x 8 grid of [Fe/H] bins per age bin,
  whose 63 logits ``fit_mcmc``'s 64 default walkers cannot sample (an affine-invariant ensemble needs at least twice as
  many walkers as dimensions), so no such fit is timed.  Steps, seconds per step and in all, wall clock, the tables built
  before the clock starts.

    python tools/binfit_timing.py [--quick] [--out FILE]
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

from binned_timing import NAMES, grids, interim_priors, timed  # noqa: E402  (the catalog and the protocol are that tool's)
from hier_timing import ROTATE, make_chain  # noqa: E402

STARS = (10 ** 4, 10 ** 6)
CELLS = (8, 64)
ROWS = (1, 64)


def make_table(S, B, seed):
    """A [B, S] on the device as a compression leaves it: a star's weight spread over a few neighbouring cells, zero in
    the others."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    centre = torch.rand(1, S, dtype=torch.float64, device="cuda", generator=g) * B
    width = 0.5 + 2.0 * torch.rand(1, S, dtype=torch.float64, device="cuda", generator=g)
    b = torch.arange(B, dtype=torch.float64, device="cuda")[:, None] + 0.5
    A = torch.exp(-0.5 * ((b - centre) / width) ** 2) * 100.0
    return torch.where(A < 1e-3, torch.zeros_like(A), A).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating tables, 10^3 and 10^5 stars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binfit", "binfit.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _binfit_cabi as fc, _binned_cabi as bc, _chain, _shrink_cabi as sc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("binfit_timing needs a GPU: a CPU run says nothing about these paths")
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

    flib, blib, slib = fc.lib(), bc.lib(), sc.lib()
    stream = dev.stream_ptr(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    for S in STARS:
        if a.quick:
            S //= 10
        for B in CELLS:
            torch.cuda.empty_cache()
            tables = [make_table(S, B, 10 + i) for i in range(rotate)]
            squares = [t * t for t in tables]
            mx = torch.zeros(S, **f64)
            for H in ROWS:
                rng = np.random.default_rng(H + B)
                lnh = torch.from_numpy(rng.normal(0.0, 1.0, (H, B))).cuda()
                N, Cm = torch.empty(H, B, **f64), torch.empty(H, B, B, **f64)
                live = torch.empty(H, dtype=torch.int32, device="cuda")
                shape = dict(S=S, B=B, H=H, rotating_tables=rotate, reps=reps)
                med_first = None
                for pairs in (False, True):
                    ws = torch.empty(int(flib.iso_binfit_workspace_doubles(B, S, H, int(pairs))), **f64)

                    def moments(i, pairs=pairs, ws=ws):
                        fc.check(flib.iso_binfit_moments(dev.ptr(tables[i]), B, S, dev.ptr(lnh), H, None, dev.ptr(N),
                                                         dev.ptr(Cm) if pairs else None, dev.ptr(live), dev.ptr(ws), stream))
                    med, best = timed(moments, rotate, reps, rotate)
                    if not pairs:
                        med_first, first = med, moments
                    # what the partial kernel moves and computes: the table once per row; per (row, star) the staging (B
                    # multiplies, B adds, B divisions), the owners' B adds and, with pairs, B (B + 1) / 2 multiplies and adds;
                    # through LDS per (row, star) the staging write, the read for s1, the read and write of the division
                    # and the count owners' read (5 B doubles) and, with pairs, six 8-byte reads per block of 3 x 3 cells
                    n_pairs = B * (B + 1) // 2 if pairs else 0
                    groups = (B + 2) // 3
                    n_blocks = groups * (groups + 1) // 2 if pairs else 0
                    table_bytes = H * B * S * 8
                    ops = H * S * (4 * B + 2 * n_pairs)
                    lds_bytes = H * S * 8 * (6 * n_blocks + 5 * B)
                    emit(path="iso_binfit_moments", pairs=pairs, median_s=med, min_s=best, table_bytes=table_bytes,
                         table_bytes_per_s=table_bytes / med, float64_ops=ops, float64_ops_per_s=ops / med, lds_bytes=lds_bytes,
                         lds_bytes_per_s=lds_bytes / med, workgroups=H * ((S + fc.CHUNK - 1) // fc.CHUNK),
                         workspace_bytes=ws.numel() * 8, estimate="from times and counts, not a counter reading",
                         live=int(live[0].item()), **shape)
                # the earlier route to the first moment, a row at a time, alternating with the new one
                ell, ess = torch.empty(1, S, **f64), torch.empty(1, S, **f64)
                lnG, cellp = torch.empty(B, S, **f64), torch.empty(B, S, **f64)
                N_old = torch.empty(H, B, **f64)

                def earlier(i):
                    for h in range(H):
                        row = dev.ptr(lnh[h:h + 1])
                        bc.check(blib.iso_binned_lnlike(dev.ptr(tables[i]), dev.ptr(squares[i]), dev.ptr(mx), B, S, 0, S, 1, row, 1,
                                                        None, dev.ptr(ell), dev.ptr(ess), None, None, stream))
                        sc.check(slib.iso_shrink_cells(dev.ptr(tables[i]), dev.ptr(mx), B, S, 0, S, row, dev.ptr(ell), 1, None,
                                                       dev.ptr(lnG), dev.ptr(cellp), stream))
                        N_old[h] = torch.nansum(cellp, dim=1)
                r_alt = 3 if a.quick else 10
                earlier(0)
                torch.cuda.synchronize()
                ms_old, ms_new = [], []
                for i in range(r_alt):
                    for f, ms in ((earlier, ms_old), (first, ms_new)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f(i % rotate)
                        e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                earlier(0)
                ws = torch.empty(int(flib.iso_binfit_workspace_doubles(B, S, H, 0)), **f64)
                fc.check(flib.iso_binfit_moments(dev.ptr(tables[0]), B, S, dev.ptr(lnh), H, None, dev.ptr(N), None, dev.ptr(live),
                                                 dev.ptr(ws), stream))
                diff = float(((N - N_old).abs().max() / max(1, int(live.max().item()))).item())
                med_o, med_n = float(np.median(ms_old)) * 1e-3, float(np.median(ms_new)) * 1e-3
                emit(path="iso_binned_lnlike + iso_shrink_cells per row + framework sum over the stars", median_s=med_o,
                     iso_binfit_moments_alongside_median_s=med_n, speedup_of_iso_binfit_moments=med_o / med_n,
                     iso_binfit_moments_alone_median_s=med_first, max_difference_of_N_over_n_live=diff, **dict(shape, reps=r_alt))
            del tables, squares

    # -- maximize end to end on the catalog of tools/binned_timing.py ------------------------------------------------
    S, W, T = (10 ** 3 if a.quick else 10 ** 4), 32, 100
    x = make_chain(S, W, T, 100)
    models = grids()
    for gname in ("age 8", "age 8 x feh 8"):
        model = models[gname]
        pp = ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim_priors())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pp.bin_tables()
        torch.cuda.synchronize()
        t_tables = time.perf_counter() - t0
        pp.maximize(max_iter=3)                                     # warm-up: the libraries, the allocator
        walls, fit = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = pp.maximize()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        wall = float(np.median(walls))
        t0 = time.perf_counter()
        pp.maximize(max_iter=fit.n_iter, errors=False)
        torch.cuda.synchronize()
        wall_no_errors = time.perf_counter() - t0
        row = dict(path="PopulationPosterior.maximize", grid=gname, S=S, W=W, T=T, B=model.n_cells, logits=model.n_params,
                   steps=fit.n_iter, converged=bool(fit.converged), wall_s=wall, s_per_step=wall / max(1, fit.n_iter),
                   wall_s_without_errors=wall_no_errors, bin_tables_s=t_tables, lnlike=fit.lnlike,
                   rise_over_the_start=float(fit.lnlike - fit.trace[0]), on_bound=list(fit.on_bound),
                   largest_mass_sd=float(np.nanmax(fit.mass_sd)), reps=3)
        if gname == "age 8":
            nb, ni = (20, 20) if a.quick else (200, 200)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp.fit_mcmc(nwalkers=64, nburn=nb, niter=ni, seed=3)
            torch.cuda.synchronize()
            # the hyper-prior is flat on the logits, so lnprior is one number inside the ranges: taken at maximize()'s theta it
            # is the best sample's as well, and lnprob minus it is that sample's lnlike
            row.update(fit_mcmc_wall_s=time.perf_counter() - t0, fit_mcmc="64 walkers x (%d + %d), tables built before" % (nb, ni),
                       fit_mcmc_best_lnprob_minus_lnprior=float(pp.sampler.flatlnprobability.max().item()
                                                                - pp.lnprior(fit.theta[None])[0]))
        else:
            row.update(fit_mcmc="not timed: 64 default walkers are fewer than twice the 63 logits")
        emit(**row)
    out.close()


if __name__ == "__main__":
    main()
