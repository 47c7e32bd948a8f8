#!/usr/bin/env python
"""Timing of the binned population likelihood on one device, JSON lines appended to profiles/binned/binned.jsonl:

* ``iso_binned_compress`` (libiso_binned.so: k_binned_compress), once per (catalog, grid): the C entry on prepared device
  records, edges and outputs, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct chains
  (and ``PopulationPosterior.bin_tables()``, which allocates the tables and uploads the records and edges around it):
  10^4 stars x 32 walkers x 100 steps and 10^4 x 300 x 100, three columns (mass: Chabrier interim, power-law population; feh: FehPrior interim; age: flat-in-age
  interim), for an 8-bin and a 32-bin age histogram ([Fe/H] a fixed Gaussian) and an 8 x 8 grid of [Fe/H] bins per age bin;
* ``iso_binned_lnlike`` (k_binned_rows + k_binned_total) on the tables, kernels alone, and ``PopulationPosterior.lnlike``
  end to end (numpy rows in, numpy ln L out: cell_table on the host, the upload, the kernels, the download), H = 64 and
  1 024 hyper rows;
* alternating with the kernels pass by pass in the same process, on the same chains, the only route there was before: per
  hyper row B rows of ``iso_hier_lnlike`` on the FLAT records of the cells, then ``logsumexp`` over the cells through
  framework ops, 3 passes.  Up to 512 FLAT rows a pass (64 on the large catalog) it is timed in full: H = 64 with 8 bins
  on the small catalog.  Beyond that, where H * B rows take from seconds to minutes a pass, it is timed on the first
  ``mixture_hyper_rows`` hyper rows and ``median_s`` is scaled to H (its cost is linear in the number of row tiles); such a
  row has ``scaled_to_H`` true and its ratio is an extrapolation;
* the compression of 10^6 injections (three columns, the 8-bin age grid) as one ensemble and in ensembles of 4 096, wall
  clock of the calls with their downloads;
* ``fit_mcmc`` of the 8-bin age histogram, 64 walkers x (200 + 200), wall clock, on the small catalog.

    python tools/binned_timing.py [--quick] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hier_timing import ROTATE, make_chain  # noqa: E402  (the chains and the protocol are that tool's)

#          S,       W,   T
SHAPES = ((10 ** 4, 32, 100), (10 ** 4, 300, 100))
ROWS = (64, 1024)
NAMES = ("mass", "feh", "age")                                     # make_chain's columns
AGE, FEH = (8.8, 10.1), (-1.0, 0.4)                                # make_chain's ranges of the two


def grids():
    """name -> (model, cells as (age bin, feh bin or None))"""
    import isochrones_amd as ia
    from isochrones_amd import priors as P
    mass = ia.Fixed(P.PowerLawPrior(-2.35, (0.1, 10.0)))
    feh = ia.Fixed(P.GaussianPrior(-0.2, 0.3, bounds=(-4.0, 0.5)))
    out = {}
    for K in (8, 32):
        out["age %d" % K] = ia.PopulationModel(mass=mass, feh=feh, age=ia.Histogram(np.linspace(*AGE, K + 1)))
    out["age 8 x feh 8"] = ia.PopulationModel(mass=mass, feh=ia.Histogram(np.linspace(*FEH, 9), given="age"),
                                              age=ia.Histogram(np.linspace(*AGE, 9)))
    return out


def interim_priors():
    from isochrones_amd import priors as P
    return {"mass": P.ChabrierPrior(), "feh": P.FehPrior(bounds=(-4.0, 0.5)), "age": P.AgePrior((5.0, 10.15))}


def flat_rows(model, n_hyper):
    """The earlier route's records [n_hyper * B, 3]: per cell the FLAT records of its bins next to the frozen records (the
    same for every hyper row), and ln(cell volume) [B]."""
    import isochrones_amd as ia
    from isochrones_amd import priors as P
    grid = model.bin_grid()
    (a0, e0) = grid["axes"][0], grid["edges"][0]
    second = len(grid["axes"]) == 2
    e1 = grid["edges"][1] if second else np.array([0.0, 1.0])
    rows, lnvol = [], []
    for k0 in range(len(e0) - 1):
        for k1 in range(len(e1) - 1):
            rec = grid["frozen"].copy()
            rec[a0] = ia.hierarchical.prior_record(P.FlatPrior((e0[k0], e0[k0 + 1])))[0]
            vol = e0[k0 + 1] - e0[k0]
            if second:
                rec[grid["axes"][1]] = ia.hierarchical.prior_record(P.FlatPrior((e1[k1], e1[k1 + 1])))[0]
                vol *= e1[k1 + 1] - e1[k1]
            rows.append(rec)
            lnvol.append(np.log(vol))
    return np.tile(np.stack(rows), (n_hyper, 1)), np.array(lnvol)


def timed(f, n_chains, reps, warm):
    """Median and minimum seconds of ``f(chain number)`` between HIP events."""
    import torch
    for i in range(warm):
        f(i % n_chains)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f(i % n_chains)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e-3, float(np.min(ms)) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars, a short fit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binned", "binned.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _binned_cabi as bc, _cabi, _chain, _hier_cabi as hc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("binned_timing needs a GPU: a CPU run says nothing about these paths")
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

    blib, hlib = bc.lib(), hc.lib()
    interim = interim_priors()
    stream = dev.stream_ptr(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    for n_shape, (S, W, T) in enumerate(SHAPES):
        if a.quick:
            S = 10 ** 3
        torch.cuda.empty_cache()
        chains = [make_chain(S, W, T, 100 + i) for i in range(rotate)]
        M = W * T
        for gname, model in grids().items():
            B = model.n_cells
            posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim) for x in chains]
            assert all(p.storage.data_ptr() == x.data_ptr() for p, x in zip(posts, chains))       # read where it lies
            shape = dict(S=S, W=W, T=T, grid=gname, B=B, columns=list(NAMES), rotating_chains=rotate, reps=reps)

            grid = model.bin_grid()
            i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
            g_axes, g_bins, g_frozen = i32(grid["axes"]), i32([len(e) - 1 for e in grid["edges"]]), i32(grid["frozen_cols"])
            d_interim = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
            d_frozen = torch.from_numpy(grid["frozen"].view(np.uint8).copy()).cuda()
            d_edges = torch.from_numpy(np.concatenate(grid["edges"])).cuda()
            cA, cA2, cmx = torch.empty(B, S, **f64), torch.empty(B, S, **f64), torch.empty(S, **f64)
            cbad, cout = torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty(S, dtype=torch.int32, device="cuda")

            def compress(i):
                bc.check(blib.iso_binned_compress(posts[i]._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                                  dev.ptr(d_interim), dev.ptr(d_frozen), len(grid["frozen_cols"]), g_frozen,
                                                  len(grid["axes"]), g_axes, g_bins, dev.ptr(d_edges), None, None, dev.ptr(cA),
                                                  dev.ptr(cA2), dev.ptr(cmx), dev.ptr(cbad), dev.ptr(cout), stream))
            med, best = timed(compress, rotate, reps, rotate)
            emit(path="iso_binned_compress", median_s=med, min_s=best, samples_per_s=S * M / med, chain_bytes_per_s=S * M * 24 / med,
                 bad_samples=int(cbad.sum().item()), out_samples=int(cout.sum().item()), **shape)

            def tables_anew(i):
                posts[i]._tables = None
                posts[i].bin_tables()
            med, best = timed(tables_anew, rotate, reps, rotate)
            emit(path="PopulationPosterior.bin_tables", median_s=med, min_s=best, **shape)
            tables = [p.bin_tables() for p in posts]
            irec = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
            for H in ROWS:
                rng = np.random.default_rng(H)
                theta = rng.uniform(-2.0, 2.0, (H, model.n_params))
                lnh_host = model.cell_table(theta)["lnh"]
                lnh = torch.from_numpy(lnh_host).cuda()
                ell, ess, L, mn = torch.empty(H, S, **f64), torch.empty(H, S, **f64), torch.empty(H, **f64), torch.empty(H, **f64)

                def rows(i):
                    tA, tA2, tmx = tables[i][:3]
                    bc.check(blib.iso_binned_lnlike(dev.ptr(tA), dev.ptr(tA2), dev.ptr(tmx), B, S, 0, S, M, dev.ptr(lnh), H, None,
                                                    dev.ptr(ell), dev.ptr(ess), dev.ptr(L), dev.ptr(mn), stream))
                med, best = timed(rows, rotate, reps, rotate)
                rows(0)
                L_binned = L.clone()
                out_bytes = 2 * H * S * 8
                emit(path="iso_binned_lnlike", H=H, median_s=med, min_s=best, rows_per_s=H / med,
                     output_bytes=out_bytes, output_bytes_per_s=out_bytes / med, table_bytes=2 * B * S * 8,
                     min_ess_median=float(mn.median().item()), **shape)
                med_e, best_e = timed(lambda i: posts[i].lnlike(theta), rotate, reps, rotate)
                emit(path="PopulationPosterior.lnlike", H=H, median_s=med_e, min_s=best_e, rows_per_s=H / med_e, **shape)
                # the earlier route on the first hyper rows
                h_mix = max(1, min(H, (64 if n_shape else 512) // B))
                rec, lnvol = flat_rows(model, h_mix)
                drec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1)).cuda()
                R = rec.shape[0]
                mell, mess = torch.empty(R, S, **f64), torch.empty(R, S, **f64)
                mbad = torch.empty(S, dtype=torch.int32, device="cuda")
                lnhv = (lnh[:h_mix] + torch.from_numpy(lnvol).cuda())[:, :, None]
                L_mix = torch.empty(h_mix, **f64)

                def mixture(i):
                    hc.check(hlib.iso_hier_lnlike(posts[i]._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                                  dev.ptr(irec), dev.ptr(drec), R, None, dev.ptr(mell), dev.ptr(mess), dev.ptr(mbad),
                                                  None, None, stream))
                    L_mix.copy_(torch.logsumexp(mell.view(h_mix, B, S) + lnhv, dim=1).sum(dim=1))
                r_mix = 3
                ms_mix, ms_bin = [], []
                mixture(0)
                torch.cuda.synchronize()
                for i in range(r_mix):                      # alternating, pass by pass, on the pass's chain
                    for f, ms in ((mixture, ms_mix), (rows, ms_bin)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f(i % rotate)
                        e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                mixture(0)
                scaled = ((L_mix - L_binned[:h_mix]).abs() / (1 + L_binned[:h_mix].abs())).max().item()
                med_m, med_b = float(np.median(ms_mix)) * 1e-3, float(np.median(ms_bin)) * 1e-3
                emit(path="iso_hier_lnlike on B FLAT rows per hyper row + logsumexp", H=H, mixture_hyper_rows=h_mix, flat_rows=R,
                     measured_median_s=med_m, median_s=med_m * H / h_mix, scaled_to_H=h_mix < H,
                     iso_binned_lnlike_alongside_median_s=med_b, speedup_of_iso_binned_lnlike=med_m * H / h_mix / med_b,
                     max_scaled_difference_of_L=scaled, **dict(shape, reps=r_mix))
                del mell, mess, ell, ess
            if n_shape == 0 and gname == "age 8":
                nb, ni = (20, 20) if a.quick else (200, 200)
                posts[0]._tables = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                posts[0].fit_mcmc(nwalkers=64, nburn=nb, niter=ni, seed=3)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                emit(path="fit_mcmc", walkers=64, nburn=nb, niter=ni, wall_s=dt, lnpost_calls=2 * (nb + ni),
                     s_per_lnpost_call=dt / (2 * (nb + ni)), includes_compression=True,
                     mean_lnprob=float(posts[0].sampler.flatlnprobability.mean().item()), **shape)
            if n_shape == 0 and gname == "age 8":
                from isochrones_amd.binned import BinnedSelection
                from isochrones_amd import priors as P
                J = 10 ** 5 if a.quick else 10 ** 6
                draw = {"mass": P.PowerLawPrior(-2.35, (0.3, 3.0)), "feh": P.FlatPrior((-1.0, 0.4)), "age": P.FlatPrior((8.8, 10.1))}
                rng = np.random.default_rng(7)
                inj = ia.InjectionSet({k: p.sample(J, rng) for k, p in draw.items()}, draw,
                                      np.where(rng.random(J) < 0.5, -np.inf, -rng.exponential(1.0, J)))
                sel = BinnedSelection(inj, model, torch.device("cuda", 0), chunk=None)
                for label, parts in (("one ensemble", [(0, 1, J)]),
                                     ("ensembles of 4096", [(0, J // 4096, 4096), (J // 4096 * 4096, 1, J % 4096)])):
                    wall = []
                    for _ in range(1 + (3 if a.quick else 5)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for first, n, Wc in parts:
                            sel._compress(first, n, Wc, *sel._buffers)
                        wall.append(time.perf_counter() - t0)
                    emit(path="iso_binned_compress on an injection set, " + label, J=J, B=B, median_wall_s=float(np.median(wall[1:])),
                         min_wall_s=float(np.min(wall[1:])), reps=len(wall) - 1, includes="the calls and the download of their tables")
                auto = BinnedSelection(inj, model, torch.device("cuda", 0))
                zero = np.zeros((1, model.n_params))
                d_alpha = float((auto.alpha(zero)[0] - sel.alpha(zero)[0]).abs().max().item())
                emit(path="ln_alpha, chunked by default against one ensemble", J=J, abs_difference=d_alpha)
            del posts, tables
        del chains
    out.close()


if __name__ == "__main__":
    main()
