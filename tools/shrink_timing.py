#!/usr/bin/env python
"""Timing of the per-star posteriors under a binned population density on one device, JSON lines appended to
profiles/shrink/shrink.jsonl:

* ``iso_shrink_cells`` (libiso_shrink.so: k_shrink_cells), ``iso_shrink_weights`` (k_shrink_weights) and
  ``iso_reweight_summary`` (libiso_reweight.so: k_reweight_summary, three value columns, three quantiles), each C entry on
  prepared device buffers between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct chains:
  10^4 stars x 32 walkers x 100 steps and 10^4 x 300 x 100, the three columns of tools/hier_timing.py, an 8-bin age
  histogram (B = 8) and an 8 x 8 grid of [Fe/H] bins per age bin (B = 64), H = 8, 64 and 1 024 hyper rows;
* ``PopulationPosterior.star_posteriors`` end to end (numpy rows in, a DataFrame out: the cell table on the host, the
  contraction for ell, the three kernels, the download);
* alternating with the three kernels pass by pass in the same process, on the same chains, the only other route:
  framework ops - the per-sample term, ``bucketize`` for the cell, broadcast weights in chunks of stars that keep the
  ``[rows, stars, samples]`` intermediates inside 4 GB, then per value column ``torch.sort``, a gather of the weights,
  ``cumsum`` and ``searchsorted``, as tools/reweight_timing.py does for the uncoupled case.  Where a pass over all stars takes
  more than ``framework_chunks`` chunks it is timed on the first that many chunks of stars and ``median_s`` is scaled to S
  (its cost is linear in the number of chunks); such a row has ``scaled_to_S`` true and its ratio is an extrapolation;
* for scale, ``iso_reweight_stars`` at the same shape and H on tools/hier_timing.py's TruncatedGaussian model;
* k_shrink_weights never reads H: its time at H = 8 against H = 1 024, a sanity line.

    python tools/shrink_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hier_timing as ht  # noqa: E402  (the chains and the protocol are that tool's)
from binned_timing import NAMES, SHAPES, grids, interim_priors, timed  # noqa: E402  (the grids are that tool's)

ROWS = (8, 64, 1024)
GRIDS = ("age 8", "age 8 x feh 8")
Q3 = (0.5, 0.16, 0.84)
FRAMEWORK_CHUNKS = 4


def framework_route(x, S, W, model, interim, lnh, ell, q, stars_limit=None):
    """The definition through framework ops on the storage ``x`` [T, 3, S * W] (mass, feh, age) with ``lnh`` [H, B] and
    ``ell`` [H, S] given: ``(quant [n, 3, K], mean [n, 3], ess [n], chunks, stars a chunk)`` of the first ``stars_limit``
    chunks' stars.  (Without the bounds tests, the counts and the closed last edge: the timed chains lie inside every bound
    and on no edge.)"""
    import torch
    from isochrones_amd import priors as P
    T = x.shape[0]
    M = T * W
    dev = x.device
    H = lnh.shape[0]
    grid = model.bin_grid()
    stars = max(1, min(S, ht.FRAMEWORK_BYTES // (4 * H * M * 8)))                    # four live [H, stars, M] tensors
    n_chunks = -(-S // stars)
    if stars_limit is not None:
        n_chunks = min(n_chunks, stars_limit)
    done = min(S, n_chunks * stars)
    ch, fe = interim["mass"], interim["feh"]
    frozen = grid["frozen"]
    edges = [torch.as_tensor(e, device=dev) for e in grid["edges"]]
    qs = torch.as_tensor(np.asarray(q), device=dev)
    quant = torch.empty(done, 3, len(q), dtype=torch.float64, device=dev)
    mean, ess = torch.empty(done, 3, dtype=torch.float64, device=dev), torch.empty(done, dtype=torch.float64, device=dev)
    for s0 in range(0, done, stars):
        n = min(stars, done - s0)
        v = x[:, :, s0 * W:(s0 + n) * W].reshape(T, 3, n, W).permute(1, 2, 0, 3).reshape(3, n, M)       # [3, n, M]
        mass, feh, age = v[0], v[1], v[2]
        lm = torch.log(mass)
        low = (math.log(1 / math.sqrt(2 * math.pi)) - math.log(ch.low.sigma) - ch.low.mu - ch.lognorms[0]) - (lm - ch.low.mu) \
            - 0.5 * ((lm - ch.low.mu) / ch.low.sigma) ** 2
        high = (math.log(ch.high._C()) - ch.lognorms[1]) + ch.high.alpha * lm
        l0 = torch.where(mass < ch.breakpoint, low, high)
        l0 = l0 + torch.log(ht._feh_shape(fe, feh) / fe._norm)
        l0 = l0 + (math.log(P._LN10 / (10 ** 10.15 - 10 ** 5.0)) + age * P._LN10)
        c = -l0
        for k in grid["frozen_cols"]:                                # mass: a power law; feh: a Gaussian
            p = frozen["p"][k]
            if NAMES[k] == "mass":
                c = c + (p[0] + p[1] * lm)
            else:
                z = (v[k] - p[0]) * p[3]
                c = c + (p[2] - z * z / 2)
        cell = torch.zeros(n, M, dtype=torch.int64, device=dev)
        for a, k in enumerate(grid["axes"]):
            kb = (torch.bucketize(v[k], edges[a], right=True) - 1).clamp_(0, len(edges[a]) - 2)
            cell = cell * (len(edges[a]) - 1) + kb
        u = torch.exp(c[None] + lnh[:, cell] - ell[:, s0:s0 + n, None]).sum(dim=0)                      # [n, M]
        tot = u.sum(dim=1)
        ess[s0:s0 + n] = tot * tot / (u * u).sum(dim=1)
        for k in range(3):
            y = v[k]
            mean[s0:s0 + n, k] = (u * y).sum(dim=1) / tot
            ys, order = torch.sort(y, dim=1)
            cum = torch.cumsum(torch.gather(u, 1, order), dim=1)
            at = torch.searchsorted(cum, (qs[None] * tot[:, None]).contiguous()).clamp_(max=M - 1)
            quant[s0:s0 + n, k] = torch.gather(ys, 1, at)
    return quant, mean, ess, n_chunks, stars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink", "shrink.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _cabi, _chain, _hier_cabi as hc, _reweight_cabi as rc, _shrink_cabi as sc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("shrink_timing needs a GPU: a CPU run says nothing about these paths")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a")
    reps, rotate = (5, 2) if a.quick else (30, ht.ROTATE)
    name = torch.cuda.get_device_name(0)

    def emit(**row):
        row["device"] = name
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row), flush=True)

    lib, rlib, hlib = sc.lib(), rc.lib(), hc.lib()
    interim = interim_priors()
    stream = dev.stream_ptr(0)
    probs = np.asarray(Q3, dtype=np.float64)
    pq = probs.ctypes.data_as(C.POINTER(C.c_double))
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
    models = grids()
    for S, W, T in SHAPES:
        if a.quick:
            S = 10 ** 3
        torch.cuda.empty_cache()
        M = W * T
        chains = [ht.make_chain(S, W, T, 100 + i) for i in range(rotate)]
        weights = torch.empty(S, M, **f64)
        wsum, ess = torch.empty(S, **f64), torch.empty(S, **f64)
        n_bad, n_out = torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty(S, dtype=torch.int32, device="cuda")
        mean, sd, quant = torch.empty(S, 3, **f64), torch.empty(S, 3, **f64), torch.empty(S, 3, 3, **f64)
        n_nan = torch.empty(S, 3, dtype=torch.int32, device="cuda")
        weights_at = {}
        for gname in GRIDS:
            model = models[gname]
            B = model.n_cells
            posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim) for x in chains]
            assert all(p.storage.data_ptr() == x.data_ptr() for p, x in zip(posts, chains))       # read where it lies
            grid = model.bin_grid()
            g_axes, g_bins, g_frozen = i32(grid["axes"]), i32([len(e) - 1 for e in grid["edges"]]), i32(grid["frozen_cols"])
            d_interim = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
            d_frozen = torch.from_numpy(grid["frozen"].view(np.uint8).copy()).cuda()
            d_edges = torch.from_numpy(np.concatenate(grid["edges"])).cuda()
            tables = [p.bin_tables() for p in posts]
            vals = [(hc.IsoHierColumn * 3)(*[hc.IsoHierColumn(p.storage.data_ptr(), 3, k, S, 0) for k in range(3)]) for p in posts]
            lnG, cellp = torch.empty(B, S, **f64), torch.empty(B, S, **f64)
            for H in ROWS:
                rng = np.random.default_rng(H)
                theta = rng.uniform(-2.0, 2.0, (H, model.n_params))
                lnh = torch.from_numpy(model.cell_table(theta)["lnh"]).cuda()
                ells = [p._evaluate_binned(torch.from_numpy(theta).cuda())[2].contiguous() for p in posts]
                shape = dict(S=S, W=W, T=T, H=H, grid=gname, B=B, columns=list(NAMES), value_columns=list(NAMES),
                             quantiles=list(Q3), rotating_chains=rotate, reps=reps)

                def cells(i):
                    sc.check(lib.iso_shrink_cells(dev.ptr(tables[i][0]), dev.ptr(tables[i][2]), B, S, 0, S, dev.ptr(lnh),
                                                  dev.ptr(ells[i]), H, None, dev.ptr(lnG), dev.ptr(cellp), stream))

                def weigh(i):
                    sc.check(lib.iso_shrink_weights(posts[i]._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                                    dev.ptr(d_interim), dev.ptr(d_frozen), len(grid["frozen_cols"]), g_frozen,
                                                    len(grid["axes"]), g_axes, g_bins, dev.ptr(d_edges), dev.ptr(tables[i][2]),
                                                    dev.ptr(lnG), None, dev.ptr(weights), dev.ptr(wsum), dev.ptr(ess),
                                                    dev.ptr(n_bad), dev.ptr(n_out), stream))

                def summarise(i):
                    rc.check(rlib.iso_reweight_summary(vals[i], 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, None, pq, 3,
                                                       dev.ptr(weights), dev.ptr(mean), dev.ptr(sd), dev.ptr(quant), dev.ptr(n_nan),
                                                       stream))

                def kernels(i):
                    cells(i)
                    weigh(i)
                    summarise(i)

                med_c, best_c = timed(cells, rotate, reps, rotate)
                emit(path="iso_shrink_cells", median_s=med_c, min_s=best_c, star_cell_rows_per_s=S * B * H / med_c, **shape)
                cells(0)
                med_w, best_w = timed(weigh, rotate, reps, rotate)
                emit(path="iso_shrink_weights", median_s=med_w, min_s=best_w, samples_per_s=S * M / med_w,
                     chain_bytes_per_s=S * M * 24 / med_w, weight_bytes_per_s=S * M * 8 / med_w, **shape)
                weights_at[(gname, H)] = med_w
                weigh(0)
                med_s, best_s = timed(summarise, rotate, reps, rotate)
                emit(path="iso_reweight_summary", median_s=med_s, min_s=best_s, **shape)
                kernels(0)
                k_quant, k_mean, k_ess = quant.clone(), mean.clone(), ess.clone()
                emit(path="the three kernels", median_s=med_c + med_w + med_s, out_samples=int(n_out.sum().item()),
                     bad_samples=int(n_bad.sum().item()), min_ess_of_the_stars=float(k_ess.min().item()),
                     max_wsum_off_H_M=float((wsum / (H * M) - 1).abs().max().item()), **shape)
                r_e = max(5, reps // 3)
                med_e, best_e = timed(lambda i: posts[i].star_posteriors(theta, columns=NAMES, q=Q3), rotate, r_e, rotate)
                emit(path="PopulationPosterior.star_posteriors", median_s=med_e, min_s=best_e, **dict(shape, reps=r_e))

                # the framework route, alternating pass by pass with the three kernels
                def framework(i):
                    return framework_route(chains[i], S, W, model, interim, lnh, ells[i], Q3, FRAMEWORK_CHUNKS)

                f_quant, f_mean, f_ess, n_chunks, per_chunk = framework(0)
                done = f_ess.shape[0]
                agree = dict(quantiles_equal_share=float((f_quant == k_quant[:done]).double().mean().item()),
                             max_scaled_difference_of_mean=float(((f_mean - k_mean[:done]).abs() / (1 + k_mean[:done].abs())).max().item()),
                             max_relative_difference_of_ess=float(((f_ess - k_ess[:done]).abs() / k_ess[:done]).max().item()))
                ms_f, ms_k = [], []
                torch.cuda.synchronize()
                for i in range(3):
                    for f, ms in ((framework, ms_f), (kernels, ms_k)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f(i % rotate)
                        e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                med_f, med_k = float(np.median(ms_f)) * 1e-3, float(np.median(ms_k)) * 1e-3
                scale = S / done
                emit(path="framework_ops", measured_median_s=med_f, measured_stars=done, stars_per_chunk=per_chunk,
                     framework_chunks=n_chunks, median_s=med_f * scale, scaled_to_S=done < S,
                     intermediate_bytes_limit=ht.FRAMEWORK_BYTES, the_three_kernels_alongside_median_s=med_k,
                     speedup_of_the_three_kernels=med_f * scale / med_k, speedup_of_star_posteriors_end_to_end=med_f * scale / med_e,
                     **agree, **dict(shape, reps=3))
                del ells, lnh
            del posts, tables, lnG, cellp
        for gname in GRIDS:
            emit(path="iso_shrink_weights, H = 8 against H = 1024 (it never reads H)", S=S, W=W, T=T, grid=gname,
                 median_s_H8=weights_at[(gname, 8)], median_s_H1024=weights_at[(gname, 1024)],
                 ratio=weights_at[(gname, 1024)] / weights_at[(gname, 8)])
        # for scale: the uncoupled route's kernels at the same shape, five value columns replaced by the model's three
        model_u, interim_u = ht.model_and_priors()
        posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model_u, interim=interim_u) for x in chains]
        irec = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
        vals = [(hc.IsoHierColumn * 3)(*[hc.IsoHierColumn(p.storage.data_ptr(), 3, k, S, 0) for k in range(3)]) for p in posts]
        for H in ROWS:
            th = ht.thetas(H)
            rows = torch.from_numpy(np.ascontiguousarray(model_u.pack(th)).view(np.uint8).reshape(-1)).cuda()
            ells = []
            for p in posts:
                ell, e2 = torch.empty(H, S, **f64), torch.empty(H, S, **f64)
                hc.check(hlib.iso_hier_lnlike(p._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, dev.ptr(irec),
                                              dev.ptr(rows), H, None, dev.ptr(ell), dev.ptr(e2), dev.ptr(n_bad), None, None, stream))
                ells.append(ell)
                del e2

            def stars_call(i):
                rc.check(rlib.iso_reweight_stars(posts[i]._columns(None, 0, S), 3, vals[i], 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                                 dev.ptr(irec), dev.ptr(rows), H, dev.ptr(ells[i]), None, pq, 3, dev.ptr(weights),
                                                 dev.ptr(wsum), dev.ptr(ess), dev.ptr(n_bad), dev.ptr(mean), dev.ptr(sd),
                                                 dev.ptr(quant), dev.ptr(n_nan), stream))
            r_u = reps if H < 1024 else max(3, reps // 10)
            med_u, best_u = timed(stars_call, rotate, r_u, min(rotate, 2))
            emit(path="iso_reweight_stars on a TruncatedGaussian model, for scale", S=S, W=W, T=T, H=H, median_s=med_u, min_s=best_u,
                 evaluations_per_s=S * M * H / med_u, value_columns=list(NAMES), rotating_chains=rotate, reps=r_u)
            del ells, rows
        del chains, posts, weights
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
