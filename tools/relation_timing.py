#!/usr/bin/env python
"""Timing of the population likelihood with a linked column on one device, JSON lines appended to
profiles/relation/relation.jsonl:

* the ``iso_relation_lnlike`` kernels alone (libiso_relation.so: k_relation_stars + k_relation_total) on prepared device
  records and outputs, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct chains:
  10^4 stars x 32 walkers x 100 steps and 10^4 x 300 x 100, H = 64 hyper rows, three columns (mass: Chabrier interim,
  power-law population; age: flat-in-age interim, truncated Gaussian; feh: FehPrior interim, a Gaussian whose mean is linear
  in the sample's age);
* alternating with it pass by pass in the same process, on the same chains, two baselines: (a) ``iso_hier_lnlike`` with a
  truncated Gaussian in place of the link - the difference is the price of the per-sample normaliser (two erfc and a log
  per linked (row, sample), in both passes) - and (b) the same definition through framework ops (``torch.special.erfc``),
  in chunks of hyper rows and stars that keep the ``[rows, stars, samples]`` intermediates inside 4 GB, as
  tools/hier_timing.py does.

    python tools/relation_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hier_timing import FRAMEWORK_BYTES, ROTATE, _feh_shape, make_chain  # noqa: E402  (the chains and the protocol are that tool's)

#          S,       W,   T,   H
SHAPES = ((10 ** 4, 32, 100, 64), (10 ** 4, 300, 100, 64))
NAMES = ("mass", "feh", "age")                                     # make_chain's columns
PIVOT = 9.5


def models():
    """``(linked, plain, interim)``: feh follows age, and the truncated Gaussian in its place."""
    import isochrones_amd as ia
    from isochrones_amd import priors as P
    mass = ia.PowerLaw((0.1, 10.0), alpha=(-4.0, 1.0))
    age = ia.TruncatedGaussian((5.0, 10.15), mean=(8.0, 10.15), sigma=(0.1, 2.0))
    linked = ia.PopulationModel(mass=mass, feh=ia.LinearGaussian("age", (-4.0, 0.5), (-2.0, 2.0), intercept=(-1.0, 0.5),
                                                                 sigma=(0.05, 1.0), pivot=PIVOT), age=age)
    plain = ia.PopulationModel(mass=mass, feh=ia.TruncatedGaussian((-4.0, 0.5), mean=(-1.0, 0.5), sigma=(0.05, 1.0)), age=age)
    interim = {"mass": P.ChabrierPrior(), "feh": P.FehPrior(bounds=(-4.0, 0.5)), "age": P.AgePrior((5.0, 10.15))}
    return linked, plain, interim


def thetas(H, seed=0):
    """``(linked [H, 6], plain [H, 5])``: the same rows, the plain ones without the slope."""
    rng = np.random.default_rng(seed)
    alpha, b0, b1, sg = rng.uniform(-3.0, -1.5, H), rng.uniform(-0.5, 0.1, H), rng.uniform(-0.8, 0.2, H), rng.uniform(0.2, 0.6, H)
    mean, width = rng.uniform(9.2, 9.8, H), rng.uniform(0.3, 1.0, H)
    return np.column_stack([alpha, b0, b1, sg, mean, width]), np.column_stack([alpha, b0, sg, mean, width])


def framework_route(x, S, W, rec, interim):
    """The definition through framework ops: ln L [H] of the packed rows ``rec`` [H, 3] (mass, feh linked to age, age) on
    the storage ``x`` [T, 3, S * W], in chunks of rows and stars whose [rows, stars, samples] intermediates stay inside
    FRAMEWORK_BYTES.  (Without the bounds tests and the bad-sample count: the timed chains lie inside every bound.)"""
    import torch
    from isochrones_amd import priors as P
    T = x.shape[0]
    M = T * W
    dev = x.device
    H = rec.shape[0]
    stars = max(1, min(S, FRAMEWORK_BYTES // (4 * M * 8)))
    rows = max(1, min(H, FRAMEWORK_BYTES // (6 * stars * M * 8)))                  # six live [rows, stars, M] tensors
    ch, fe = interim["mass"], interim["feh"]
    L = torch.zeros(H, dtype=torch.float64, device=dev)
    root_half = 0.7071067811865476
    for s0 in range(0, S, stars):
        n = min(stars, S - s0)
        v = x[:, :, s0 * W:(s0 + n) * W].reshape(T, 3, n, W).permute(1, 2, 0, 3).reshape(3, n, M)
        mass, feh, age = v[0], v[1], v[2]
        lm = torch.log(mass)
        low = (math.log(1 / math.sqrt(2 * math.pi)) - math.log(ch.low.sigma) - ch.low.mu - ch.lognorms[0]) - (lm - ch.low.mu) \
            - 0.5 * ((lm - ch.low.mu) / ch.low.sigma) ** 2
        high = (math.log(ch.high._C()) - ch.lognorms[1]) + ch.high.alpha * lm
        l0 = torch.where(mass < ch.breakpoint, low, high)
        l0 = l0 + torch.log(_feh_shape(fe, feh) / fe._norm)
        l0 = l0 + (math.log(P._LN10 / (10 ** 10.15 - 10 ** 5.0)) + age * P._LN10)
        for h0 in range(0, H, rows):
            p = rec[h0:h0 + rows]
            c = lambda q, k: torch.as_tensor(np.ascontiguousarray(p["p"][:, q, k]), device=dev)[:, None, None]
            r = c(0, 0) + c(0, 1) * lm[None]
            z = (age[None] - c(2, 0)) * c(2, 3)
            r = r + (c(2, 2) - z * z / 2)
            # the link: the mean per (row, sample), the mass in the lower tail
            mu = c(1, 0) + c(1, 4) * (age[None] - c(1, 5))
            z = (feh[None] - mu) * c(1, 3)
            r = r + (c(1, 2) - z * z / 2)
            lo, hi = float(p["lo"][0, 1]), float(p["hi"][0, 1])
            a, b = (lo - mu) * c(1, 3), (hi - mu) * c(1, 3)
            flip = a > 0
            a, b = torch.where(flip, -b, a), torch.where(flip, -a, b)
            del mu, z, flip
            mass_ = 0.5 * (torch.special.erfc(-b * root_half) - torch.special.erfc(-a * root_half))
            del a, b
            r = r - torch.log(mass_)
            del mass_
            r = r - l0[None]
            mx = r.amax(dim=2, keepdim=True)
            w = torch.exp(r - mx)
            L[h0:h0 + rows] += (mx[:, :, 0] + torch.log(w.sum(dim=2)) - math.log(M)).sum(dim=1)
            del r, w
    return L


def alternating_time(routes, n_chains, reps, warmup=1):
    """Median and minimum seconds of every route ``f(chain number)``; in each pass the routes run one after the other on
    the pass's chain, so all of them see the same state of the device."""
    import torch
    for i in range(max(warmup, n_chains)):
        for f in routes:
            f(i % n_chains)
    torch.cuda.synchronize()
    ms = [[] for _ in routes]
    for i in range(reps):
        for k, f in enumerate(routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(i % n_chains)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)) * 1e-3, float(np.min(m)) * 1e-3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation", "relation.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _cabi, _chain, _hier_cabi as hc, _relation_cabi as rl, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("relation_timing needs a GPU: a CPU run says nothing about these paths")
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

    linked, plain, interim = models()
    rlib, hlib = rl.lib(), hc.lib()
    for S, W, T, H in SHAPES:
        if a.quick:
            S = 10 ** 3
        torch.cuda.empty_cache()
        chains = [make_chain(S, W, T, 100 + i) for i in range(rotate)]
        th_l, th_p = thetas(H)
        posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, linked, interim=interim) for x in chains]
        assert all(p.storage.data_ptr() == x.data_ptr() for p, x in zip(posts, chains))       # read where it lies
        n_eval = S * W * T * H
        shape = dict(S=S, W=W, T=T, H=H, columns=list(NAMES), linked="feh on age", evaluations=n_eval, rotating_chains=rotate,
                     reps=reps, row_tile=rl.ROW_TILE)
        up = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1)).cuda()
        rec_l = linked.pack(th_l)
        rows_l, rows_p = up(rec_l), up(plain.pack(th_p))
        irec = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        ell, ess = torch.empty(H, S, **f64), torch.empty(H, S, **f64)
        n_bad, L, mn = torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty(H, **f64), torch.empty(H, **f64)
        stream = dev.stream_ptr(0)

        def relation(i):
            rl.check(rlib.iso_relation_lnlike(posts[i]._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                              dev.ptr(irec), dev.ptr(rows_l), H, None, dev.ptr(ell), dev.ptr(ess),
                                              dev.ptr(n_bad), dev.ptr(L), dev.ptr(mn), stream))

        def hier(i):
            hc.check(hlib.iso_hier_lnlike(posts[i]._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, dev.ptr(irec),
                                          dev.ptr(rows_p), H, None, dev.ptr(ell), dev.ptr(ess), dev.ptr(n_bad), dev.ptr(L),
                                          dev.ptr(mn), stream))
        (med, best), (med_h, best_h) = alternating_time([relation, hier], rotate, reps)
        relation(0)
        L_kernel = L.clone()
        emit(path="iso_relation_lnlike", median_s=med, min_s=best, evaluations_per_s=n_eval / med,
             min_ess_median=float(mn.median().item()), bad_samples=int(n_bad.sum().item()), **shape)
        emit(path="iso_hier_lnlike, a truncated Gaussian in place of the link", median_s=med_h, min_s=best_h,
             evaluations_per_s=n_eval / med_h, relation_over_hier=med / med_h,
             ns_per_linked_row_sample_of_the_normaliser=(med - med_h) / n_eval * 1e9, **shape)
        L_fw = framework_route(chains[0], S, W, rec_l, interim)
        scaled = ((L_fw - L_kernel).abs() / (1 + L_kernel.abs())).max().item()
        r_fw = max(3, reps // 10)
        (med_k, _), (med_f, best_f) = alternating_time([relation, lambda i: framework_route(chains[i], S, W, rec_l, interim)],
                                                       rotate, r_fw)
        emit(path="framework_ops", median_s=med_f, min_s=best_f, evaluations_per_s=n_eval / med_f,
             intermediate_bytes_limit=FRAMEWORK_BYTES, max_scaled_difference_of_L_to_the_kernel=scaled,
             iso_relation_lnlike_alongside_median_s=med_k, speedup_of_iso_relation_lnlike=med_f / med_k, **dict(shape, reps=r_fw))
        del posts, chains, rows_l, rows_p, ell, ess
    out.close()


if __name__ == "__main__":
    main()
