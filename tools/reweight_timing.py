#!/usr/bin/env python
"""Timing of the population-informed per-star posteriors on one device, JSON lines appended to
profiles/reweight/reweight.jsonl:

* the ``iso_reweight_stars`` kernels alone (libiso_reweight.so: k_reweight_weights + k_reweight_summary) on prepared device
  records, ``ell`` and outputs, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct
  chains: 10^4 stars x 32 walkers x 100 steps and 10^4 x 300 x 100, three model columns (those of tools/hier_timing.py), H =
  8 and 64 hyper rows, 5 value columns (the three and two more), three quantiles.  Reported: density-ratio evaluations (star
  x sample x row) per second, and the share of the vector-float64 bound of the weights kernel (hier_timing's count of
  operations for one pass instead of two);
* ``PopulationPosterior.star_posteriors`` end to end on the same chains (``ell`` from ``iso_hier_lnlike``, packing, the
  slices under the budget, the DataFrame);
* in the same process, on the same chains, alternating with the kernels, the only other way to these numbers: framework
  ops - broadcast weights in chunks of stars that keep the ``[rows, stars, samples]`` intermediates inside 4 GB, then per
  value column ``torch.sort``, a gather of the weights, ``cumsum`` and ``searchsorted``.

    python tools/reweight_timing.py [--quick] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import hier_timing as ht  # noqa: E402  (the chains' model columns, the rows, the framework-op family arithmetic, the clock)

#          S,       W,   T
SHAPES = ((10 ** 4, 32, 100), (10 ** 4, 300, 100))
ROWS = (8, 64)
ROTATE = 8
NAMES = ("mass", "feh", "age", "distance", "AV")
Q3 = (0.5, 0.16, 0.84)
#: hier_timing's count for one pass over the samples instead of two: the family arithmetic (17), the subtraction of
#: ln_norm, an exp (25) and the sum over the rows
OPS_PER_EVALUATION = 17 + 1 + 25 + 1


def make_chain(S, W, T, seed):
    """hier_timing's (mass, feh, age) and two more columns, parameter-major [T, 5, S * W] on the device."""
    import torch
    x = torch.empty(T, 5, S * W, dtype=torch.float64, device="cuda")
    x[:, :3] = ht.make_chain(S, W, T, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1000)
    x[:, 3] = 100.0 + 10.0 * torch.randn(T, S * W, dtype=torch.float64, device="cuda", generator=g)
    x[:, 4] = torch.rand(T, S * W, dtype=torch.float64, device="cuda", generator=g)
    return x


def framework_route(x, S, W, theta, model, interim, ell, q):
    """The definition through framework ops on the storage ``x`` [T, 5, S * W] with ``ell`` [H, S] given: ``(quant [S, 5, K],
    mean [S, 5], sd [S, 5], ess [S])``.  (Without the bounds tests, the bad-sample count and the NaN counts: the timed chains lie
    inside every bound.)"""
    import torch
    from isochrones_amd import priors as P
    T = x.shape[0]
    M = T * W
    dev = x.device
    H = len(theta)
    rec = model.pack(theta)
    stars = max(1, min(S, ht.FRAMEWORK_BYTES // (4 * H * M * 8)))                    # four live [H, stars, M] tensors
    ch, fe = interim["mass"], interim["feh"]
    c = lambda k, j: torch.as_tensor(np.ascontiguousarray(rec["p"][:, k, j]), device=dev)[:, None, None]
    qs = torch.as_tensor(np.asarray(q), device=dev)
    quant = torch.empty(S, 5, len(q), dtype=torch.float64, device=dev)
    mean, sd = torch.empty(S, 5, dtype=torch.float64, device=dev), torch.empty(S, 5, dtype=torch.float64, device=dev)
    ess = torch.empty(S, dtype=torch.float64, device=dev)
    for s0 in range(0, S, stars):
        n = min(stars, S - s0)
        v = x[:, :, s0 * W:(s0 + n) * W].reshape(T, 5, n, W).permute(1, 2, 0, 3).reshape(5, n, M)       # [5, n, M]
        mass, feh, age = v[0], v[1], v[2]
        lm = torch.log(mass)
        low = (math.log(1 / math.sqrt(2 * math.pi)) - math.log(ch.low.sigma) - ch.low.mu - ch.lognorms[0]) - (lm - ch.low.mu) \
            - 0.5 * ((lm - ch.low.mu) / ch.low.sigma) ** 2
        high = (math.log(ch.high._C()) - ch.lognorms[1]) + ch.high.alpha * lm
        l0 = torch.where(mass < ch.breakpoint, low, high)
        l0 = l0 + torch.log(ht._feh_shape(fe, feh) / fe._norm)
        l0 = l0 + (math.log(P._LN10 / (10 ** 10.15 - 10 ** 5.0)) + age * P._LN10)
        r = c(0, 0) + c(0, 1) * lm[None]
        for k, col in ((1, feh), (2, age)):
            z = (col[None] - c(k, 0)) * c(k, 3)
            r = r + (c(k, 2) - z * z / 2)
        u = torch.exp(r - l0[None] - ell[:, s0:s0 + n, None]).sum(dim=0)                                    # [n, M]
        del r, z
        tot = u.sum(dim=1)
        ess[s0:s0 + n] = tot * tot / (u * u).sum(dim=1)
        for k in range(5):
            y = v[k]
            mu = (u * y).sum(dim=1) / tot
            mean[s0:s0 + n, k] = mu
            sd[s0:s0 + n, k] = torch.sqrt((u * (y - mu[:, None]) ** 2).sum(dim=1) / tot)
            ys, order = torch.sort(y, dim=1)
            cum = torch.cumsum(torch.gather(u, 1, order), dim=1)
            at = torch.searchsorted(cum, (qs[None] * tot[:, None]).contiguous()).clamp_(max=M - 1)
            quant[s0:s0 + n, k] = torch.gather(ys, 1, at)
    return quant, mean, sd, ess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reweight", "reweight.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _cabi, _chain, _hier_cabi as hc, _reweight_cabi as rc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("reweight_timing needs a GPU: a CPU run says nothing about these paths")
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

    model, interim = ht.model_and_priors()
    lib, hlib = rc.lib(), hc.lib()
    stream = dev.stream_ptr(0)
    probs = np.asarray(Q3, dtype=np.float64)
    f64 = dict(dtype=torch.float64, device="cuda")
    for S, W, T in SHAPES:
        if a.quick:
            S = 10 ** 3
        M = W * T
        chains = [make_chain(S, W, T, 100 + i) for i in range(rotate)]
        posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim) for x in chains]
        assert all(p.storage.data_ptr() == x.data_ptr() for p, x in zip(posts, chains))       # read where it lies
        irec = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
        weights = torch.empty(S, M, **f64)
        wsum, ess, n_bad = torch.empty(S, **f64), torch.empty(S, **f64), torch.empty(S, dtype=torch.int32, device="cuda")
        mean, sd, quant = torch.empty(S, 5, **f64), torch.empty(S, 5, **f64), torch.empty(S, 5, 3, **f64)
        n_nan = torch.empty(S, 5, dtype=torch.int32, device="cuda")
        for H in ROWS:
            th = ht.thetas(H)
            n_eval = S * M * H
            shape = dict(S=S, W=W, T=T, H=H, columns=list(NAMES[:3]), value_columns=list(NAMES), quantiles=list(Q3),
                         evaluations=n_eval, rotating_chains=rotate, reps=reps)
            rows = torch.from_numpy(np.ascontiguousarray(model.pack(th)).view(np.uint8).reshape(-1)).cuda()
            ells = []
            for p in posts:                                             # ell of every chain, prepared once
                ell, e2 = torch.empty(H, S, **f64), torch.empty(H, S, **f64)
                hc.check(hlib.iso_hier_lnlike(p._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, dev.ptr(irec),
                                              dev.ptr(rows), H, None, dev.ptr(ell), dev.ptr(e2), dev.ptr(n_bad), None, None, stream))
                ells.append(ell)
            vals = [(hc.IsoHierColumn * 5)(*[hc.IsoHierColumn(p.storage.data_ptr(), 5, k, S, 0) for k in range(5)]) for p in posts]

            def kernels(i):
                rc.check(lib.iso_reweight_stars(posts[i]._columns(None, 0, S), 3, vals[i], 5, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S,
                                                dev.ptr(irec), dev.ptr(rows), H, dev.ptr(ells[i]), None,
                                                probs.ctypes.data_as(C.POINTER(C.c_double)), 3, dev.ptr(weights), dev.ptr(wsum),
                                                dev.ptr(ess), dev.ptr(n_bad), dev.ptr(mean), dev.ptr(sd), dev.ptr(quant),
                                                dev.ptr(n_nan), stream))

            def framework(i):
                return framework_route(chains[i], S, W, th, model, interim, ells[i], Q3)

            # what the two routes give on the first chain
            kernels(0)
            k_quant, k_mean, k_ess = quant.clone(), mean.clone(), ess.clone()
            f_quant, f_mean, _, f_ess = framework(0)
            agree = dict(quantiles_equal_share=float((f_quant == k_quant).double().mean().item()),
                         max_scaled_difference_of_mean=float(((f_mean - k_mean).abs() / (1 + k_mean.abs())).max().item()),
                         max_relative_difference_of_ess=float(((f_ess - k_ess).abs() / k_ess).max().item()))
            # alternating in the same process: a block of kernel passes, the framework passes, the rest of the kernel passes
            r_fw = max(3, reps // 10)
            med1, best1 = ht.device_time([lambda i=i: kernels(i) for i in range(rotate)], reps // 2)
            med_f, best_f = ht.device_time([lambda i=i: framework(i) for i in range(rotate)], r_fw, warmup=1)
            med2, best2 = ht.device_time([lambda i=i: kernels(i) for i in range(rotate)], reps - reps // 2)
            med, best = (med1 + med2) / 2, min(best1, best2)
            least = n_eval * OPS_PER_EVALUATION / ht.PEAK_F64_VECTOR_OPS_PER_S
            emit(path="iso_reweight_stars", median_s=med, min_s=best, median_s_of_the_two_blocks=[med1, med2],
                 evaluations_per_s=n_eval / med, f64_vector_ops_per_evaluation=OPS_PER_EVALUATION,
                 least_time_vector_f64_s=least, share_of_vector_f64_bound=least / med,
                 min_ess_of_the_stars=float(k_ess.min().item()), bad_samples=int(n_bad.sum().item()), **shape)
            med_e, best_e = ht.device_time([lambda p=p: p.star_posteriors(th, columns=NAMES, q=Q3) for p in posts], max(5, reps // 3))
            emit(path="PopulationPosterior.star_posteriors", median_s=med_e, min_s=best_e, evaluations_per_s=n_eval / med_e,
                 **dict(shape, reps=max(5, reps // 3)))
            emit(path="framework_ops", median_s=med_f, min_s=best_f, evaluations_per_s=n_eval / med_f,
                 intermediate_bytes_limit=ht.FRAMEWORK_BYTES, speedup_of_iso_reweight_stars=med_f / med,
                 speedup_of_star_posteriors_end_to_end=med_f / med_e, **agree, **dict(shape, reps=r_fw))
            del rows, ells
        del chains, posts, weights
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
