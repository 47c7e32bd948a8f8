#!/usr/bin/env python
"""Timing of the hierarchical population likelihood on one device, JSON lines appended to profiles/hier/hier.jsonl:

* the ``iso_hier_lnlike`` kernels alone (libiso_hier.so: k_hier_stars + k_hier_total) on prepared device records and
  outputs, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct chains: 10^4 stars x 32
  walkers x 100 steps with 3 columns (mass: Chabrier interim, power-law population; feh: FehPrior interim, truncated
  Gaussian; age: flat-in-age interim, truncated Gaussian) at H = 64 and H = 1024 hyper rows, and 10^4 x 300 x 100 at
  H = 64.  Reported: density-ratio evaluations (star x sample x row) per second, and the share of the vector-float64
  bound: the float64 vector operations the definition needs per evaluation (``OPS_PER_EVALUATION``, counted from the
  source: both passes' family arithmetic, one exp, the weight sums) over the chip's peak vector-float64 issue rate;
* ``PopulationPosterior.lnlike`` end to end on the same chains (packing the records, the upload, the call, the download);
* in the same process, on the same chains, the only other way to these numbers: the same definition through framework
  ops, in chunks of hyper rows (and of stars) that keep the ``[rows, stars, samples]`` intermediates inside 4 GB;
* ``fit_mcmc`` of the three hyper-parameters (mass.alpha, feh.mean, feh.sigma), 64 walkers x (200 + 200), on the
  32-walker catalog.

    python tools/hier_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#          S,       W,   T,   H
SHAPES = ((10 ** 4, 32, 100, 64), (10 ** 4, 32, 100, 1024), (10 ** 4, 300, 100, 64))
ROTATE = 8
NAMES = ("mass", "feh", "age")
#: MI355X: 78.6 TFLOP/s of vector float64 counts a fused multiply-add as two; an add, a multiply or an fma is one issue
PEAK_F64_VECTOR_OPS_PER_S = 78.6e12 / 2
#: float64 vector operations per (star, sample, row) of the three-column model above, counted from hier.hip: the power law
#: (multiply, add) and two truncated Gaussians (subtract, three multiplies, add), the three interim differences and two sums
#: of the log ratio: 17, in both passes; the maximum; the subtraction, an exp (range reduction, an 11-term polynomial, the
#: scaling: 25) and the two weight sums (multiply, two adds)
OPS_PER_EVALUATION = 2 * 17 + 1 + 1 + 25 + 3
FRAMEWORK_BYTES = 4 << 30


def make_chain(S, W, T, seed):
    """Parameter-major storage [T, 3, S * W] of (mass, feh, age) on the device: every star has a point of its own and its
    samples scatter about it, as a fit leaves them."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)

    def col(lo, hi, width):
        centre = lo + (hi - lo) * (0.1 + 0.8 * torch.rand(S, 1, dtype=torch.float64, device="cuda", generator=g))
        x = centre + width * (hi - lo) * torch.randn(T, S, W, dtype=torch.float64, device="cuda", generator=g)
        return x.clamp_(lo, hi).view(T, S * W)
    x = torch.empty(T, 3, S * W, dtype=torch.float64, device="cuda")
    x[:, 0] = col(0.3, 3.0, 0.05)
    x[:, 1] = col(-1.0, 0.4, 0.1)
    x[:, 2] = col(8.8, 10.1, 0.05)
    return x


def model_and_priors():
    import isochrones_amd as ia
    from isochrones_amd import priors as P
    model = ia.PopulationModel(mass=ia.PowerLaw((0.1, 10.0), alpha=(-4.0, 1.0)),
                               feh=ia.TruncatedGaussian((-4.0, 0.5), mean=(-1.0, 0.5), sigma=(0.05, 1.0)),
                               age=ia.TruncatedGaussian((5.0, 10.15), mean=(8.0, 10.15), sigma=(0.1, 2.0)))
    interim = {"mass": P.ChabrierPrior(), "feh": P.FehPrior(bounds=(-4.0, 0.5)), "age": P.AgePrior((5.0, 10.15))}
    return model, interim


def thetas(H, seed=0):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-3.0, -1.5, H), rng.uniform(-0.5, 0.1, H), rng.uniform(0.2, 0.6, H),
                            rng.uniform(9.2, 9.8, H), rng.uniform(0.3, 1.0, H)])


def framework_route(x, S, W, theta, model, interim):
    """The definition through framework ops: ln L [H] of the rows ``theta`` on the storage ``x`` [T, 3, S * W], in chunks of
    rows and stars whose [rows, stars, samples] intermediates stay inside FRAMEWORK_BYTES.  (Without the bounds tests and
    the bad-sample count: the timed chains lie inside every bound.)"""
    import torch
    from isochrones_amd import priors as P
    T = x.shape[0]
    M = T * W
    dev = x.device
    rec = model.pack(theta)
    stars = max(1, min(S, FRAMEWORK_BYTES // (4 * M * 8)))                          # four live [1, stars, M] tensors at least
    rows = max(1, min(len(theta), FRAMEWORK_BYTES // (4 * stars * M * 8)))
    ch, fe = interim["mass"], interim["feh"]
    L = torch.zeros(len(theta), dtype=torch.float64, device=dev)
    for s0 in range(0, S, stars):
        n = min(stars, S - s0)
        v = x[:, :, s0 * W:(s0 + n) * W].reshape(T, 3, n, W).permute(1, 2, 0, 3).reshape(3, n, M)       # [3, n, M]
        mass, feh, age = v[0], v[1], v[2]
        lm = torch.log(mass)
        # the interim terms, once per sample: Chabrier, FehPrior, flat in age
        low = (math.log(1 / math.sqrt(2 * math.pi)) - math.log(ch.low.sigma) - ch.low.mu - ch.lognorms[0]) - (lm - ch.low.mu) \
            - 0.5 * ((lm - ch.low.mu) / ch.low.sigma) ** 2
        high = (math.log(ch.high._C()) - ch.lognorms[1]) + ch.high.alpha * lm
        l0 = torch.where(mass < ch.breakpoint, low, high)
        l0 = l0 + torch.log(_feh_shape(fe, feh) / fe._norm)
        l0 = l0 + (math.log(P._LN10 / (10 ** 10.15 - 10 ** 5.0)) + age * P._LN10)
        for h0 in range(0, len(theta), rows):
            p = rec[h0:h0 + rows]
            c = lambda q, k: torch.as_tensor(np.ascontiguousarray(p["p"][:, q, k]), device=dev)[:, None, None]
            r = c(0, 0) + c(0, 1) * lm[None]
            for q, col in ((1, feh), (2, age)):
                z = (col[None] - c(q, 0)) * c(q, 3)
                r = r + (c(q, 2) - z * z / 2)
            r = r - l0[None]
            mx = r.amax(dim=2, keepdim=True)
            w = torch.exp(r - mx)
            L[h0:h0 + rows] += (mx[:, :, 0] + torch.log(w.sum(dim=2)) - math.log(M)).sum(dim=1)
            del r, w, z
    return L


def _feh_shape(fe, feh):
    import torch
    disk = (1.0 / 2.5066282746310007 * (0.8 / 0.15 * torch.exp(-0.5 * (feh - 0.016) ** 2 / 0.15 ** 2)
                                        + 0.2 / 0.22 * torch.exp(-0.5 * (feh + 0.15) ** 2 / 0.22 ** 2)))
    halo = 1.0 / math.sqrt(2 * math.pi * 0.4 ** 2) * torch.exp(-0.5 * (feh + 1.5) ** 2 / 0.4 ** 2)
    return fe.halo_fraction * halo + (1 - fe.halo_fraction) * disk


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
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating chains, 10^3 stars, a short fit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hier", "hier.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _cabi, _chain, _hier_cabi as hc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("hier_timing needs a GPU: a CPU run says nothing about these paths")
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

    model, interim = model_and_priors()
    lib = hc.lib()
    chains, key = None, None
    for S, W, T, H in SHAPES:
        if a.quick:
            S = 10 ** 3
        if key != (S, W, T):
            del chains
            torch.cuda.empty_cache()
            chains, key = [make_chain(S, W, T, 100 + i) for i in range(rotate)], (S, W, T)
        th = thetas(H)
        posts = [ia.PopulationPosterior((_chain.from_storage(x, S, W, False), NAMES), None, model, interim=interim) for x in chains]
        assert all(p.storage.data_ptr() == x.data_ptr() for p, x in zip(posts, chains))       # read where it lies
        n_eval = S * W * T * H
        shape = dict(S=S, W=W, T=T, H=H, columns=list(NAMES), evaluations=n_eval, rotating_chains=rotate, reps=reps)
        # the kernels alone: records and outputs prepared once
        rows = torch.from_numpy(np.ascontiguousarray(model.pack(th)).view(np.uint8).reshape(-1)).cuda()
        irec = torch.from_numpy(posts[0].interim.view(np.uint8).copy()).cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        ell, ess = torch.empty(H, S, **f64), torch.empty(H, S, **f64)
        n_bad, L, mn = torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty(H, **f64), torch.empty(H, **f64)
        stream = dev.stream_ptr(0)

        def kernels(p):
            hc.check(lib.iso_hier_lnlike(p._columns(None, 0, S), 3, _cabi.CHAIN_PARAM_MAJOR, T, S, W, 0, S, dev.ptr(irec),
                                         dev.ptr(rows), H, None, dev.ptr(ell), dev.ptr(ess), dev.ptr(n_bad), dev.ptr(L),
                                         dev.ptr(mn), stream))
        med, best = device_time([lambda p=p: kernels(p) for p in posts], reps)
        least = n_eval * OPS_PER_EVALUATION / PEAK_F64_VECTOR_OPS_PER_S
        kernels(posts[0])
        L_kernel = L.clone()
        emit(path="iso_hier_lnlike", median_s=med, min_s=best, evaluations_per_s=n_eval / med,
             f64_vector_ops_per_evaluation=OPS_PER_EVALUATION, least_time_vector_f64_s=least, share_of_vector_f64_bound=least / med,
             min_ess_median=float(mn.median().item()), bad_samples=int(n_bad.sum().item()), **shape)
        med_e, best_e = device_time([lambda p=p: p.lnlike(th) for p in posts], reps)
        emit(path="PopulationPosterior.lnlike", median_s=med_e, min_s=best_e, evaluations_per_s=n_eval / med_e, **shape)
        if H <= 64:
            L_fw = framework_route(chains[0], S, W, th, model, interim)
            scaled = ((L_fw - L_kernel).abs() / (1 + L_kernel.abs())).max().item()
            r_fw = max(3, reps // 10)
            med_f, best_f = device_time([lambda x=x: framework_route(x, S, W, th, model, interim) for x in chains], r_fw, warmup=1)
            emit(path="framework_ops", median_s=med_f, min_s=best_f, evaluations_per_s=n_eval / med_f,
                 intermediate_bytes_limit=FRAMEWORK_BYTES, max_scaled_difference_of_L_to_the_kernel=scaled,
                 speedup_of_iso_hier_lnlike=med_f / med, speedup_of_lnlike_end_to_end=med_f / med_e, **dict(shape, reps=r_fw))
        if (W, H) == (32, 64):
            fit_model = ia.PopulationModel(mass=model.families[0], feh=model.families[1])
            pp = ia.PopulationPosterior((_chain.from_storage(chains[0], S, W, False), NAMES), None, fit_model,
                                        interim={k: interim[k] for k in ("mass", "feh")})
            kw = dict(nwalkers=64, nburn=20, niter=20) if a.quick else dict(nwalkers=64, nburn=200, niter=200)
            pp.fit_mcmc(nwalkers=64, nburn=2, niter=2, seed=1)                        # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp = pp.fit_mcmc(seed=2, **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            df = pp.samples
            calls = 2 * (kw["nburn"] + kw["niter"]) + 1
            emit(path="fit_mcmc", wall_s=wall, lnlike_calls=calls, rows_per_call=32, s_per_call=wall / calls,
                 evaluations_per_s=calls * 32 * S * W * T / wall, parameters=list(fit_model.param_names),
                 acceptance=float(smp.acceptance_fraction.mean().item()), finite_lnprob=bool(np.isfinite(df["lnprob"]).all()),
                 S=S, W=W, T=T, **kw)
        del posts, rows, ell, ess
    out.close()


if __name__ == "__main__":
    main()
