#!/usr/bin/env python
"""Timing of the selection term of the hierarchical likelihood on one device, JSON lines appended to
profiles/selection/selection.jsonl:

* the ``iso_select_alpha`` kernels alone (libiso_select.so: k_select_partial + k_select_total) on prepared device records,
  workspace and outputs, between HIP events, median of ``--reps`` passes after warm-up, rotating over 8 distinct injection
  sets: J = 10^5 and 10^6 injections at H = 32, 64 and 1 024 hyper rows, three columns (those of tools/hier_timing.py:
  mass drawn from a Chabrier density with a power-law population, feh from ``FehPrior`` with a truncated Gaussian, age flat
  in age with a truncated Gaussian).  Reported: (injection, row) evaluations per second;
* in the same process, alternating with it pass by pass on the same sets, the only earlier route to the same number for
  0/1 detection: ``iso_hier_lnlike`` on the one-star chain made of the detected injections (plus ln(J_det / J) on the
  host); the ratio of the two medians, the spread of the passes of each (interquartile range), and the largest difference
  of the two results;
* ``PopulationPosterior.lnlike`` end to end with and without an injection set of 10^6 on the 10^4 x 32 x 100 catalog.

    python tools/selection_timing.py [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hier_timing as ht  # noqa: E402  (the model, the priors, the rows and the catalog chains of the section-17 timing)

#          J,       H
SHAPES = ((10 ** 5, 32), (10 ** 5, 64), (10 ** 5, 1024), (10 ** 6, 32), (10 ** 6, 64), (10 ** 6, 1024))
ROTATE = 8


def make_injections(J, seed, priors):
    """``(x [3, J] CUDA tensor, lnd [J])``: the three columns drawn on the host from their densities; 0/1 detection that
    keeps the more massive, younger and nearer half (a stand-in for a magnitude cut: what is timed does not depend on it)."""
    import torch
    rng = np.random.default_rng(seed)
    x = np.stack([np.asarray(priors[c].sample(J, rng), dtype=np.float64) for c in ht.NAMES])
    score = np.log(x[0]) - 0.3 * (x[2] - 9.0) + 0.2 * rng.normal(size=J)
    lnd = np.where(score > np.median(score), 0.0, -np.inf)
    return torch.from_numpy(x).cuda(), torch.from_numpy(lnd).cuda()


def alternating_times(fa, fb, reps, warmup=3):
    """Seconds of every pass of the calls ``fa[i]`` and ``fb[i]``, alternating a, b, a, b, ... and rotating over i."""
    import torch
    n = len(fa)
    for i in range(max(warmup, n)):
        fa[i % n]()
        fb[i % n]()
    torch.cuda.synchronize()
    out = ([], [])
    for i in range(reps):
        for k, fns in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[i % n]()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e-3)
    return np.array(out[0]), np.array(out[1])


def spread(t):
    q1, q2, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_s=float(q2), min_s=float(t.min()), iqr_s=float(q3 - q1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 rotating sets, J = 10^5 only, 10^3 stars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection", "selection.jsonl"))
    a = ap.parse_args()
    import torch
    import isochrones_amd as ia
    from isochrones_amd import _cabi, _chain, _hier_cabi as hc, _select_cabi as sc, device as dev
    if not torch.cuda.is_available():
        raise SystemExit("selection_timing needs a GPU: a CPU run says nothing about these paths")
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

    model, priors = ht.model_and_priors()
    draw = torch.from_numpy(np.concatenate([ia.hierarchical.prior_record(priors[c]) for c in ht.NAMES]).view(np.uint8).copy()).cuda()
    slib, hlib = sc.lib(), hc.lib()
    stream = dev.stream_ptr(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    sets, key = None, None
    for J, H in SHAPES:
        if a.quick and J > 10 ** 5:
            continue
        if key != J:
            del sets
            torch.cuda.empty_cache()
            sets, key = [make_injections(J, 200 + i, priors) for i in range(rotate)], J
            # the earlier route's input: the detected injections as one star of J_det walkers and one step, [1, 3, J_det]
            chains = [x[:, torch.isneginf(lnd).logical_not()].contiguous() for x, lnd in sets]
        th = ht.thetas(H)
        rows = torch.from_numpy(np.ascontiguousarray(model.pack(th)).view(np.uint8).reshape(-1)).cuda()
        ws = torch.empty(int(slib.iso_select_workspace_doubles(J, H)), **f64)
        la, ne, nb = torch.empty(H, **f64), torch.empty(H, **f64), torch.empty(1, dtype=torch.int32, device="cuda")
        ell, ess, n_bad = torch.empty(H, 1, **f64), torch.empty(H, 1, **f64), torch.empty(1, dtype=torch.int32, device="cuda")
        L, mn = torch.empty(H, **f64), torch.empty(H, **f64)

        def new(s):
            x, lnd = s
            sc.check(slib.iso_select_alpha(dev.ptr(x), 3, J, dev.ptr(lnd), dev.ptr(draw), dev.ptr(rows), H, dev.ptr(ws),
                                           dev.ptr(la), dev.ptr(ne), dev.ptr(nb), stream))

        def old(c):
            n = int(c.shape[1])
            cols = (hc.IsoHierColumn * 3)(*[hc.IsoHierColumn(c.data_ptr(), 3, q, 1, 0) for q in range(3)])
            hc.check(hlib.iso_hier_lnlike(cols, 3, _cabi.CHAIN_PARAM_MAJOR, 1, 1, n, 0, 1, dev.ptr(draw), dev.ptr(rows), H, None,
                                          dev.ptr(ell), dev.ptr(ess), dev.ptr(n_bad), dev.ptr(L), dev.ptr(mn), stream))

        t_new, t_old = alternating_times([lambda s=s: new(s) for s in sets], [lambda c=c: old(c) for c in chains], reps)
        new(sets[0])
        old(chains[0])
        shift = float(np.log(chains[0].shape[1] / J))
        d_alpha = float((la - (L + shift)).abs().max().item())
        d_neff = float(((ne - ess[:, 0]).abs() / ess[:, 0]).max().item())
        n_eval = J * H
        shape = dict(J=J, H=H, columns=list(ht.NAMES), evaluations=n_eval, rotating_sets=rotate, reps=reps,
                     chunks=-(-J // sc.CHUNK), workgroups=-(-J // sc.CHUNK) * -(-H // sc.ROW_TILE))
        s_new, s_old = spread(t_new), spread(t_old)
        emit(path="iso_select_alpha", evaluations_per_s=n_eval / s_new["median_s"], n_eff_median=float(ne.median().item()),
             bad_injections=int(nb.item()), **s_new, **shape)
        emit(path="iso_hier_lnlike on the one-star chain of detected injections", detected=int(chains[0].shape[1]),
             workgroups_of_this_route=-(-H // hc.ROW_TILE), **s_old, **dict(shape, workgroups=None))
        emit(path="ratio", earlier_route_over_iso_select_alpha=s_old["median_s"] / s_new["median_s"],
             difference_of_medians_s=s_old["median_s"] - s_new["median_s"], sum_of_iqr_s=s_old["iqr_s"] + s_new["iqr_s"],
             faster_by_more_than_the_spread=bool(s_old["median_s"] - s_new["median_s"] > s_old["iqr_s"] + s_new["iqr_s"]),
             max_abs_difference_of_ln_alpha=d_alpha, max_rel_difference_of_n_eff=d_neff, J=J, H=H)
    # lnlike end to end on the section-17 catalog, with and without the injections
    S, W, T, H = (10 ** 3 if a.quick else 10 ** 4), 32, 100, 32
    J = 10 ** 5 if a.quick else 10 ** 6
    del sets, chains
    torch.cuda.empty_cache()
    cats = [ht.make_chain(S, W, T, 100 + i) for i in range(rotate)]
    th = ht.thetas(H)
    x, lnd = make_injections(J, 200, priors)
    inj = ia.InjectionSet({c: x[q] for q, c in enumerate(ht.NAMES)}, priors, lnd)
    src = lambda c: (_chain.from_storage(c, S, W, False), ht.NAMES)
    plain = [ia.PopulationPosterior(src(c), None, model, interim=priors) for c in cats]
    with_sel = [ia.PopulationPosterior(src(c), None, model, interim=priors, injections=inj) for c in cats]
    t_with, t_plain = alternating_times([lambda p=p: p.lnlike(th) for p in with_sel], [lambda p=p: p.lnlike(th) for p in plain], reps)
    shape = dict(S=S, W=W, T=T, H=H, J=J, rotating_chains=rotate, reps=reps)
    emit(path="PopulationPosterior.lnlike with injections", **spread(t_with), **shape)
    emit(path="PopulationPosterior.lnlike without injections", **spread(t_plain), **shape)
    out.close()


if __name__ == "__main__":
    main()
