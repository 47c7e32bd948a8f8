#!/usr/bin/env python
"""Timing of iso_members_moments (StarClusterModel.star_moments) against iso_cluster_lnlike on the same inputs, on one device:
JSON lines with the shape, the kernels' time of each call between HIP events, and their ratio.

The two calls alternate pass by pass in one process, so that whatever else the device and the host are doing falls on both;
each pass takes the next of 8 row sets (other rows, the same shape), so that no pass finds its own inputs in the cache.  What
is timed is the C-ABI call alone (both kernels of each library): the columns are built before, once per row set.  The figure
is the ratio of the medians; the register counts and waves per SIMD of both pairs kernels come from the build's tables.

    python tools/members_timing.py [--quick] [--out FILE]      (default: profiles/members/members.jsonl)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOTEBOOK = [8.84, -0.2, 500.0, 0.03, -3.0, 0.3, 0.3]
SPREAD = [0.02, 0.03, 5.0, 0.01, 0.2, 0.05, 0.05]
ROW_SETS = 8
PASSES = 30


def _model(n_stars, seed, bands="gri", minq=0.5):
    import isochrones_amd as ia
    ic = ia.synthetic_isochrone(bands=tuple(bands))
    cat = ia.simulate_cluster(n_stars, *NOTEBOOK, bands=bands, ic=ic, seed=seed)
    cols = ["%s_mag" % b for b in bands]
    df = cat.df[np.isfinite(cat.df[cols].to_numpy()).all(axis=1)]
    return ia.StarClusterModel(ic, df, bands=list(bands), props=["parallax"], eep_bounds=(200, 700), minq=minq)


def time_shape(mod, n_rows, passes, rng):
    import torch
    from isochrones_amd import _cluster_cabi as CC, _members_cabi as MC, device as dev
    device = dev.current_device()
    d = torch.device("cuda", device)
    st = mod._device_state(device)
    ne = st["eeps"].numel()
    ns, nb, npr = len(mod.stars), len(mod.bands), len(mod.props)
    sets = []
    for i in range(ROW_SETS):
        rows = np.array(NOTEBOOK) + (np.array(SPREAD) * rng.standard_normal((n_rows, 7)) if n_rows > 1 or i else 0.0)
        x = torch.as_tensor(rows, dtype=torch.float64, device=d).reshape(n_rows, 7)
        sets.append(mod._chunk_columns(x, st, device))
    f64 = dict(dtype=torch.float64, device=d)
    work1 = torch.empty(n_rows * ns * ne, **f64)
    work6 = torch.empty(n_rows * ns * MC.NINNER * ne, **f64)
    tot, per_star = torch.empty(n_rows, **f64), torch.empty((n_rows, ns), **f64)
    ln_like, moments = torch.empty((n_rows, ns), **f64), torch.empty((n_rows, ns, MC.NMOM), **f64)
    stream = dev.stream_ptr(device)

    def like(cols, nv, rp):
        CC.check(CC.lib().iso_cluster_lnlike(dev.ptr(cols), ne, n_rows, dev.ptr(nv), dev.ptr(rp), dev.ptr(st["val"]),
                                             dev.ptr(st["w"]), ns, nb, npr, mod.minq, dev.ptr(work1), dev.ptr(tot),
                                             dev.ptr(per_star), stream))

    def members(cols, nv, rp):
        MC.check(MC.lib().iso_members_moments(dev.ptr(cols), ne, n_rows, dev.ptr(nv), dev.ptr(rp), dev.ptr(st["val"]),
                                              dev.ptr(st["w"]), ns, nb, npr, mod.minq, dev.ptr(work6), dev.ptr(ln_like),
                                              dev.ptr(moments), stream))

    def timed(fn, args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    for args in sets[:2]:                                   # warm-up: code objects, first launches
        like(*args)
        members(*args)
    torch.cuda.synchronize()
    t_like, t_mem = [], []
    for i in range(passes):
        args = sets[i % ROW_SETS]
        t_like.append(timed(like, args))
        t_mem.append(timed(members, args))
    same = bool(torch.equal(per_star.view(torch.int64), ln_like.view(torch.int64)))     # the last pass: the same row set
    n_valid = float(torch.stack([s[1] for s in sets]).double().mean())
    kl, km = float(np.median(t_like)), float(np.median(t_mem))
    return dict(case="notebook_%drows" % n_rows, stars=ns, bands=nb, props=npr, eeps=int(ne), valid_eeps=n_valid,
                rows=int(n_rows), passes=passes, row_sets=ROW_SETS, likelihood_s=kl, members_s=km,
                ratio_members_over_likelihood=km / kl, likelihood_min_s=float(np.min(t_like)),
                members_min_s=float(np.min(t_mem)), ln_like_same_bits=same, device=torch.cuda.get_device_name(device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="6 passes, no 1 024-row shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members", "members.jsonl"))
    a = ap.parse_args()
    import torch
    from isochrones_amd.csrc import libraries
    assert torch.cuda.is_available(), "members_timing needs a GPU"
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = {spec.name: spec.resource_table() for spec in (libraries.CLUSTER, libraries.MEMBERS)}
    build = {k: {f: res[lib][k][f] for f in ("vgpr", "sgpr", "waves", "scratch")}
             for lib, k in (("cluster", "k_cluster_pairs"), ("members", "k_members_pairs"), ("members", "k_members_finish"))}
    mod = _model(50, seed=1)
    rng = np.random.default_rng(0)
    with open(a.out, "w") as out:
        for n_rows in (1, 256) if a.quick else (1, 256, 1024):
            rec = time_shape(mod, n_rows, 6 if a.quick else PASSES, rng)
            rec["build"] = build
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
