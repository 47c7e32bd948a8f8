"""fit_stars_nested_gpu / fit_catalog(method="nested") / select_multiplicity on the device (libiso_nested.so,
isochrones_amd/csrc/nested/nested_kernel.h): a device fit replayed macro-step by macro-step from what it stored, against the
CPU oracle's lnpost and the numpy twin's ellipsoid and random numbers; the bookkeeping recomputed from the dead points; the
evidences against the existing per-star route (fit_multinest); invariance, failure isolation, model selection; and every
instantiation the library compiles launched once."""
import os

import numpy as np
import pytest

import isochrones_amd as ia
from isochrones_amd.catalog import StarCatalog, fit_stars_nested_gpu, nested_result_columns
from tests import _fixtures as fx
from tests import _nested_twin as T

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def small_ic(kind, bands):
    fehs = np.array([-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5])
    if kind == "track":
        masses = ia.grids.mist_masses()[20:150:3]
        eeps = np.arange(200.0, 700.0)
        return ia.synthetic_track(bands=bands, fehs=fehs, masses=masses, eeps=eeps, eep_bounds=(eeps[0], eeps[-1]),
                                  limits=dict(mass=(masses[0], masses[-1]), feh=(-2.0, 0.5), age=(5, 10.13)))
    ages = ia.grids.mist_log_ages()[40::3]
    eeps = np.arange(150.0, 700.0)
    return ia.synthetic_isochrone(bands=bands, ages=ages, fehs=fehs, eeps=eeps, eep_bounds=(eeps[0], eeps[-1]),
                                  limits=dict(age=(ages[0], ages[-1]), feh=(-2.0, 0.5)))


def replay_star(ex, row, s, desc, oic, seed, gidx, nlive, D, steps=None):
    """Teacher-forced replay of star ``s`` of a ``return_dead=True`` fit.  For every macro-step (or the first ``steps``), from
    the live set the STORED dead points define:

    (a) the twin's ellipsoid of the survivors against the stored one.  Bound: the device sums the same numbers in another
        order and with fused multiply-adds; how much that can move the factor is set by the conditioning of the Cholesky
        factor, which is measured per step as the distance between the twin in float64 and in long double (64-bit
        mantissa).  Allowed: 64 x that distance + 64 ulp of the largest entry - the multiple covers the up to 29 sums of
        ~n/9 terms whose order differs; printed per star as the worst ratio seen;
    (b) every consumed draw index regenerates, from Philox and the STORED ellipsoid, a point; the accepted ones must be
        stored points to 2^-44: u = mean + A z has D + 1 terms; z is a unit vector times a radius <= 1 whose components carry
        the few ulp by which the device's log / sincospi / exp and fused multiply-adds differ from libm's and from 2 pi u
        rounded (the argument of tests/_replay.py:65-70), <= 16 ulp each; the rows of A of an enlarged ellipsoid sum to a
        few units - 256 ulp of 1;
    (c) their stored logl is the oracle's lnpost (rtol 1e-9, atol 1e-11);
    (d) every draw skipped in between is outside the cube, non-finite or <= thr by the oracle, every accepted one > thr,
        except near ties |logl - thr| < 1e-9 (1 + |logl| + |thr|), which are counted and returned with the number of
        replayed draws."""
    K = ex["K"]
    n_dead, n_steps = int(ex["n_dead"][s]), int(ex["n_steps"][s])
    du, dl = ex["dead_u"][s, :n_dead], ex["logl"][s, :n_dead]
    lo, hi = ex["lo"][s], ex["hi"][s]
    span = hi - lo
    assert np.all(np.diff(dl) >= 0)

    def oracle(u):
        ll = oic.lnpost(desc, np.ascontiguousarray((lo + u * span).T), nthreads=8, parts=False)
        return np.where(np.isfinite(ll), ll, -np.inf)

    # the fill: exact unit-cube draws; held = the first nlive with a finite oracle lnpost, and they are stored points
    fill_chunks = int(round(ex["trace"][s, 0, 1])) // T.BLOCK if n_steps else None
    assert fill_chunks is not None and fill_chunks >= 1
    u = T.fill_draws(seed, gidx, np.repeat(np.arange(fill_chunks), T.BLOCK), D, np.tile(np.arange(T.BLOCK), fill_chunks))
    ll = oracle(u)
    fin = ll > -np.inf
    assert abs(fin.sum() / (fill_chunks * T.BLOCK) - row[2 * D + 5]) < 1e-15          # prior_fraction
    live_u, live_l = u[fin][:nlive], ll[fin][:nlive]
    assert live_l.size == nlive
    stored = {tuple(r): l for r, l in zip(du, dl)}
    got_l = np.array([stored[tuple(r)] for r in live_u])                                # KeyError: a fill point that was never stored
    np.testing.assert_allclose(got_l, live_l, rtol=1e-9, atol=1e-11)
    live_l = got_l                                                                      # teacher forcing: the stored values decide
    order = np.argsort(live_l, kind="stable")
    live_u, live_l = live_u[order], live_l[order]
    near, replayed, worst_ratio, worst_match = 0, 0, 0.0, 0.0
    for m in range(n_steps if steps is None else min(steps, n_steps)):
        tr = ex["trace"][s, m]
        thr, first, last = tr[0], int(round(tr[1])), int(round(tr[2]))
        mean_d, A_d = tr[3:3 + D], tr[3 + D:].reshape(D, D)
        assert np.array_equal(live_u[:K], du[m * K:(m + 1) * K]) and np.array_equal(live_l[:K], dl[m * K:(m + 1) * K])
        assert thr == live_l[K - 1]
        sv_u, sv_l = live_u[K:], live_l[K:]
        # (a)
        mean64, A64 = T.bounding_ellipsoid(sv_u, 1.5)
        meanL, AL = T.bounding_ellipsoid(sv_u, 1.5, dtype=np.longdouble)
        cond = float(np.max(np.abs(A64 - AL))) + float(np.max(np.abs(mean64 - meanL)))
        tol = 64 * cond + 64 * EPS * float(np.max(np.abs(A64)))
        err = max(float(np.max(np.abs(A_d - A64))), float(np.max(np.abs(mean_d - mean64))))
        worst_ratio = max(worst_ratio, err / max(cond, EPS * float(np.max(np.abs(A64)))))
        assert err <= tol, (m, err, tol)
        # (b) - (d)
        assert first % T.BLOCK == 0 and last >= first
        idx = np.arange(first, last + 1)
        x, inside = T.ellipsoid_draws(seed, gidx, idx // T.BLOCK, mean_d, A_d, idx % T.BLOCK)
        ll = np.full(idx.size, -np.inf)
        if inside.any():
            ll[inside] = oracle(x[inside])
        tie = inside & np.isfinite(ll) & (np.abs(ll - thr) < 1e-9 * (1 + np.abs(ll) + abs(thr)))
        near += int(tie.sum())
        replayed += int(idx.size)
        # the points the device accepted: the K stored points born in this step = the next live set minus the survivors
        born = []
        sv_set = {tuple(r) for r in sv_u}
        nxt = du[(m + 1) * K:]                                      # every later dead point that is not a survivor of this step
        # candidates by proximity: an accepted draw must be a stored point to 2^-44
        acc_idx = []
        for j in np.nonzero(inside & (ll > -np.inf) & ((ll > thr) | tie))[0]:
            d = np.max(np.abs(nxt - x[j]), axis=1)
            k = int(np.argmin(d))
            if d[k] <= 2.0 ** -44 and tuple(nxt[k]) not in sv_set:
                acc_idx.append(j)
                born.append(k)
                worst_match = max(worst_match, float(d[k]))
        acc_idx = np.array(acc_idx, dtype=int)
        assert acc_idx.size == K, (m, acc_idx.size, K)
        assert idx[acc_idx[-1]] == last
        new_u, new_l = nxt[born], dl[(m + 1) * K:][born]
        np.testing.assert_allclose(new_l, ll[acc_idx], rtol=1e-9, atol=1e-11)              # (c)
        accepted = np.zeros(idx.size, dtype=bool)
        accepted[acc_idx] = True
        assert np.all((ll[accepted] > thr) | tie[accepted])                                # (d)
        assert np.all(~inside[~accepted] | ~(ll[~accepted] > thr) | tie[~accepted])
        all_u, all_l = np.vstack([sv_u, new_u]), np.concatenate([sv_l, new_l])
        order = np.argsort(all_l, kind="stable")
        live_u, live_l = all_u[order], all_l[order]
    return near, replayed, worst_ratio, worst_match


def check_bookkeeping(ex, row, s, nlive, D):
    """lnZ, H, lnZ_err and the moments recomputed from the stored dead points.  The device's streamed sums and these sums add
    the same n_dead terms of one sign in another order: relative round-off n_dead 2^-52 x 8 (as in
    tests/test_nested_catalog_cpu.py::test_streamed_moments_equal_the_dead_points_moments; the factor covers exp() of the
    device against libm's, a few ulp per term)."""
    n = int(ex["n_dead"][s])
    K = ex["K"]
    logwt, logl, th = ex["logwt"][s, :n], ex["logl"][s, :n], ex["dead"][s, :n]
    bound = n * EPS * 8
    lnz = np.logaddexp.reduce(logwt)
    w = np.exp(logwt - lnz)
    frac = row[2 * D + 5]
    assert abs(row[2 * D] - np.log(frac) - lnz) <= bound * (1 + abs(lnz))
    h = max(w @ logl - lnz, 0.0)
    assert abs(row[2 * D + 2] - h) <= bound * (w @ np.abs(logl) + abs(lnz))
    assert abs(row[2 * D + 1] - np.sqrt(row[2 * D + 2] / nlive)) <= 4 * EPS * row[2 * D + 1]
    mean, std = row[0:2 * D:2], row[1:2 * D:2]
    m = w @ th
    ex2 = w @ th ** 2
    assert np.all(np.abs(mean - m) <= bound * (w @ np.abs(th)))
    assert np.all(np.abs(std ** 2 + mean ** 2 - ex2) <= 2 * bound * ex2)
    niter, n_steps = int(row[2 * D + 4]), int(ex["n_steps"][s])
    assert niter == (n_steps + 1) * K and n == niter + nlive - K
    assert np.all(np.diff(logl) >= 0)
    tr = ex["trace"][s, :n_steps]
    assert np.all(tr[:, 2] >= tr[:, 1]) and np.all(np.diff(tr[:, 1]) > 0) and np.all(tr[1:, 1] > tr[:-1, 2])
    # ncall: every fill draw, and at most every draw examined afterwards (those outside the cube are not evaluated)
    fill = tr[0, 1]
    examined = (np.floor(tr[:, 2] / T.BLOCK) + 1) * T.BLOCK - tr[:, 1]
    assert fill + K * n_steps <= row[2 * D + 3] <= fill + examined.sum()


def _fit(cat, ic, idx, N, nlive, seed, **kw):
    return fit_stars_nested_gpu(cat, ic, np.asarray(idx), N=N, n_live_points=nlive, seed=seed, return_dead=True, **kw)


@pytest.mark.parametrize("kind,ns,nb", [("track", 1, 3), ("track", 1, 6), ("iso", 1, 3), ("iso", 1, 6), ("iso", 2, 3), ("iso", 2, 6)])
def test_teacher_forced_replay_against_the_oracle(kind, ns, nb):
    bands = list(ia.grids.KNOWN_BANDS[:nb])
    ic = small_ic(kind, bands)
    S, nlive, seed, D = 20, 100, 77 + nb, ns + 4
    cat, _ = ia.synthetic_catalog(ic, S, bands=bands, seed=5 + nb, mag_unc=0.02, with_parallax=True)
    rows, ex = _fit(cat, ic, np.arange(S), ns, nlive, seed)
    assert ex["kernel"] == "k_catalog_nested<%d, %d, %d>" % (0 if kind == "track" else 1, ns, nb)
    oic = fx.make_oracle_ic(ic)
    near = replayed = n_ok = 0
    assert np.all(rows[:, -1] == 1), rows[:, -2:]                # stars drawn from the model itself: every one is fitted
    for s in range(S):
        n_ok += 1
        desc = cat.model(s, ic, N=ns).model_desc()
        a, b, ratio, match = replay_star(ex, rows[s], s, desc, oic, seed, s, nlive, D)
        check_bookkeeping(ex, rows[s], s, nlive, D)
        print("%s N=%d nb=%d star %d: lnZ %.3f +- %.3f niter %d ncall %d near ties %d of %d, ellipsoid error / conditioning %.2f, worst match %.2e"
              % (kind, ns, nb, s, rows[s, 2 * D], rows[s, 2 * D + 1], rows[s, 2 * D + 4], rows[s, 2 * D + 3], a, b, ratio, match))
        near += a
        replayed += b
    assert n_ok == S
    assert near <= 1e-3 * replayed, (near, replayed)
    ic.release()


def test_bookkeeping_at_the_reference_default_of_1000_live_points():
    bands = ["G", "BP", "RP"]
    ic = small_ic("track", bands)
    cat, _ = ia.synthetic_catalog(ic, 6, bands=bands, seed=2, mag_unc=0.02)
    assert ia.nested_max_live(cat, ic) >= 1000
    rows, ex = _fit(cat, ic, np.arange(6), 1, 1000, 3)
    assert np.all(rows[:, -1] == 1), rows[:, -2:]
    for s in range(6):
        check_bookkeeping(ex, rows[s], s, 1000, 5)
    with pytest.raises(ValueError, match="above"):
        fit_stars_nested_gpu(cat, ic, np.arange(6), n_live_points=ia.nested_max_live(cat, ic) + 1)
    ic.release()


def test_evidence_agrees_with_fit_multinest():
    """lnZ of the catalog fit against SingleStarModel.fit_multinest (host loop, another random stream), bounds of
    tests/test_nested_cpu.py: |dlnZ| < 4 sqrt(err1^2 + err2^2) + 0.08, means within 0.15 sigma of the host fit.  The host route
    is run twice (seeds 0, 1): its self-agreement is printed next to each star."""
    bands = ["G", "BP", "RP"]
    ic = small_ic("track", bands)
    S, nlive = 30, 400
    cat, _ = ia.synthetic_catalog(ic, S, bands=bands, seed=8, mag_unc=0.02)
    rows = fit_stars_nested_gpu(cat, ic, np.arange(S), n_live_points=nlive, seed=1)
    D = 5
    assert np.all(rows[:, -1] == 1)
    bad = []
    for s in range(S):
        mod = cat.model(s, ic)
        h0 = mod.fit_multinest(n_live_points=nlive, seed=0)
        h1 = mod.fit_multinest(n_live_points=nlive, seed=1)
        m0 = h0.weights @ h0.samples
        s0 = np.sqrt(h0.weights @ (h0.samples - m0) ** 2)
        dz, ez = rows[s, 2 * D] - h0.logz, np.hypot(rows[s, 2 * D + 1], h0.logz_err)
        dm = np.max(np.abs(rows[s, 0:2 * D:2] - m0) / s0)
        self_dz = h1.logz - h0.logz
        self_dm = np.max(np.abs(h1.weights @ h1.samples - m0) / s0)
        print("star %d: lnZ device %.3f +- %.3f host %.3f +- %.3f (host seed 1: %+.3f) | mean shift %.3f sigma (host self %.3f)"
              % (s, rows[s, 2 * D], rows[s, 2 * D + 1], h0.logz, h0.logz_err, self_dz, dm, self_dm))
        if not (abs(dz) < 4 * ez + 0.08 and dm < 0.15):
            bad.append(s)
    assert not bad, bad
    ic.release()


_WORLD = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[2])
import isochrones_amd as ia
from tests.test_gpu_nested_catalog import small_ic
dist.init_process_group("gloo")
torch.cuda.set_device(0)
bands = ["G", "BP", "RP"]
ic = small_ic("track", bands)
cat, _ = ia.synthetic_catalog(ic, 12, bands=bands, seed=4, mag_unc=0.02)
res = ia.fit_catalog(cat, ic, method="nested", n_live_points=100, seed=6)
res.to_pickle(os.path.join(sys.argv[1], "res%d.pkl" % dist.get_rank()))
dist.destroy_process_group()
'''


def test_a_row_does_not_depend_on_the_batch_the_rank_or_the_run(tmp_path):
    import socket
    import subprocess
    import sys
    import pandas as pd
    bands = ["G", "BP", "RP"]
    ic = small_ic("track", bands)
    cat, _ = ia.synthetic_catalog(ic, 12, bands=bands, seed=4, mag_unc=0.02)
    full = fit_stars_nested_gpu(cat, ic, np.arange(12), n_live_points=100, seed=6)
    again = fit_stars_nested_gpu(cat, ic, np.arange(12), n_live_points=100, seed=6)
    assert np.array_equal(full, again, equal_nan=True)
    assert np.all(full[:, -1] == 1), full[:, -2:]
    alone = fit_stars_nested_gpu(cat, ic, np.array([7]), n_live_points=100, seed=6)
    assert np.array_equal(alone[0], full[7], equal_nan=True)
    some = fit_stars_nested_gpu(cat, ic, np.array([9, 2, 7]), n_live_points=100, seed=6)
    assert np.array_equal(some, full[[9, 2, 7]], equal_nan=True)
    other = fit_stars_nested_gpu(cat, ic, np.array([7]), n_live_points=100, seed=7)
    assert not np.array_equal(other[0], full[7], equal_nan=True)
    one = ia.fit_catalog(cat, ic, method="nested", n_live_points=100, seed=6)
    assert list(one.columns) == nested_result_columns(ic.param_names)
    assert np.array_equal(one.to_numpy(), full, equal_nan=True)
    # two ranks sharing the one GPU (fresh child processes)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "world.py"
    script.write_text(_WORLD)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script), str(tmp_path), root]
    r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r0, r1 = pd.read_pickle(tmp_path / "res0.pkl"), pd.read_pickle(tmp_path / "res1.pkl")
    assert r0.equals(r1)
    assert np.array_equal(r0.to_numpy(), full, equal_nan=True)
    ic.release()


def test_a_star_without_support_fails_alone():
    """A star whose magnitudes are finite but 10^200 mag from anything a model can produce: the squared residual of every
    photometric term overflows, so lnlike - and lnpost - is -inf at every point of its box.  Its workgroup finds no live
    point within max_fill_chunks chunks and reports status 1; the rows of its neighbours are, bit for bit, those of the
    run without it."""
    bands = ["G", "BP", "RP"]
    ic = small_ic("track", bands)
    D = 5
    cat, _ = ia.synthetic_catalog(ic, 8, bands=bands, seed=12, mag_unc=0.02)
    base = fit_stars_nested_gpu(cat, ic, np.arange(8), n_live_points=100, seed=2, max_fill_chunks=64)
    assert np.all(base[:, -1] == 1), base[:, -2:]
    df = cat.df.copy()
    for b in bands:
        df.loc[df.index[3], "%s_mag" % b] = 1.0e200
    bad = StarCatalog(df, bands=bands, props=list(cat.props))
    rows, ex = fit_stars_nested_gpu(bad, ic, np.arange(8), n_live_points=100, seed=2, max_fill_chunks=64, return_dead=True)
    keep = np.arange(8) != 3
    assert np.array_equal(rows[keep], base[keep])
    assert rows[3, -1] == 0 and rows[3, 2 * D + 6] == 1                       # ok = 0, status "no support"
    assert np.isnan(rows[3, :2 * D + 3]).all()                                # moments, lnZ, lnZ_err, H
    assert rows[3, 2 * D + 3] == 64 * 256 and rows[3, 2 * D + 4] == 0 and rows[3, 2 * D + 5] == 0      # ncall, niter, prior_fraction
    assert ex["n_dead"][3] == 0 and ex["n_steps"][3] == 0 and np.all(ex["n_dead"][keep] > 0)
    # through fit_catalog the row reads the same
    out = ia.fit_catalog(bad, ic, method="nested", n_live_points=100, seed=2, max_fill_chunks=64)
    assert out["ok"].to_numpy().tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and np.isnan(out["lnZ"].iloc[3])
    # no support found within the fill budget: one chunk of 256 draws cannot hold 400 live points - every star reports it
    none = fit_stars_nested_gpu(cat, ic, np.arange(8), n_live_points=400, seed=2, max_fill_chunks=1)
    assert np.all(none[:, -1] == 0) and np.all(none[:, 2 * D + 6] == 1) and np.isnan(none[:, :2 * D + 3]).all()
    assert np.all(none[:, 2 * D + 3] == 256) and np.all(none[:, 2 * D + 4] == 0)
    ic.release()


def test_fast_args_export_checks_its_arguments():
    """iso_catalog_fast_args (the one export libiso_hip.so gained) on a real catalog: a wrong size is refused with the
    size message, the right size copies the block and reports the catalog's shape."""
    import ctypes as C
    from isochrones_amd import _cabi, _nested_cabi as NC
    from isochrones_amd.catalog import CatalogPosterior
    bands = ["G", "BP", "RP"]
    ic = small_ic("iso", bands)
    cat, _ = ia.synthetic_catalog(ic, 4, bands=bands, seed=1, mag_unc=0.02)
    post = CatalogPosterior.from_catalog(cat, ic, N=2)
    L = _cabi.lib()
    size = int(NC.lib().iso_nested_fast_args_size())
    buf = C.create_string_buffer(size + 8)
    kind, ns, nb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    for wrong in (size - 8, size + 8, 0):
        assert L.iso_catalog_fast_args(post._h, buf, wrong, C.byref(kind), C.byref(ns), C.byref(nb)) == -1
        assert b"size" in L.iso_last_error()
        assert (kind.value, ns.value, nb.value) == (-1, -1, -1) and buf.raw == bytes(size + 8)
    assert L.iso_catalog_fast_args(post._h, None, size, None, None, None) == -1
    assert L.iso_catalog_fast_args(post._h, buf, size, C.byref(kind), C.byref(ns), C.byref(nb)) == 0
    assert (kind.value, ns.value, nb.value) == (1, 2, 3) and buf.raw[:size] != bytes(size)
    assert L.iso_catalog_fast_args(post._h, buf, size, None, None, None) == 0
    assert NC.lib().iso_nested_max_live_catalog(buf, size, 2, 3) >= 400
    post.close()
    ic.release()


def test_select_multiplicity():
    bands = ["G", "BP", "RP"]
    ic = small_ic("iso", bands)
    cat, _ = ia.synthetic_catalog(ic, 10, bands=bands, seed=6, mag_unc=0.02)
    sel = ia.select_multiplicity(cat, ic, Ns=(1, 2), n_live_points=100, seed=3)
    assert list(sel.columns) == ["lnZ_1", "lnZ_err_1", "lnZ_2", "lnZ_err_2", "best_N", "dlnZ"] and len(sel) == 10
    assert sel.index.equals(cat.df.index)
    ok = np.isfinite(sel["lnZ_1"]) & np.isfinite(sel["lnZ_2"])
    assert ok.all(), sel
    assert set(sel["best_N"][ok]) <= {1, 2} and np.all(sel["dlnZ"][ok] >= 0)
    one = ia.fit_catalog(cat, ic, N=1, method="nested", n_live_points=100, seed=3)
    assert np.array_equal(sel["lnZ_1"].to_numpy(), one["lnZ"].to_numpy(), equal_nan=True)
    assert np.array_equal(sel["lnZ_err_1"].to_numpy(), one["lnZ_err"].to_numpy(), equal_nan=True)
    print(sel)
    ic.release()


def test_every_instantiation_is_launched_and_replayed():
    """Every (parametrisation, stars, bands) kernel of libiso_nested.so, by name, on a 4-star catalog with 40 live points; the
    first two macro-steps of every fitted star are replayed against the oracle."""
    from isochrones_amd.csrc.libraries import NESTED as B
    launched = set()
    seed, nlive = 31, 40
    for nb in range(1, 13):
        bands = list(ia.grids.KNOWN_BANDS[:nb])
        for kind, multiplicities in (("track", (1,)), ("iso", (1, 2, 3))):
            ic = small_ic(kind, bands)
            oic = fx.make_oracle_ic(ic)
            cat, _ = ia.synthetic_catalog(ic, 4, bands=bands, seed=40 + nb, mag_unc=0.02)
            for ns in multiplicities:
                rows, ex = _fit(cat, ic, np.arange(4), ns, nlive, seed, max_iter=40 * nlive)
                launched.add(ex["kernel"])
                assert ex["kernel"] == "k_catalog_nested<%d, %d, %d>" % (0 if kind == "track" else 1, ns, nb)
                assert np.all(rows[:, -1] == 1), (kind, ns, nb, rows[:, -2:])
                for s in range(2):
                    replay_star(ex, rows[s], s, cat.model(int(s), ic, N=ns).model_desc(), oic, seed, int(s), nlive, ns + 4, steps=2)
                    check_bookkeeping(ex, rows[s], s, nlive, ns + 4)
            ic.release()
    assert launched == set(B.KERNELS)
