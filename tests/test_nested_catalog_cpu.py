"""The catalog nested sampler without a GPU: its numpy twin (tests/_nested_twin.py - the same algorithm text, the same
Philox stream) on analytic likelihoods, libiso_nested.so's build, gates and argument checks, and the unchanged digest of
an MCMC catalog shard."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import _nested_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss(mu, sig):
    mu, sig = np.asarray(mu, float), np.asarray(sig, float)

    def f(x):
        return -0.5 * np.sum(((x - mu) / sig) ** 2, axis=1)
    return f


def _moments(res):
    w = np.exp(res["logwt"] - res["logwt"].max())
    w /= w.sum()
    m = w @ res["dead"]
    return w, m, np.sqrt(w @ (res["dead"] - m) ** 2)


# ---- 1. the algorithm on analytic cases: the bounds of tests/test_nested_cpu.py::test_batched_variant_same_integral ----
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_gaussian_evidence_and_posterior(seed):
    d = 5
    mu = np.array([0.3, 0.5, 0.6, 0.45, 0.7]) * 10 - 2          # box [-2, 8]^5
    sig = np.array([0.3, 0.5, 0.2, 0.4, 0.6])
    res = T.nested_fit(_gauss(mu, sig), [-2.0] * d, [8.0] * d, nlive=600, gidx=11, seed=seed)
    want = np.sum(np.log(np.sqrt(2 * np.pi) * sig)) - d * np.log(10.0)
    print("gaussian seed %d: lnZ %.4f want %.4f err %.4f niter %d ncall %d" % (seed, res["lnZ"], want, res["lnZ_err"], res["niter"], res["ncall"]))
    assert res["status"] == 0
    assert abs(res["lnZ"] - want) < 4 * res["lnZ_err"] + 0.08, (res["lnZ"], want, res["lnZ_err"])
    assert np.all(np.abs(res["mean"] - mu) < 0.15 * sig) and np.all(np.abs(res["std"] / sig - 1) < 0.15)
    assert np.all(np.diff(res["logl"]) >= 0)                    # the dead points come out in order


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_half_excluded_box(seed):
    sig = np.array([0.05, 0.08, 0.04])
    g = _gauss([0.5, 0.5, 0.5], sig)

    def f(x):
        ll = g(x)
        ll[x[:, 0] < 0.5] = -np.inf
        ll[x[:, 1] > 0.9] = np.nan
        return ll
    res = T.nested_fit(f, [0, 0, 0], [1, 1, 1], nlive=500, gidx=3, seed=seed)
    want = np.sum(np.log(np.sqrt(2 * np.pi) * sig)) + np.log(0.5)
    print("half box seed %d: lnZ %.4f want %.4f err %.4f frac %.3f" % (seed, res["lnZ"], want, res["lnZ_err"], res["prior_fraction"]))
    assert abs(res["lnZ"] - want) < 4 * res["lnZ_err"] + 0.08, (res["lnZ"], want)
    assert 0.3 < res["prior_fraction"] < 0.6
    assert np.all(res["dead"][:, 0] >= 0.5) and np.all(res["dead"][:, 1] <= 0.9)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_two_modes(seed):
    sg = 0.03
    a, b = _gauss([0.25, 0.3], [sg, sg]), _gauss([0.75, 0.7], [sg, sg])
    res = T.nested_fit(lambda x: np.logaddexp(a(x), b(x) + np.log(3.0)), [0, 0], [1, 1], nlive=800, gidx=5, seed=seed)
    want = np.log(4.0 * 2 * np.pi * sg * sg)
    w, _, _ = _moments(res)
    share = w[res["dead"][:, 0] > 0.5].sum()
    print("two modes seed %d: lnZ %.4f want %.4f err %.4f share %.3f" % (seed, res["lnZ"], want, res["lnZ_err"], share))
    assert abs(res["lnZ"] - want) < 4 * res["lnZ_err"] + 0.08
    assert abs(share - 0.75) < 0.07


def test_twin_no_support_is_a_status_not_an_exception():
    res = T.nested_fit(lambda x: np.full(x.shape[0], -np.inf), [0, 0], [1, 1], nlive=50, max_fill_chunks=8)
    assert res["status"] == 1 and res["prior_fraction"] == 0.0 and res["ncall"] == 8 * T.BLOCK


# ---- 2. streamed moments = moments of the dead points ----
def test_streamed_moments_equal_the_dead_points_moments():
    """The streamed sums and the sums over the stored dead points add the same n_dead non-negative terms w_i f_i in another
    order and with another reference exponent.  A sum of n terms of one sign carries a relative round-off of at most
    (n - 1) 2^-53 per ordering (Higham, Accuracy and Stability, eq. 4.4), each term's weight exp(t - R) another few ulp
    (one subtraction, one exp, one rescaling per macro-step that raised R: bounded by 4 ulp per rescaling, at most
    n_steps of them).  Bound asserted on S_f / S_0 for f = 1, logl, theta, theta^2: n_dead * 2^-52 * 8 relative to
    sum w |f| / sum w."""
    d = 5
    mu = np.array([0.3, 0.5, 0.6, 0.45, 0.7]) * 10 - 2
    sig = np.array([0.3, 0.5, 0.2, 0.4, 0.6])
    res = T.nested_fit(_gauss(mu, sig), [-2.0] * d, [8.0] * d, nlive=400, gidx=2, seed=4)
    n = res["logl"].size
    bound = n * 2.0 ** -52 * 8
    w, m, s = _moments(res)
    ex2 = w @ res["dead"] ** 2
    lnz = np.logaddexp.reduce(res["logwt"])
    h = w @ res["logl"] - lnz
    print("n_dead %d bound %.2e: mean %.2e second moment %.2e lnZ %.2e H %.2e" % (
        n, bound, np.max(np.abs(res["mean"] - m) / (w @ np.abs(res["dead"]))),
        np.max(np.abs(res["std"] ** 2 + res["mean"] ** 2 - ex2) / ex2), abs(res["lnZ"] - np.log(res["prior_fraction"]) - lnz),
        abs(res["H"] - h)))
    assert np.all(np.abs(res["mean"] - m) <= bound * (w @ np.abs(res["dead"])))
    assert np.all(np.abs(res["std"] ** 2 + res["mean"] ** 2 - ex2) <= 2 * bound * ex2)     # (mean^2 enters with its own error)
    assert abs(res["lnZ"] - np.log(res["prior_fraction"]) - lnz) <= bound * (1 + abs(lnz))
    assert abs(res["H"] - h) <= bound * (w @ np.abs(res["logl"]) + abs(lnz))


# ---- 3. a star's stream is keyed by its global index ----
def test_star_index_keying_is_independent_of_the_batch():
    mu, sig = np.array([0.4, 0.6, 0.5]), np.array([0.05, 0.08, 0.04])
    g = _gauss(mu, sig)
    alone = T.nested_fit(g, [0, 0, 0], [1, 1, 1], nlive=100, gidx=7, seed=9)
    batch = [T.nested_fit(g, [0, 0, 0], [1, 1, 1], nlive=100, gidx=k, seed=9) for k in range(20)]
    for key in ("lnZ", "lnZ_err", "H", "ncall", "niter", "prior_fraction"):
        assert alone[key] == batch[7][key], key
    for key in ("mean", "std", "dead_u", "logl", "logwt"):
        assert np.array_equal(alone[key], batch[7][key]), key
    assert len({b["lnZ"] for b in batch}) == 20                 # and the stars do differ
    hi = T.nested_fit(g, [0, 0, 0], [1, 1, 1], nlive=100, gidx=7 + (1 << 32), seed=9)
    assert hi["lnZ"] != alone["lnZ"]                            # the high word of the index enters the counter


# ---- 4. the library ----
def _built():
    from isochrones_amd.csrc.libraries import NESTED as B
    path = B.build()
    assert os.path.exists(path) and B.up_to_date()
    return path


def test_library_header_symbols_are_exported():
    path = _built()
    text = open(os.path.join(ROOT, "include", "isochrones_amd_nested.h")).read()
    syms = set(re.findall(r"\b(iso_nested_\w+)\s*\(", text))
    from isochrones_amd import _nested_cabi
    assert syms == set(_nested_cabi.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(path)          # host code only: loading it needs no device
    for s in syms:
        getattr(lib, s)


def test_library_kernel_set_and_gates():
    from isochrones_amd.csrc.libraries import NESTED as B
    _built()
    table = B.resource_table()
    want = {"k_catalog_nested<%d, %d, %d>" % (kind, ns, nb) for kind, ns in ((0, 1), (1, 1), (1, 2), (1, 3)) for nb in range(1, 13)}
    assert set(table) == want == set(B.KERNELS)
    for name, r in table.items():
        assert r["agpr"] == 0 and r["vgpr"] <= 256 and r["waves"] >= 2, (name, r)
        assert r["scratch"] <= B.SCRATCH_BUDGET["k_catalog_nested"], (name, r)
        if "<1, 3," not in name and name != "k_catalog_nested<1, 2, 12>":
            assert r["scratch"] == 0, (name, r)                 # only the many-band multiples spill
    assert B.violations(table) == []


def test_library_generated_code_is_clean_and_the_main_library_untouched():
    from isochrones_amd.csrc import build as main, isa_check
    from isochrones_amd.csrc.libraries import NESTED as B
    path = _built()
    assert isa_check.scan_library(path, jobs=1) == []
    assert not any("nested" in os.path.basename(s) for s in main.sources())
    assert B.OBJDIR != main.OBJDIR and B.RESOURCES != main.RESOURCES and B.STAMP != main.STAMP


def test_library_argument_errors_without_a_gpu():
    _built()
    from isochrones_amd import _nested_cabi as NC
    L = NC.lib()
    size = L.iso_nested_fast_args_size()
    assert size > 100
    blob = ctypes.create_string_buffer(size)                    # all zero: not a catalog's block
    rows = (ctypes.c_double * 64)()
    gidx = (ctypes.c_int64 * 1)(0)
    base = dict(fa=blob, size=size, kind=0, ns=1, nb=3, n=1, gidx=gidx, nlive=100, rows=rows)

    def call(**kw):
        a = dict(base, **kw)
        return L.iso_nested_fit(a["fa"], a["size"], a["kind"], a["ns"], a["nb"], a["n"], a["gidx"], a["nlive"], 0.5, 1.5, 0, 1000,
                                16, 1024, a["rows"], None, None, 0, None, None, 0, None)
    assert call(fa=None) == -1 and b"NULL" in L.iso_nested_last_error()
    assert call(rows=None) == -1 and call(gidx=None) == -1
    assert call(size=size - 8) == -1 and b"size" in L.iso_nested_last_error()
    assert call(kind=0, ns=2) == -1 and call(nb=13) == -1 and call(nb=0) == -1 and call(ns=4) == -1
    assert call(nlive=19) == -1 and b"n_live" in L.iso_nested_last_error()
    assert call(n=0) == -1
    assert call() == -1 and b"corner-packed" in L.iso_nested_last_error()       # the zero block is refused before any launch
    with pytest.raises(NC.IsoError):
        NC.check(call(fa=None))
    # the cap: the largest n_live whose buffers fit 160 KB, monotone in the shape, and enforced
    cap = L.iso_nested_max_live(1, 12, 2000)
    assert L.iso_nested_max_live(1, 3, 2000) > cap > L.iso_nested_max_live(3, 12, 2000) > 100
    assert L.iso_nested_max_live(1, 12, 6144) < cap
    assert L.iso_nested_max_live(0, 3, 100) == -1 and L.iso_nested_max_live(1, 13, 100) == -1
    D, K = 5, L.iso_nested_remove(cap, 1)
    lds = lambda n, k: 8 * (2000 + 256 * 13 + 256 + 64 + 128 + 256 + 3 * k + k * (D + 1) + 2 * n * (D + 1))
    assert lds(cap, K) <= 160 * 1024 < lds(cap + 1, L.iso_nested_remove(cap + 1, 1))
    assert L.iso_nested_remove(1000, 1) == 100 and L.iso_nested_remove(24, 1) == 2 and L.iso_nested_remove(40, 3) == 4
    assert K == T.remove_per_step(cap, D)


def test_fast_args_export_refuses_bad_arguments():
    """NULL arguments, then the size: the size is compared before the catalog is looked at, so a stand-in handle shows the
    branch without a GPU (the full path on a real catalog: tests/test_gpu_nested_catalog.py)."""
    from isochrones_amd import _cabi, _nested_cabi as NC
    _built()
    L = _cabi.lib()
    size = int(NC.lib().iso_nested_fast_args_size())
    buf = ctypes.create_string_buffer(size)
    kind = ctypes.c_int(-1)
    assert L.iso_catalog_fast_args(None, buf, size, None, None, None) == -1 and b"NULL" in L.iso_last_error()
    handle = ctypes.create_string_buffer(4096)                  # never read: the size check comes first
    assert L.iso_catalog_fast_args(handle, None, size, None, None, None) == -1 and b"NULL" in L.iso_last_error()
    for wrong in (size - 8, size + 8, 0):
        assert L.iso_catalog_fast_args(handle, buf, wrong, ctypes.byref(kind), None, None) == -1
        assert b"size" in L.iso_last_error() and kind.value == -1 and buf.raw == bytes(size)


def test_python_argument_checks_need_no_gpu():
    import isochrones_amd as ia
    ic = ia.synthetic_track(bands=("V", "J"), fehs=[-1, 0], masses=[0.8, 1.0, 1.2], eeps=np.arange(300., 340.))
    import pandas as pd
    df = pd.DataFrame({"V_mag": [10.0], "V_mag_unc": [0.02], "J_mag": [9.0], "J_mag_unc": [0.02]}, index=["s"])
    cat = ia.StarCatalog(df, bands=["V", "J"])
    with pytest.raises(ValueError, match="n_live_points"):
        ia.fit_stars_nested_gpu(cat, ic, [0], n_live_points=10)
    with pytest.raises(ValueError, match="method"):
        ia.fit_catalog(cat, ic, method="other")
    with pytest.raises(ValueError, match="return_dead"):
        ia.fit_catalog(cat, ic, method="nested", return_dead=True)
    assert ia.fit_stars_nested_gpu(cat, ic, [], n_live_points=50).shape == (0, 18)
    names = ("mass", "eep", "feh", "distance", "AV")
    cols = ia.nested_result_columns(names)
    assert len(cols) == 18 and cols[:2] == ["mass_mean", "mass_std"] and cols[-8:] == ["lnZ", "lnZ_err", "H", "ncall", "niter", "prior_fraction", "status", "ok"]


# ---- 5. an MCMC shard's digest is what it was ----
def test_mcmc_shard_digest_is_unchanged(tmp_path):
    """The digest of a fixed small catalog under fit_catalog's default method, as the code before method= computed it
    (tests/golden/nested_mcmc_digest.json, data); a nested shard's digest differs from it."""
    import isochrones_amd as ia
    from isochrones_amd import catalog as cat_mod
    import pandas as pd
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "nested_mcmc_digest.json")))
    ic = ia.synthetic_track(bands=("V", "J", "K"), fehs=np.array([-1.0, -0.5, 0.0, 0.5]), masses=np.array([0.7, 0.9, 1.0, 1.1, 1.3, 2.0]),
                            eeps=np.arange(300.0, 420.0), limits=dict(mass=(0.7, 2.0), feh=(-1.0, 0.5), age=(5, 10.13)), eep_bounds=(300, 419))
    rng = np.random.default_rng(5)
    n = 6
    df = pd.DataFrame({"V_mag": 10 + rng.random(n), "V_mag_unc": np.full(n, 0.02), "J_mag": 9 + rng.random(n), "J_mag_unc": np.full(n, 0.02),
                       "K_mag": 8.5 + rng.random(n), "K_mag_unc": np.full(n, 0.03), "parallax": 5 + rng.random(n), "parallax_unc": np.full(n, 0.1)},
                      index=["star%02d" % i for i in range(n)])
    cat = ia.StarCatalog(df, bands=["V", "J", "K"], props=["parallax"])
    mine = np.arange(n)
    kw = dict(nwalkers=32, nburn=20, niter=10, seed=3)
    assert cat_mod._shard_fingerprint(cat, mine, 1, kw, ic) == gold["digest"]
    # ... and it is the digest fit_catalog stores next to a shard, with the default method and with method="mcmc"
    fake = lambda catalog, ic, idx, N=1, **k: np.zeros((len(idx), 18))
    for sub, extra in (("a", {}), ("b", dict(method="mcmc"))):
        out = ia.fit_catalog(cat, ic, fit_fn=fake, checkpoint_dir=str(tmp_path / sub), **kw, **extra)
        assert list(out.columns) == cat_mod.result_columns(ic.param_names)
        with np.load(tmp_path / sub / "shard_0of1.npz") as z:
            assert str(z["digest"]) == gold["digest"]
    assert cat_mod._shard_fingerprint(cat, mine, 1, dict(kw, method="nested"), ic) != gold["digest"]
