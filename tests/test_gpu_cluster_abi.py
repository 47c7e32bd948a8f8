"""libiso_cluster.so through its C ABI against the long-double reference (tests/_cluster_hp.py).

Synthetic ABI inputs from a seeded generator go straight to iso_cluster_lnlike: there is no interpolation in the loop, so a
failure points at the kernels.  The cases cover the tile seams of the pairs kernel (64 stars per workgroup, secondaries in
blocks of 64), the stride of the finishing kernel (256), 1-32 bands (the >64 KB LDS launch at 32), 0-8 properties,
``n_valid`` outside ``[0, ld]``, and the operation's edges: ``fB`` of 0 and 1, ``m_k / m_j == minq`` exactly, non-monotone
masses, uneven EEP gaps, stars whose every cell underflows, NaN measurements."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import device as dev

from . import _cluster_hp as H

pytestmark = pytest.mark.gpu

#: |got - ref| <= TOL (1 + |ref|) for ln like_s and lnlike: float64 rounding of the binary magnitude, amplified by
#: delta / sigma^2 at sigma = 0.01, is about 4e-13 per cell and band
TOL = 1e-11
GUARD = 1024
SENTINEL_BITS = np.int64(0x7FF4DEADBEEF0001)          # a NaN payload no kernel writes
WORST = {}


# -- inputs -------------------------------------------------------------------------------------------------------------
def draw(seed, ns, nb, npr, n_valid, ld=None, kind="smooth", fB=None, minq=0.1, off=(), nan=()):
    """ABI inputs of one launch: every row is an isochrone of ``ld`` EEPs (filled to its clamped ``n_valid``, NaN past
    it, so a read past ``n_valid`` shows) and the stars are drawn near the longest row's isochrone.

    kind: "smooth" (integer EEPs, increasing mass), "gaps" (EEP steps of 0.4-5, not integers), "nonmono" (mass goes up
    and down: q > 1), "ties" (masses (i + 40) / 64 and minq = 0.5, so m_k / m_j == minq exactly in float64 at every
    other j).  off: stars moved 40 mag off the isochrone (every cell underflows); nan: stars with a NaN magnitude."""
    rng = np.random.default_rng(seed)
    n_valid = np.asarray(n_valid, dtype=np.int32)
    P = n_valid.size
    ld = int(max(1, n_valid.max())) if ld is None else ld
    fill = np.clip(n_valid, 0, ld)
    t = np.arange(ld) / max(ld - 1, 1)
    if kind == "gaps":
        eep = 150.0 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.4, 5.0, ld - 1))])
    else:
        eep = 150.0 + np.arange(ld, dtype=float)
    if kind == "ties":
        minq = 0.5
        mass = (np.arange(ld) + 40.0) / 64.0
    elif kind == "nonmono":
        mass = 0.5 + 0.8 * t + 0.15 * np.sin(6 * np.pi * t)
    else:
        mass = 0.3 + 0.9 * t ** 1.3
    lndm = np.log(0.01 + 0.005 * np.cos(3 * t))
    base = rng.uniform(6.0, 12.0, nb)
    color = rng.uniform(-0.5, 0.5, nb)
    mags = base[None, :] - 3.0 * (mass[:, None] - 0.3) + color[None, :] * t[:, None]          # [ld, nb]
    props = np.column_stack([np.sin((p + 1) * t) + 0.1 * p for p in range(npr)]) if npr else np.zeros((ld, 0))
    ncol = 3 + 2 * nb + npr
    cols = np.full((P, ncol, ld), np.nan)
    rowpar = np.empty((P, 4))
    for r in range(P):
        alpha, gamma = rng.uniform(-3.0, -2.0), rng.uniform(0.1, 0.5)
        fb = rng.uniform(0.2, 0.5) if fB is None else fB
        c, rp = H.row_columns(eep, mass, lndm, mags, props, alpha, gamma, fb, minq, 0.1, 300.0, ld)
        n = int(fill[r])
        cols[r][:, :n] = c[:, :n]
        rowpar[r] = rp
    # stars: a primary at EEP index j (and for a fraction fB, default 0.35, a secondary k <= j), sigma 0.01-0.03
    span = int(max(1, fill.max()))
    j = rng.integers(0, span, ns)
    k = (j * rng.uniform(0.3, 1.0, ns)).astype(int)
    binary = rng.random(ns) < (0.35 if fB is None else fB)
    flux = 10 ** (-0.4 * mags)
    obs = np.where(binary[:, None], -2.5 * np.log10(flux[j] + flux[k]), mags[j])
    unc = rng.uniform(0.01, 0.03, (ns, nb))
    obs = obs + unc * rng.standard_normal((ns, nb))
    for s in off:
        obs[s] += 40.0
    for s in nan:
        obs[s, int(rng.integers(0, nb))] = np.nan
    punc = rng.uniform(0.05, 0.2, (ns, npr))
    pobs = props[j] + punc * rng.standard_normal((ns, npr))
    star_val = np.ascontiguousarray(np.concatenate([obs.T, pobs.T]))
    star_w = np.ascontiguousarray(1.0 / np.concatenate([unc.T, punc.T]) ** 2)
    return dict(cols=cols, n_valid=n_valid, rowpar=rowpar, star_val=star_val, star_w=star_w, minq=float(minq), nb=nb,
                npr=npr, ld=ld, ns=ns, mass=mass)


def reference(a, minq=None):
    """(lnlike [P], ln like_s [P][N_s]) of the long-double reference, after checking the draw: every like_s is exactly 0 or
    above 1e-280, so no comparison is decided in the subnormal range."""
    tot, ln = H.lnlike(a["cols"], a["n_valid"], a["rowpar"], a["star_val"], a["star_w"],
                       a["minq"] if minq is None else minq, a["nb"], a["npr"])
    like = np.exp(ln)
    bad = (like != 0) & (like <= 1e-280)
    assert not bad.any(), "draw has like_s in (0, 1e-280]: %s" % np.argwhere(bad)[:5]
    return tot.astype(float), ln.astype(float)


# -- calls ---------------------------------------------------------------------------------------------------------------
def _guarded(n, torch, device):
    """A [n] view inside a buffer with GUARD sentinels on each side."""
    host = np.full(n + 2 * GUARD, SENTINEL_BITS, dtype=np.int64).view(np.float64)
    buf = torch.from_numpy(host).to(device)
    return buf, buf[GUARD:GUARD + n]


def call(a, device=0, star_terms=True, stream=None):
    """Run iso_cluster_lnlike on ``a`` (on ``stream``, default: the current one).  lnlike, lnlike_star and work live
    inside sentinel guard bands that must come back untouched.  Returns (lnlike [P], ln like_s [P][N_s] or None)."""
    import torch
    from isochrones_amd import _cluster_cabi as CC
    d = torch.device("cuda", device)
    P, ns, ld = a["n_valid"].size, a["ns"], a["ld"]
    with torch.cuda.device(device):
        def t(x, dt=torch.float64):
            return torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=d)
        cols, nv, rp, val, w = t(a["cols"]), t(a["n_valid"], torch.int32), t(a["rowpar"]), t(a["star_val"]), t(a["star_w"])
        lb, lnlike = _guarded(P, torch, d)
        sb, per_star = _guarded(P * ns, torch, d)
        wb, work = _guarded(P * ns * ld, torch, d)
        st = torch.cuda.current_stream(device) if stream is None else stream
        torch.cuda.current_stream(device).synchronize()              # inputs are ready before a side stream reads them
        CC.check(CC.lib().iso_cluster_lnlike(dev.ptr(cols), ld, P, dev.ptr(nv), dev.ptr(rp), dev.ptr(val), dev.ptr(w), ns,
                                             a["nb"], a["npr"], a["minq"], dev.ptr(work), dev.ptr(lnlike),
                                             dev.ptr(per_star) if star_terms else None, C.c_void_p(st.cuda_stream)))
        st.synchronize()
        out = {}
        for name, buf, n in (("lnlike", lb, P), ("lnlike_star", sb, P * ns), ("work", wb, P * ns * ld)):
            host = buf.cpu().numpy()
            bits = host.view(np.int64)
            assert np.all(bits[:GUARD] == SENTINEL_BITS) and np.all(bits[GUARD + n:] == SENTINEL_BITS), \
                "%s: a write outside its [%d] elements" % (name, n)
            out[name] = host[GUARD:GUARD + n]
    if not star_terms:
        assert np.all(out["lnlike_star"].view(np.int64) == SENTINEL_BITS), "lnlike_star is NULL but was written"
        return out["lnlike"], None
    return out["lnlike"], out["lnlike_star"].reshape(P, ns)


def close(got, want, what):
    """Same NaN / -inf / +inf pattern and |got - want| <= TOL (1 + |want|) elsewhere; returns the worst ratio."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    for kind, f in (("NaN", np.isnan), ("-inf", np.isneginf), ("+inf", np.isposinf)):
        assert np.array_equal(f(got), f(want)), (what, kind + " pattern", np.argwhere(f(got) != f(want))[:5])
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / (1 + np.abs(want[fin]))
    worst = float(err.max()) if err.size else 0.0
    WORST[what] = max(WORST.get(what, 0.0), worst)
    assert worst <= TOL, (what, worst)
    return worst


# -- the covering list ---------------------------------------------------------------------------------------------------
MIXED_NV = [0, 1, 2, 63, 64, 65, 127, 128, 129, -5, 500]           # one launch, ld = 130: -5 and 500 are clamped
CASES = {
    "1star_1band": dict(ns=1, nb=1, npr=0, n_valid=[66, 2]),
    "63stars": dict(ns=63, nb=2, npr=1, n_valid=[63]),
    "64stars": dict(ns=64, nb=3, npr=0, n_valid=[64]),
    "65stars": dict(ns=65, nb=3, npr=1, n_valid=[65]),
    "255stars": dict(ns=255, nb=2, npr=0, n_valid=[127]),
    "256stars": dict(ns=256, nb=1, npr=1, n_valid=[128]),
    "257stars": dict(ns=257, nb=2, npr=0, n_valid=[129]),
    "1000stars": dict(ns=1000, nb=3, npr=1, n_valid=[65, 64]),
    "mixed_n_valid": dict(ns=70, nb=3, npr=2, n_valid=MIXED_NV, ld=130),
    "200eeps": dict(ns=70, nb=3, npr=1, n_valid=[200, 199]),
    "16bands": dict(ns=65, nb=16, npr=0, n_valid=[70]),
    "31bands": dict(ns=64, nb=31, npr=0, n_valid=[66]),
    "32bands": dict(ns=65, nb=32, npr=0, n_valid=[129, 65]),
    "32bands_8props": dict(ns=20, nb=32, npr=8, n_valid=[80]),
    "8props_257stars": dict(ns=257, nb=2, npr=8, n_valid=[129, 128]),
    "fB0": dict(ns=64, nb=3, npr=0, n_valid=[70], fB=0.0),
    "fB1": dict(ns=64, nb=3, npr=0, n_valid=[70], fB=1.0),
    "ties": dict(ns=65, nb=2, npr=0, n_valid=[130], kind="ties"),
    "nonmonotone_mass": dict(ns=65, nb=3, npr=1, n_valid=[100], kind="nonmono"),
    "eep_gaps": dict(ns=64, nb=2, npr=1, n_valid=[90, 66], kind="gaps"),
    "underflow_star": dict(ns=65, nb=3, npr=0, n_valid=[70], off=(10,)),
    "nan_star": dict(ns=65, nb=3, npr=0, n_valid=[70], nan=(40,)),
    "nan_and_underflow": dict(ns=257, nb=2, npr=0, n_valid=[70], nan=(3,), off=(256,)),
    "ld_past_n_valid": dict(ns=64, nb=2, npr=1, n_valid=[66, 30], ld=200),
}
SEEDS = {name: 1000 + i for i, name in enumerate(CASES)}
_REF = {}


def case(name):
    a = draw(SEEDS[name], **CASES[name])
    if name not in _REF:
        _REF[name] = reference(a)
    return a, _REF[name]


def test_the_list_covers_the_seams():
    got = {k: set() for k in ("ns", "nv", "nb", "npr")}
    for c in CASES.values():
        got["ns"].add(c["ns"])
        got["nv"].update(c["n_valid"])
        got["nb"].add(c["nb"])
        got["npr"].add(c["npr"])
    assert {1, 63, 64, 65, 255, 256, 257, 1000} <= got["ns"]
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, -5, 500} <= got["nv"]
    assert {1, 2, 16, 31, 32} <= got["nb"] and {0, 1, 8} <= got["npr"]
    assert max(c["n_valid"][0] for c in CASES.values() if c["nb"] == 32) > 64
    assert min(c["n_valid"][0] for c in CASES.values() if c["npr"] == 8) > 64


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_long_double_reference(name):
    a, (tot, ln) = case(name)
    got, per_star = call(a)
    e1 = close(per_star, ln, "ln like_s")
    e2 = close(got, tot, "lnlike")
    print("%-20s worst |d|/(1+|ref|): ln like_s %.2e, lnlike %.2e" % (name, e1, e2))


def test_semantic_cases_are_what_they_say():
    a, (tot, ln) = case("underflow_star")
    assert np.all(ln[:, 10] == -np.inf) and np.isfinite(np.delete(ln, 10, axis=1)).all() and np.all(tot == -np.inf)
    a, (tot, ln) = case("nan_star")
    assert np.isnan(ln[:, 40]).all() and np.isfinite(np.delete(ln, 40, axis=1)).all() and np.isnan(tot).all()
    a, (tot, ln) = case("nan_and_underflow")
    assert np.isnan(ln[:, 3]).all() and np.all(ln[:, 256] == -np.inf) and np.all(tot == -np.inf)
    a, (tot, ln) = case("nonmonotone_mass")
    n = a["n_valid"][0]
    m = a["mass"][:n]
    assert np.any(np.tril(m[None, :] / m[:, None] > 1, -1)) and np.isfinite(tot).all()
    a, (tot, ln) = case("eep_gaps")
    d = np.diff(a["cols"][0, 0, :a["n_valid"][0]])
    assert d.max() > 3 and np.any(d != np.round(d))
    for name in ("fB0", "fB1"):
        a, (tot, ln) = case(name)
        assert np.isfinite(tot).all(), name
    a, (tot, ln) = case("mixed_n_valid")
    assert np.all(tot[[0, 1, 9]] == -np.inf) and np.isfinite(tot[[6, 7, 8, 10]]).all()   # n_valid 0, 1, -5: no pair
    assert np.all(np.isfinite(ln[3:9]).sum(axis=1) > 50)             # the seams carry finite stars


def test_exact_mass_ratio_ties_carry_a_visible_share():
    """m_k / m_j == minq in float64 at the cut of every other primary, and those cells move ln like_s by far more than the
    bar: a kernel that drops them (q <= minq) fails."""
    a, (tot, ln) = case("ties")
    n = a["n_valid"][0]
    m = a["mass"][:n]
    q = m[None, :] / m[:, None]
    assert np.count_nonzero(np.tril(q == a["minq"])) >= n // 3
    _, ln_cut = reference(a, minq=np.nextafter(a["minq"], 1.0))      # the same cut with the ties dropped
    assert np.isfinite(ln).all() and np.max(np.abs(ln_cut - ln)) > 1e3 * TOL


def test_rows_are_bitwise_the_same_alone_and_among_others():
    a, _ = case("mixed_n_valid")
    got, per_star = call(a)
    for r in range(a["n_valid"].size):
        one = dict(a, cols=a["cols"][r:r + 1], n_valid=a["n_valid"][r:r + 1], rowpar=a["rowpar"][r:r + 1])
        g1, s1 = call(one)
        assert g1.view(np.int64)[0] == got.view(np.int64)[r], r
        assert np.array_equal(s1[0].view(np.int64), per_star[r].view(np.int64)), r


def test_lnlike_is_bitwise_the_same_without_star_terms():
    for name in ("mixed_n_valid", "nan_and_underflow"):
        a, _ = case(name)
        got, _ = call(a)
        bare, none = call(a, star_terms=False)
        assert none is None and np.array_equal(got.view(np.int64), bare.view(np.int64)), name


def test_bitwise_the_same_on_a_side_stream():
    import torch
    a, _ = case("257stars")
    got, per_star = call(a)
    side = torch.cuda.Stream(device=0)
    g2, s2 = call(a, stream=side)
    assert np.array_equal(got.view(np.int64), g2.view(np.int64))
    assert np.array_equal(per_star.view(np.int64), s2.view(np.int64))


def test_32_bands_on_every_device():
    """The >64 KB LDS launch on device 0, then device 1: the LDS limit is a per-device function attribute."""
    import torch
    a, (tot, ln) = case("32bands")
    devices = list(range(min(2, torch.cuda.device_count())))
    if len(devices) < 2:
        pytest.skip("one device visible: the second-device launch cannot run")
    for d in devices:
        got, per_star = call(a, device=d)
        close(per_star, ln, "ln like_s")
        close(got, tot, "lnlike")


def test_zz_worst_error():
    """(last) the worst error of this module's comparisons against the long-double reference"""
    if not WORST:
        pytest.skip("no comparison ran")
    print("worst |got - ref| / (1 + |ref|): " + ", ".join("%s %.3e" % kv for kv in sorted(WORST.items())))
    assert max(WORST.values()) <= TOL
