"""libiso_binned.so's host entries through ctypes, no GPU needed: iso_binned_compress_host and iso_binned_lnlike_host against
the long-double twin of tests/_binned_twin.py within its limits, the bin rule at the edges, the out and bad samples, the
special heights, masked stars, `extra`, every refusal with its message, and the identity with iso_hier_lnlike_host on FLAT
records of the bins."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _binned_cabi as bc, _hier_cabi as hc, hierarchical as hi, priors as P
from isochrones_amd.csrc.libraries import BINNED as build_binned, HIER as build_hier
from tests import _binned_twin as bt, _hier_twin as tw

PM, RM = bt.PM, bt.RM


@pytest.fixture(scope="module")
def lib():
    build_binned.build()
    return bc.lib()


def _err(lib):
    return lib.iso_binned_last_error().decode() if isinstance(lib.iso_binned_last_error(), bytes) else str(lib.iso_binned_last_error())


@pytest.mark.parametrize("S, W, T, n_bins, H, layout, n_frozen, extra", [
    (3, 5, 7, (4,), 3, PM, 1, False), (2, 16, 16, (1,), 1, RM, 0, False), (3, 7, 11, (64,), 9, PM, 2, True),
    (3, 5, 7, (3, 5), 8, RM, 1, False), (2, 8, 9, (8, 8), 17, PM, 2, True), (2, 4, 5, (2, 1), 2, PM, 0, False)])
def test_host_entries_match_the_twin(lib, S, W, T, n_bins, H, layout, n_frozen, extra):
    case = bt.make_case(S, W, T, n_bins, H, seed=3 + H + W, layout=layout, n_frozen=n_frozen, extra=extra)
    tab, out = bt.run(lib, case)
    worst = bt.assert_tables_match(tab, case, (S, W, T, n_bins))
    print("tables against the twin: worst |d| / limit = %.3f" % worst)
    assert (tab["n_out"] > 0).any() and np.isfinite(out["ell"]).any()
    bt.assert_matches(out, case, (S, W, T, n_bins, H))
    # the contraction alone, from the library's own tables in long double
    ref = bt.lnlike(tab, case["lnh"], W * T)
    assert np.allclose(out["ell"], ref["ell"], rtol=0, atol=1e-11, equal_nan=True)


def test_the_bin_rule_and_nonuniform_edges(lib):
    edges = np.array([0.0, 0.5, 2.0, 2.25, 4.0])
    below, above = np.nextafter(0.0, -1.0), np.nextafter(4.0, 5.0)
    x = np.array([[0.0, 0.5, np.nextafter(0.5, 0.0), 2.0, 2.25, 4.0, np.nextafter(4.0, 0.0), below, above, -3.0, 1.0, 3.0]])
    case = bt.one_axis_case(x, edges, W=3, T=4)
    rc, tab = bt.call_compress(lib, case)
    assert rc == 0, _err(lib)
    # flat interim prior of width 200: every weight is the same, exp(c - mx) = 1, so A counts the samples of a bin
    assert tab["A"][:, 0].tolist() == [2.0, 2.0, 1.0, 4.0] and tab["A2"][:, 0].tolist() == [2.0, 2.0, 1.0, 4.0]
    assert np.array_equal(tab["A"][:, 0], np.histogram(x[0], edges)[0])
    assert tab["n_out"][0] == 3 and tab["n_bad"][0] == 0 and tab["mx"][0] == -np.log(1.0 / 200.0)
    bt.assert_tables_match(tab, case)


def test_out_and_bad_samples_are_counted_once(lib):
    rng = np.random.default_rng(1)
    S, W, T = 3, 5, 7
    case = bt.make_case(S, W, T, (3, 2), 2, seed=4, n_frozen=1)
    x = case["x"].copy()
    a0, a1, fz = case["axes"][0], case["axes"][1], case["frozen_cols"][0]
    x[a0, 0, 3], x[a1, 0, 3] = 99.0, 0.9                             # out on both axes (inside the interim priors): once
    x[a0, 0, 4] = np.nan                                            # NaN on an axis: bad, not out
    x[a0, 1, 5] = 99.0
    x[fz, 1, 5] = np.nan                                            # out and bad: bad
    x[fz, 2, :] = np.nan                                            # every sample bad
    case = bt.replace_x(case, x)
    tab, out = bt.run(lib, case)
    bt.assert_tables_match(tab, case)
    want = bt.want(case)["tab"]
    assert tab["n_bad"][2] == W * T and tab["n_out"][2] == 0 and np.isneginf(tab["mx"][2]) and not tab["A"][:, 2].any()
    assert np.isneginf(out["ell"][:, 2]).all() and (out["ess"][:, 2] == 0).all()
    assert tab["n_bad"][0] == want["n_bad"][0] >= 1 and tab["n_bad"][1] >= 1
    bt.assert_matches(out, case)


def test_a_star_with_every_sample_out(lib):
    x = np.stack([np.linspace(5.0, 6.0, 12), np.linspace(0.1, 0.9, 12)])
    case = bt.one_axis_case(x, [0.0, 0.5, 1.0], W=3, T=4, lnh=[[0.1, -0.2]])
    tab, out = bt.run(lib, case)
    assert tab["n_out"].tolist() == [12, 0] and np.isneginf(tab["mx"][0]) and not tab["A"][:, 0].any()
    assert np.isneginf(out["ell"][0, 0]) and out["ess"][0, 0] == 0.0 and np.isfinite(out["ell"][0, 1])
    assert np.isneginf(out["L"][0]) and out["min_ess"][0] == 0.0
    bt.assert_matches(out, case)


def test_heights_of_zero(lib):
    rng = np.random.default_rng(2)
    x = rng.uniform(0.0, 3.0, (2, 35))
    x[1] = rng.uniform(0.0, 1.0, 35)                                 # star 1 lies in bin 0 alone
    lnh = np.array([[0.0, -np.inf, 0.3], [-np.inf, 0.2, 0.1], [-np.inf, -np.inf, -np.inf], [np.nan, 0.0, np.nan]])
    case = bt.one_axis_case(x, [0.0, 1.0, 2.0, 3.0], W=5, T=7, lnh=lnh)
    tab, out = bt.run(lib, case)
    assert np.isfinite(out["ell"][0]).all() and np.isfinite(out["ell"][1, 0]) and np.isneginf(out["ell"][1, 1])
    assert np.isneginf(out["ell"][2]).all() and (out["ess"][2] == 0).all() and np.isneginf(out["L"][2])
    assert np.isfinite(out["ell"][3, 0]) and np.isneginf(out["ell"][3, 1])          # a NaN height is a height of 0
    bt.assert_matches(out, case)
    rc, _ = bt.call_lnlike(lib, tab, [[0.0, np.inf, 0.0]], 35)
    assert rc == bc.ERR_INVALID and "+inf" in _err(lib)


def test_masked_stars_and_ranges(lib):
    case = bt.make_case(3, 5, 7, (4,), 3, seed=9, mask=[1, 0, 1])
    tab, out = bt.run(lib, case)
    assert np.isnan(tab["mx"][1]) and not tab["A"][:, 1].any() and not tab["A2"][:, 1].any()
    assert tab["n_bad"][1] == 0 and tab["n_out"][1] == 0
    assert np.isnan(out["ell"][:, 1]).all() and np.isnan(out["ess"][:, 1]).all() and np.isfinite(out["L"]).all()
    bt.assert_tables_match(tab, case)
    bt.assert_matches(out, case)
    none = dict({k: v for k, v in case.items() if k != "want"}, mask=np.zeros(3, np.int32))
    _, o = bt.run(lib, none)
    assert (o["L"] == 0.0).all() and np.isposinf(o["min_ess"]).all()
    # a sub-range writes its stars and leaves the rest alone
    rc, part = bt.call_compress(lib, case, ens_begin=2, n_ens_out=1)
    assert rc == 0 and (part["A"][:, :2] == -7.0).all() and (part["mx"][:2] == -7.0).all() and (part["n_out"][:2] == -7).all()
    assert part["A"][:, 2].tobytes() == tab["A"][:, 2].tobytes() and part["mx"][2] == tab["mx"][2]
    rc, po = bt.call_lnlike(lib, tab, case["lnh"], 35, case["mask"], ens_begin=0, n_ens_out=1, total=False)
    assert rc == 0 and (po["ell"][:, 1:] == -7.0).all() and (po["L"] == -7.0).all()
    assert po["ell"][:, 0].tobytes() == out["ell"][:, 0].tobytes()


def test_extra(lib):
    x = np.full((1, 8), 0.5)
    extra = np.array([-np.inf, 0.0, -0.0, 2.0, np.nan, -1.0, -2.0, np.nextafter(0.0, 1.0)])
    case = bt.one_axis_case(x, [0.0, 1.0], W=2, T=4, extra=extra, lnh=[[0.0]])
    tab, out = bt.run(lib, case)
    assert tab["n_bad"][0] == 3 and tab["n_out"][0] == 0              # positive (twice) and NaN; -inf is a good sample of weight 0
    want = np.exp(0.0) * 2 + np.exp(-1.0) + np.exp(-2.0)
    assert tab["mx"][0] == -np.log(1.0 / 200.0) and abs(tab["A"][0, 0] - want) < 1e-14
    bt.assert_tables_match(tab, case)
    bt.assert_matches(out, case)


REFUSALS = [
    (dict(n_bins=[65]), "more than 64 cells"), (dict(n_bins=[9, 8], n_axes=2, axis_col=[0, 1], n_frozen=0), "more than 64 cells"),
    (dict(n_axes=3, axis_col=[0, 1, 1], n_bins=[2, 2, 2]), "1 or 2 binned axes"), (dict(n_axes=0), "1 or 2 binned axes"),
    (dict(frozen_col=[0, 1], n_frozen=2), "both as a binned axis and as frozen"),
    (dict(frozen_col=[], n_frozen=0), "neither a binned axis nor frozen"),
    (dict(axis_col=[0, 0], n_axes=2, n_bins=[2, 2]), "binned axis twice"), (dict(axis_col=[2]), "no column"),
    (dict(n_bins=[0]), "at least 1 bin"),
    (dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(layout=7), "unknown chain layout"),
    (dict(T=0), "at least 1"), (dict(T=(2 ** 31 - 1) // 3), "2^31 - 257 samples"), (dict(T=2 ** 30), "2^31 - 257 samples"),
    (dict(edges=[0.0, 1.0, 1.0, 2.0, 3.0]), "finite and strictly increasing"),
    (dict(edges=[0.0, 1.0, np.inf, 3.0, 4.0]), "finite and strictly increasing"),
    (dict(edges=[0.0, np.nan, 2.0, 3.0, 4.0]), "finite and strictly increasing"),
]


@pytest.mark.parametrize("over, message", REFUSALS)
def test_refusals(lib, over, message):
    case = bt.make_case(2, 3, 4, (4,), 1, seed=1, n_frozen=1)          # Q = 2: column 0 binned, column 1 frozen
    assert bt.call_compress(lib, case)[0] == 0
    rc, tab = bt.call_compress(lib, case, **over)
    assert rc == bc.ERR_INVALID and message in _err(lib), _err(lib)
    assert _err(lib).startswith("iso_binned_compress_host: ") and (tab["A"] == -7.0).all()


def test_refused_ranges_and_records(lib):
    case = bt.make_case(2, 3, 4, (4,), 1, seed=1, n_frozen=1)
    for kw in (dict(ens_begin=2, n_ens_out=1), dict(ens_begin=0, n_ens_out=0), dict(ens_begin=1, n_ens_out=2)):
        assert bt.call_compress(lib, case, **kw)[0] == bc.ERR_INVALID and "ensemble range" in _err(lib)
    cols = [(k, nc, col, 1, 1) for k, nc, col in case["where"]]
    assert bt.call_compress(lib, case, cols=cols)[0] == bc.ERR_INVALID and "does not hold the ensembles" in _err(lib)
    bad = dict(case, frozen=case["frozen"].copy())
    bad["frozen"]["kind"][1] = 9
    assert bt.call_compress(lib, bad)[0] == bc.ERR_INVALID and "kinds 1 to 8" in _err(lib)
    _, tab = bt.call_compress(lib, case)
    for kw, message in ((dict(B=65), "1 to 64 cells"), (dict(B=0), "1 to 64 cells"), (dict(ens_begin=2), "ensemble range")):
        assert bt.call_lnlike(lib, tab, case["lnh"], 12, **kw)[0] == bc.ERR_INVALID and message in _err(lib)
    assert bt.call_lnlike(lib, tab, case["lnh"], 0)[0] == bc.ERR_INVALID and "M must be" in _err(lib)
    assert bt.call_lnlike(lib, tab, case["lnh"][:0], 12)[0] == bc.ERR_INVALID and "H must be" in _err(lib)
    fn = lib.iso_binned_lnlike_host
    a = C.c_void_p(tab["A"].ctypes.data)
    assert fn(a, a, a, 4, 2, 0, 2, 12, a, 1, None, a, a, a, None, None) == bc.ERR_INVALID and "go together" in _err(lib)
    assert fn(None, a, a, 4, 2, 0, 2, 12, a, 1, None, a, a, None, None, None) == bc.ERR_INVALID and "null pointer" in _err(lib)


@pytest.mark.parametrize("K", [1, 3])
def test_identity_with_the_hierarchical_library(lib, K):
    """ell of a histogram row equals logsumexp_b(lnh_b + ln width_b + ell_b), ell_b from iso_hier_lnlike_host on the FLAT
    record of bin b (whose ln f is -ln width_b), and ess follows from the bins' sums; the samples lie off the interior
    edges, where FLAT (closed on both sides) and the bin rule differ."""
    build_hier.build()
    hlib = hc.lib()
    rng = np.random.default_rng(K)
    S, W, T = 3, 5, 7
    M = W * T
    edges = np.array([0.0, 4.0]) if K == 1 else np.array([0.0, 0.7, 2.5, 4.0])
    x = rng.uniform(-0.5, 4.5, (1, S, M))
    x[0, 0, :2] = edges[0], edges[-1]                                # the outer edges are in both
    f = rng.uniform(0.2, 3.0, (1, S, M))                             # a frozen column next to it
    xs = np.concatenate([x, f])
    interim = [P.GaussianPrior(2.0, 1.5), P.FlatPrior((0.1, 10.0))]
    pop = P.PowerLawPrior(-2.35, (0.1, 10.0))
    H = 4
    lnh = bt.random_lnh(rng, H, K)
    case = dict(x=xs, interim=np.concatenate([hi.prior_record(p) for p in interim]),
                frozen=np.concatenate([hi.records(1), hi.prior_record(pop)]), frozen_cols=(1,), axes=(0,), edges=[edges], S=S, W=W,
                T=T, layout=PM, mask=None, extra=None, lnh=lnh)
    case["storages"], case["where"] = tw.place(xs, W, T, PM, 0)
    _, got = bt.run(lib, case)
    flat = tw.fixed_case(xs, interim, [[P.FlatPrior((edges[b], edges[b + 1])), pop] for b in range(K)], W, T)
    rc, ref = tw.call(hlib, flat)
    assert rc == 0
    with np.errstate(all="ignore"):
        terms = lnh[:, :, None] + np.log(np.diff(edges))[None, :, None] + ref["ell"][None, :, :]      # [H, K, S]
        top = terms.max(axis=1)
        want = top + np.log(np.exp(terms - top[:, None, :]).sum(axis=1))
        # a bin's sums from its (ell, ess): S1_b = M exp(ell_b), S2_b = S1_b^2 / ess_b, each times the row's height
        s1 = np.exp(terms - top[:, None, :])
        s2 = np.where(ref["ess"][None] > 0, s1 * s1 / ref["ess"][None], 0.0)
        ess = s1.sum(axis=1) ** 2 / s2.sum(axis=1)
    fin = np.isfinite(want)
    assert fin.any() and np.array_equal(np.isfinite(got["ell"]), fin)
    d = np.abs(got["ell"] - want)[fin]
    print("K = %d: max |d ell| = %.2e" % (K, d.max()))
    assert np.all(d <= 1e-11)
    assert np.all(np.abs(got["ess"] - ess)[fin] <= 1e-11 * ess[fin])
