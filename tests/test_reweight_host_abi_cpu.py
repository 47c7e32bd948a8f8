"""libiso_reweight.so's host entry through ctypes, no GPU needed: iso_reweight_stars_host against the long-double twin within
the twin's limits (quantiles exactly), the anchor cases that need no tolerance, the conjugate-Gaussian shrinkage check and
the arguments it refuses."""
import ctypes as C

import numpy as np
import pytest

from isochrones_amd import _cabi, _hier_cabi as hc, _reweight_cabi as rc
from isochrones_amd.csrc.libraries import HIER as build_hier, REWEIGHT as build_reweight
from tests import _reweight_twin as tw


@pytest.fixture(scope="module")
def lib():
    build_hier.build()
    build_reweight.build()
    return rc.lib()


#: (S, W, T, Q, H, V, layout): the device test's sample counts, with H through one and several row tiles
SHAPES = [(3, 1, 1, 1, 1, 1, 1), (3, 3, 7, 2, 8, 2, 1), (2, 8, 8, 4, 9, 8, 0), (2, 16, 16, 3, 29, 3, 1), (2, 257, 1, 1, 8, 2, 0),
          (2, 3, 257, 4, 9, 1, 1), (2, 32, 100, 2, 29, 5, 1), (2, 3, 7, 4, 150, 2, 1)]


@pytest.mark.parametrize("S, W, T, Q, H, V, layout", SHAPES)
def test_host_matches_the_twin(lib, S, W, T, Q, H, V, layout):
    case = tw.random_case(S, W, T, Q, H, V, seed=W + T + Q + H, layout=layout, probs=tw.PROBS8 if V == 8 else tw.PROBS3)
    code, got = tw.call(lib, case)
    assert code == 0, lib.iso_reweight_last_error()
    want = tw.want(case)
    assert (want["wsum"] > 0).all() and (want["n_bad"] == 0).all()
    # ln_norm = ell: the weights average to one per row
    assert np.max(np.abs(got["wsum"] / (H * W * T) - 1.0)) <= 1e-10
    tw.assert_matches(got, want, (S, W, T, Q, H, V))


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_interim_and_as_row(lib, kind):
    case = tw.kind_case(kind)
    code, got = tw.call(lib, case)
    assert code == 0, lib.iso_reweight_last_error()
    assert (tw.want(case)["wsum"] > 0).all()
    tw.assert_matches(got, tw.want(case), kind)


def test_special_cases(lib):
    res = {}
    for name, case in tw.special_cases().items():
        code, got = tw.call(lib, case)
        assert code == 0, lib.iso_reweight_last_error()
        tw.assert_matches(got, tw.want(case), name)
        res[name] = (case, got)
    case, g = res["one_dead_row"]
    assert np.isneginf(case["ln_norm"][0, 1]) and np.isfinite(case["ln_norm"][1]).all()
    assert abs(g["wsum"][1] / 35 - 1.0) < 1e-12 and abs(g["wsum"][0] / 35 - 2.0) < 1e-12      # one live row, two live rows
    case, g = res["all_dead_rows"]
    assert np.isneginf(case["ln_norm"][:, 1]).all()
    assert g["wsum"][1] == 0.0 and g["ess"][1] == 0.0 and (g["weights"][1] == 0.0).all()
    assert np.isnan(g["mean"][1]).all() and np.isnan(g["sd"][1]).all() and np.isnan(g["quant"][1]).all()
    assert np.isfinite(g["quant"][[0, 2]]).all()
    case, g = res["bad_and_nan"]
    assert list(g["n_bad"]) == [1, 0, 2] and g["weights"][0, 3] == 0.0 and g["weights"][2, 7] == 0.0 == g["weights"][2, 11]
    assert g["n_nan"].tolist() == [[2, 0], [0, 35], [0, 1]]
    assert np.isnan(g["mean"][1, 1]) and np.isnan(g["quant"][1, 1]).all() and np.isfinite(g["mean"][1, 0])
    case, g = res["masked"]
    assert np.isnan(g["wsum"][1]) and np.isnan(g["ess"][1]) and g["n_bad"][1] == 0 and (g["n_nan"][1] == 0).all()
    assert np.isnan(g["mean"][1]).all() and np.isnan(g["quant"][1]).all() and (g["weights"][1] == -7.0).all()


@pytest.mark.parametrize("W, T", [(3, 7), (37, 1), (3, 257)])
def test_unit_weights_are_numpy_s_inverted_cdf(lib, W, T):
    """rows equal to the interim record and ln_norm = ell: every u is exactly 1.0, ess = M, and the quantiles are
    numpy.percentile(method="inverted_cdf") bit for bit (p * M is no integer at these M)"""
    M = W * T
    y = np.random.default_rng(M).normal(size=(3, 2, M))
    case = tw.unit_case(y, W, T, probs=tw.PROBS8)
    assert not np.any(np.abs(np.round(tw.PROBS8 * M) - tw.PROBS8 * M) < 1e-9)
    code, got = tw.call(lib, case)
    assert code == 0 and (case["ln_norm"] == 0.0).all()
    assert (got["weights"] == 1.0).all() and (got["ess"] == M).all() and (got["wsum"] == M).all()
    want = np.percentile(y, 100 * tw.PROBS8, axis=2, method="inverted_cdf").transpose(2, 1, 0)     # [S, V, K]
    assert got["quant"].tobytes() == want.tobytes()
    tw.assert_matches(got, tw.want(case), (W, T))


@pytest.mark.parametrize("H", [2, 4, 8, 64, 128])
def test_equal_rows_multiply_the_weight_exactly(lib, H):
    tw.check_equal_rows(lib, None, H)


def test_integer_weights_and_ties(lib):
    """integer weights: every sum is exact, so ties in C(y) >= p * tot are decided as the definition says"""
    rng = np.random.default_rng(2)
    W, T = 4, 10
    M = W * T
    u = rng.integers(0, 5, (1, M))
    y = np.stack([rng.integers(0, 6, (1, M)).astype(float), rng.normal(size=(1, M)), np.full((1, M), 2.75)])
    probs = np.array([0.5, 0.25, 0.1, 0.75, 1.0 / u.sum(), 0.999])
    case = tw.integer_case(y, u, W, T, probs)
    code, got = tw.call(lib, case)
    assert code == 0, lib.iso_reweight_last_error()
    assert np.array_equal(got["weights"], u.astype(float)) and got["wsum"][0] == u.sum()
    assert got["ess"][0] == u.sum() ** 2 / (u * u).sum()
    tw.assert_matches(got, tw.want(case), "integer", exact=True)
    # the definition, in integers
    for v in range(3):
        for k, p in enumerate(probs):
            ys = np.unique(y[v, 0][u[0] > 0])
            cdf = np.array([u[0][y[v, 0] <= val].sum() for val in ys])
            assert got["quant"][0, v, k] == ys[np.flatnonzero(cdf >= p * u.sum())[0]], (v, p)
    assert (got["quant"][0, 2] == 2.75).all() and got["sd"][0, 2] == 0.0 and got["mean"][0, 2] == 2.75


@pytest.mark.parametrize("M", [21, 64, 771])
def test_every_radix_digit_decides(lib, M):
    y = tw.digit_values(M, seed=M)
    case = tw.unit_case(y, M, 1, probs=tw.PROBS8)
    code, got = tw.call(lib, case)
    assert code == 0 and (got["weights"] == 1.0).all()
    for v in range(4):
        want = np.percentile(y[v, 0] + 0.0, 100 * tw.PROBS8, method="inverted_cdf")
        assert np.array_equal(got["quant"][0, v], want), v
    assert len(set(got["quant"][0, 0])) >= 7
    tw.assert_matches(got, tw.want(case), M, exact=True)


def test_ranges_and_storages(lib):
    """a sub-range of the stars, and value columns from a storage that holds a slice of them (`first`), leave every star's
    numbers as they are and the other stars alone"""
    case = tw.random_case(5, 3, 7, 2, 9, 3, seed=4, layout=_cabi.CHAIN_ROW_MAJOR)
    code, full = tw.call(lib, case)
    assert code == 0
    code, part = tw.call(lib, case, ens_begin=1, n_ens_out=3, value_range=(1, 4))
    assert code == 0, lib.iso_reweight_last_error()
    for k, a in part.items():
        assert np.array_equal(a[1:4], full[k][1:4]), k
        assert (a[[0, 4]] == -7).all(), k
    code, sub = tw.call(lib, case, values=[2], probs=[0.84])
    assert code == 0 and np.array_equal(sub["quant"][:, 0, 0], full["quant"][:, 2, 2])
    assert np.array_equal(sub["mean"][:, 0], full["mean"][:, 2]) and np.array_equal(sub["weights"], full["weights"])


def test_shrinkage_to_the_conjugate_posterior(lib):
    """a Gaussian population N(0, 1) over stars observed with error 0.5: every star's weighted mean lies within
    5 * sd_post / sqrt(ess) of obs / 1.25 and its sd within 20 % of sqrt(0.2) (seed 3, host entry: the worst star is at
    2.94 of the 5 and 3.7 % of the 20 %; the smallest ess is 428)"""
    case, obs = tw.shrinkage_case()
    code, got = tw.call(lib, case)
    assert code == 0, lib.iso_reweight_last_error()
    sd_post = np.sqrt(0.2)
    ratio = np.abs(got["mean"][:, 0] - obs / 1.25) / (sd_post / np.sqrt(got["ess"]))
    off = np.abs(got["sd"][:, 0] / sd_post - 1.0)
    print("worst mean ratio %.2f of 5, worst sd offset %.3f of 0.2, min ess %.0f" % (ratio.max(), off.max(), got["ess"].min()))
    assert (ratio <= 5.0).all() and (off <= 0.2).all()
    assert (got["n_bad"] == 0).all() and np.max(np.abs(got["wsum"] / 3200 - 1.0)) <= 1e-10


def test_refused_arguments(lib):
    case = tw.random_case(3, 3, 7, 2, 3, 2, seed=3)
    assert tw.call(lib, case)[0] == 0
    msg = lambda: (lib.iso_reweight_last_error() or b"").decode()
    for kw, text in ((dict(probs=[0.5, 0.0]), "outside (0, 1)"), (dict(probs=[1.0]), "outside (0, 1)"),
                     (dict(probs=[np.nan]), "outside (0, 1)"), (dict(probs=np.linspace(0.1, 0.9, 9)), "K must be 1 to 8"),
                     (dict(probs=[]), "K must be 1 to 8"), (dict(values=[]), "V must be 1 to 8"),
                     (dict(values=[0, 1] * 5), "V must be 1 to 8"), (dict(ens_begin=2, n_ens_out=2), "ensemble range"),
                     (dict(ens_begin=0, n_ens_out=3, value_range=(1, 2)), "does not hold the ensembles"),
                     (dict(rows=case["rows"][:0], ln_norm=np.zeros((1, 3))), "H must be")):
        code, _ = tw.call(lib, case, **kw)
        assert code == rc.ERR_INVALID and text in msg() and msg().startswith("iso_reweight_stars_host: "), (kw, msg())
    # Q out of range, null pointers and a bad layout, on the raw entry; the device entry refuses the same before it
    # touches a device
    x = np.zeros((7, 2, 9))
    cols = (hc.IsoHierColumn * 5)(*[hc.IsoHierColumn(x.ctypes.data, 2, 0, 3, 0)] * 5)
    rec, ln, pr = np.zeros(8 * 72, np.uint8), np.zeros((1, 3)), np.array([0.5])
    outs = [np.zeros(3 * 21), np.zeros(3), np.zeros(3), np.zeros(3, np.int32), np.zeros(3), np.zeros(3), np.zeros(3),
            np.zeros(3, np.int32)]
    p = lambda a: C.c_void_p(a.ctypes.data)

    def run(fn, Q=1, layout=1, weights=True):
        o = [p(a) for a in outs]
        if not weights:
            o[0] = None
        return fn(cols, Q, cols, 1, layout, 7, 3, 3, 0, 3, p(rec), p(rec), 1, p(ln), None, pr.ctypes.data_as(C.POINTER(C.c_double)),
                  1, *o, None)

    for fn, who in ((lib.iso_reweight_stars_host, "iso_reweight_stars_host: "), (lib.iso_reweight_stars, "iso_reweight_stars: ")):
        for kw, text in ((dict(Q=0), "Q must be 1 to 4"), (dict(Q=5), "Q must be 1 to 4"), (dict(layout=2), "unknown chain layout"),
                         (dict(weights=False), "null pointer")):
            assert run(fn, **kw) == rc.ERR_INVALID and text in msg() and msg().startswith(who), (kw, msg())
