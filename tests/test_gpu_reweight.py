"""iso_reweight_stars (k_reweight_weights, k_reweight_summary) on the device against iso_reweight_stars_host and the
long-double twin, within the limits of tests/_reweight_twin.py (quantiles exactly), on the smallest shapes at which the
kernels can still go wrong: M = 1, 21, 64 (no full workgroup), 256 (one pass of it exactly), 257 and 771 (a partial last
pass) and 3 200 (the catalog's 32 x 100); H = 1, 8, 9, 29 (one row tile), 150 (three tiles, the last ragged) and 1 024 with
Q = 4 (sixteen tiles); Q = 1 and 4, V = 1 and 8, K = 1 and 8; every family kind; both layouts, star ranges, `first`, masks;
the dead-row, bad-sample and NaN-value cases, ties and the values on which every radix digit decides.  Then the anchors that
need no tolerance, bit identity, and the conjugate-Gaussian shrinkage check."""
import numpy as np
import pytest

from isochrones_amd import _cabi, _hier_cabi as hc, _reweight_cabi as rc
from tests import _hier_twin as ht, _reweight_twin as tw

pytestmark = pytest.mark.gpu
OUT = ("weights", "wsum", "ess", "n_bad", "mean", "sd", "quant", "n_nan")


@pytest.fixture(scope="module")
def lib():
    return rc.lib()


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _against_host(lib, device, case, what, exact=False, **kw):
    code, host = tw.call(lib, case, **kw)
    assert code == 0, lib.iso_reweight_last_error()
    code, got = tw.call(lib, case, device=device, **kw)
    assert code == 0, lib.iso_reweight_last_error()
    twin = tw.want(case)
    live = host["weights"] > 0
    if live.any():
        print(what, "max rel d weights device - host = %.2e" % np.max(np.abs(got["weights"][live] / host["weights"][live] - 1.0)))
    tw.assert_matches(host, twin, what, exact=exact)
    tw.assert_matches(got, twin, what, exact=exact)
    assert np.array_equal(got["quant"], host["quant"], equal_nan=True), what
    return got


#: (S, W, T, Q, H, V, K, layout)
SHAPES = [(3, 1, 1, 1, 1, 1, 1, 1), (3, 1, 1, 4, 9, 8, 8, 0), (3, 3, 7, 4, 8, 8, 8, 1), (2, 3, 7, 1, 29, 1, 3, 0),
          (2, 8, 8, 1, 9, 8, 1, 0), (2, 8, 8, 4, 1, 1, 8, 1), (2, 16, 16, 4, 29, 3, 3, 1), (2, 16, 16, 1, 150, 2, 3, 0),
          (2, 257, 1, 1, 8, 2, 3, 0), (2, 257, 1, 4, 9, 8, 8, 1), (2, 3, 257, 4, 9, 1, 1, 1), (2, 3, 257, 1, 150, 8, 3, 0),
          (2, 32, 100, 4, 29, 5, 3, 1), (2, 32, 100, 1, 8, 8, 8, 0), (1, 3, 7, 4, 1024, 1, 1, 1)]


@pytest.mark.parametrize("S, W, T, Q, H, V, K, layout", SHAPES)
def test_device_matches_the_host_entry_and_the_twin(lib, device, S, W, T, Q, H, V, K, layout):
    probs = {1: [0.31], 3: tw.PROBS3, 8: tw.PROBS8}[K]
    case = tw.random_case(S, W, T, Q, H, V, seed=W + T + Q + H + V, layout=layout, probs=probs)
    got = _against_host(lib, device, case, (S, W, T, Q, H, V, K))
    assert (got["wsum"] > 0).all() and (got["n_bad"] == 0).all()
    # ln_norm = ell of the device's own iso_hier_lnlike: the weights average to one per row
    code, hier = ht.call(hc.lib(), case, device=device, total=False)
    assert code == 0
    code, own = tw.call(lib, case, device=device, ln_norm=hier["ell"])
    assert code == 0 and np.max(np.abs(own["wsum"] / (H * W * T) - 1.0)) <= 1e-10


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_interim_and_as_row(lib, device, kind):
    got = _against_host(lib, device, tw.kind_case(kind), kind)
    assert (got["wsum"] > 0).all()


def test_special_cases(lib, device):
    res = {name: _against_host(lib, device, case, name) for name, case in tw.special_cases().items()}
    g = res["all_dead_rows"]
    assert g["wsum"][1] == 0.0 and g["ess"][1] == 0.0 and (g["weights"][1] == 0.0).all()
    assert np.isnan(g["mean"][1]).all() and np.isnan(g["sd"][1]).all() and np.isnan(g["quant"][1]).all()
    g = res["one_dead_row"]
    assert abs(g["wsum"][1] / 35 - 1.0) < 1e-12 and abs(g["wsum"][0] / 35 - 2.0) < 1e-12
    g = res["bad_and_nan"]
    assert list(g["n_bad"]) == [1, 0, 2] and g["n_nan"].tolist() == [[2, 0], [0, 35], [0, 1]]
    assert g["weights"][0, 3] == 0.0 and np.isnan(g["quant"][1, 1]).all()
    g = res["masked"]
    assert np.isnan(g["wsum"][1]) and np.isnan(g["ess"][1]) and g["n_bad"][1] == 0 and (g["n_nan"][1] == 0).all()
    assert np.isnan(g["mean"][1]).all() and np.isnan(g["quant"][1]).all() and (g["weights"][1] == -7.0).all()


@pytest.mark.parametrize("W, T", [(3, 7), (37, 1), (3, 257)])
def test_unit_weights_are_numpy_s_inverted_cdf(lib, device, W, T):
    M = W * T
    y = np.random.default_rng(M).normal(size=(3, 2, M))
    case = tw.unit_case(y, W, T, probs=tw.PROBS8)
    code, got = tw.call(lib, case, device=device)
    assert code == 0 and (case["ln_norm"] == 0.0).all()
    assert (got["weights"] == 1.0).all() and (got["ess"] == M).all() and (got["wsum"] == M).all()
    want = np.percentile(y, 100 * tw.PROBS8, axis=2, method="inverted_cdf").transpose(2, 1, 0)
    assert got["quant"].tobytes() == want.tobytes()
    tw.assert_matches(got, tw.want(case), (W, T))


@pytest.mark.parametrize("H", [2, 4, 8, 64, 128])
def test_equal_rows_multiply_the_weight_exactly(lib, device, H):
    tw.check_equal_rows(lib, device, H)


def test_integer_weights_and_ties(lib, device):
    rng = np.random.default_rng(2)
    W, T = 4, 10
    M = W * T
    u = rng.integers(0, 5, (1, M))
    y = np.stack([rng.integers(0, 6, (1, M)).astype(float), rng.normal(size=(1, M)), np.full((1, M), 2.75)])
    probs = np.array([0.5, 0.25, 0.1, 0.75, 1.0 / u.sum(), 0.999])
    got = _against_host(lib, device, tw.integer_case(y, u, W, T, probs), "integer", exact=True)
    assert np.array_equal(got["weights"], u.astype(float)) and got["wsum"][0] == u.sum()
    assert got["ess"][0] == u.sum() ** 2 / (u * u).sum()
    assert (got["quant"][0, 2] == 2.75).all() and got["sd"][0, 2] == 0.0 and got["mean"][0, 2] == 2.75


@pytest.mark.parametrize("M", [21, 64, 771])
def test_every_radix_digit_decides(lib, device, M):
    y = tw.digit_values(M, seed=M)
    got = _against_host(lib, device, tw.unit_case(y, M, 1, probs=tw.PROBS8), M, exact=True)
    assert (got["weights"] == 1.0).all()
    for v in range(4):
        assert np.array_equal(got["quant"][0, v], np.percentile(y[v, 0] + 0.0, 100 * tw.PROBS8, method="inverted_cdf")), v
    assert len(set(got["quant"][0, 0])) >= 7


def test_bit_identity(lib, device):
    """a star alone, in a batch, in any star range, from either layout and from columns at another address; a value column
    alone and among eight; a repeated call"""
    S, W, T, Q, H, V = 5, 16, 17, 3, 70, 8
    case = tw.random_case(S, W, T, Q, H, V, seed=9, probs=tw.PROBS8)
    code, full = tw.call(lib, case, device=device)
    assert code == 0, lib.iso_reweight_last_error()
    code, again = tw.call(lib, case, device=device)
    assert code == 0 and all(again[k].tobytes() == full[k].tobytes() for k in OUT)
    code, moved = tw.call(lib, case, device=device, offset=37)
    assert code == 0 and all(moved[k].tobytes() == full[k].tobytes() for k in OUT)
    other = tw.random_case(S, W, T, Q, H, V, seed=9, layout=_cabi.CHAIN_ROW_MAJOR, probs=tw.PROBS8)
    assert np.array_equal(other["x"], case["x"]) and np.array_equal(other["y"], case["y"])
    code, rowmajor = tw.call(lib, other, device=device)
    assert code == 0 and all(rowmajor[k].tobytes() == full[k].tobytes() for k in OUT)
    for s0, n in ((0, 1), (2, 1), (4, 1), (1, 3), (3, 2)):
        code, part = tw.call(lib, case, device=device, ens_begin=s0, n_ens_out=n, value_range=(s0, n))
        assert code == 0, lib.iso_reweight_last_error()
        for k in OUT:
            assert part[k][s0:s0 + n].tobytes() == full[k][s0:s0 + n].tobytes(), (k, s0, n)
            rest = np.delete(part[k], np.arange(s0, s0 + n), axis=0)
            assert (rest == -7).all(), (k, s0, n)
    for v in (0, 3, 7):
        code, one = tw.call(lib, case, device=device, values=[v])
        assert code == 0
        for k in ("mean", "sd", "n_nan", "quant"):
            assert one[k][:, 0].tobytes() == np.ascontiguousarray(full[k][:, v]).tobytes(), (k, v)
        assert one["weights"].tobytes() == full["weights"].tobytes()
    code, onep = tw.call(lib, case, device=device, probs=[tw.PROBS8[5]])
    assert code == 0 and np.array_equal(onep["quant"][:, :, 0], full["quant"][:, :, 5])
    tw.assert_matches(full, tw.want(case), "bit identity")


def test_shrinkage_to_the_conjugate_posterior(lib, device):
    """as tests/test_reweight_host_abi_cpu.py: 200 stars x 32 x 100 samples at seed 3, on the device"""
    case, obs = tw.shrinkage_case()
    code, got = tw.call(lib, case, device=device)
    assert code == 0, lib.iso_reweight_last_error()
    sd_post = np.sqrt(0.2)
    ratio = np.abs(got["mean"][:, 0] - obs / 1.25) / (sd_post / np.sqrt(got["ess"]))
    off = np.abs(got["sd"][:, 0] / sd_post - 1.0)
    print("worst mean ratio %.2f of 5, worst sd offset %.3f of 0.2, min ess %.0f" % (ratio.max(), off.max(), got["ess"].min()))
    assert (ratio <= 5.0).all() and (off <= 0.2).all()
    assert (got["n_bad"] == 0).all() and np.max(np.abs(got["wsum"] / 3200 - 1.0)) <= 1e-10


def test_star_posteriors_on_a_device_chain_with_derived_columns():
    """PopulationPosterior.star_posteriors / star_weights on a CUDA chain of a track grid: `age` (a model column) and
    `radius` (a value column only) are derived on the device.  Against the host entry on the same chain with the derived
    columns copied in as parameters; budget slicing changes no bit."""
    import torch
    import isochrones_amd as ia
    from isochrones_amd import priors as P
    ic = ia.synthetic_track(bands=("V", "J", "K"), fehs=np.array([-1.0, -0.5, 0.0, 0.5]),
                            masses=np.array([0.7, 0.9, 1.0, 1.1, 1.3, 2.0]), eeps=np.arange(300.0, 420.0),
                            limits=dict(mass=(0.7, 2.0), feh=(-1.0, 0.5), age=(5, 10.13)), eep_bounds=(300, 419))
    names = tuple(ic.param_names)
    assert names[:3] == ("mass", "eep", "feh") and len(names) == 5
    rng = np.random.default_rng(12)
    S, W, T = 9, 8, 13
    centre = np.stack([rng.uniform(0.95, 1.7, S), rng.uniform(330.0, 390.0, S), rng.uniform(-0.7, 0.25, S), np.full(S, 100.0),
                       np.full(S, 0.2)], axis=1)
    chain = centre[:, None, None, :] + np.array([0.05, 5.0, 0.05, 3.0, 0.02]) * rng.normal(size=(S, W, T, 5))
    dchain = torch.from_numpy(chain).cuda()
    model = ia.PopulationModel(mass=ia.PowerLaw((0.7, 2.0)), age=ia.TruncatedGaussian((5.0, 10.15)))
    interim = {"mass": P.PowerLawPrior(-2.35, (0.7, 2.0)), "age": P.FlatPrior((5.0, 10.15))}
    mask = np.ones(S, dtype=np.int32)
    mask[2] = 0
    theta = np.array([[-2.0, 8.0, 0.6], [-1.0, 7.8, 0.9], [-2.6, 8.3, 0.5]])
    post = ia.PopulationPosterior((dchain, names), ic, model, interim=interim, mask=mask)
    assert post.derived_cols == ["age"]
    cols = ["mass", "feh", "age", "radius"]
    df = post.star_posteriors(theta, columns=cols)
    extra, _ = ia.chain_derived(dchain, ic, ("age", "radius"))
    wide = np.concatenate([chain, extra.cpu().numpy()], axis=3)
    assert np.isfinite(wide).all()
    host = ia.PopulationPosterior((wide, names + ("age", "radius")), None, model, interim=interim, mask=mask)
    want = host.star_posteriors(theta, columns=cols)
    assert list(df.columns) == list(want.columns) and df.loc[2, [c for c in df.columns if c != "n_bad"]].isna().all()
    live = np.flatnonzero(mask)
    for c in df.columns:
        g, w = df[c].to_numpy()[live], want[c].to_numpy()[live]
        if c.endswith(("_median", "_p16", "_p84")) or c == "n_bad":
            assert np.array_equal(g, w), c
        else:
            assert np.all(np.abs(g - w) <= 1e-10 * np.maximum(np.abs(w), 1.0)), c
    # the default columns: the chain's parameters, then the model's derived column
    default = post.star_posteriors(theta, as_tensors=True)
    assert [k for k in default if k.endswith("_mean")] == [n + "_mean" for n in names + ("age",)]
    assert default["age_median"].is_cuda and np.array_equal(default["age_median"].cpu().numpy(), df["age_median"].to_numpy(),
                                                            equal_nan=True)
    w = post.star_weights(theta, stars=[4, 0])
    hw = host.star_weights(theta, stars=[4, 0])
    assert w.is_cuda and w.shape == (2, W * T) and np.max(np.abs(w.cpu().numpy() - hw)) <= 1e-11 * hw.max()
    # slices of two stars (the model's derived column, radius and the weights: three doubles a sample)
    cut = ia.PopulationPosterior((dchain, names), ic, model, interim=interim, mask=mask, budget_bytes=2 * 3 * W * T * 8)
    from isochrones_amd import reweight as rw
    assert [n for _, n in rw._slices(cut, 1)] == [2, 2, 2, 2, 1]
    assert cut.star_posteriors(theta, columns=cols).equals(df)
    assert torch.equal(cut.star_weights(theta, stars=[4, 0]), w)
