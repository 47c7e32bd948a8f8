"""iso_select_alpha (k_select_partial, k_select_total) on the device against iso_select_alpha_host and the long-double
twin, within the limits of tests/_select_twin.py, on the smallest shapes at which the kernels can still go wrong: no full
wavefront (J = 1, 37), one pass of the workgroup exactly (256) and a partial second one (257), one chunk short by one
(4095), one chunk exactly (4096), two chunks (4097) and four with a ragged last one (3 * 4096 + 5), 65 and 257 chunks (a
second wavefront and a second pass of the total); H = 1, the row tile,
tile + 1 and 3 tiles + 5; Q = 1 and 4; every family kind; the -inf, NaN, zero-density and +-700 cases.  And bit identity
of a row alone, in any range or tiling of the rows, on a repeated call and from x at another address."""
import numpy as np
import pytest

from isochrones_amd import _hier_cabi as hc, _select_cabi as sc
from tests import _hier_twin as ht, _select_twin as tw

pytestmark = pytest.mark.gpu
TILE, CHUNK = sc.ROW_TILE, sc.CHUNK


@pytest.fixture(scope="module")
def lib():
    return sc.lib()


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _against_host(lib, device, case, what):
    rc, host = tw.call(lib, case)
    assert rc == 0, lib.iso_select_last_error()
    rc, got = tw.call(lib, case, device=device)
    assert rc == 0, lib.iso_select_last_error()
    twin = tw.want(case)
    tw.assert_matches(host, twin, what)
    fin = np.isfinite(host["ln_alpha"])
    if fin.any():
        print(what, "max |d ln_alpha| device - host = %.2e" % np.max(np.abs(got["ln_alpha"][fin] - host["ln_alpha"][fin])))
    tw.assert_matches(got, twin, what)
    tw.assert_matches(got, dict(host, tmax=twin["tmax"]), what)
    return got


SHAPES = [(J, Q, H) for J in (1, 37, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5) for Q in (1, 4)
          for H in (1, TILE, TILE + 1, 3 * TILE + 5)]


@pytest.mark.parametrize("J, Q, H", SHAPES)
def test_device_matches_the_host_entry_and_the_twin(lib, device, J, Q, H):
    case = tw.random_case(J, Q, H, seed=7 * Q + H + J)
    if J == 1:
        case["lnd"][:] = np.log(0.5)
    got = _against_host(lib, device, case, (J, Q, H))
    assert np.isfinite(got["ln_alpha"]).all() and got["n_bad"] == 0


@pytest.mark.parametrize("kind", range(1, 9))
def test_every_kind_as_draw_and_as_population(lib, device, kind):
    got = _against_host(lib, device, tw.kind_case(kind), kind)
    assert np.isfinite(got["ln_alpha"]).all()


@pytest.mark.parametrize("J", [300, CHUNK + 300])
def test_special_cases(lib, device, J):
    cases = tw.special_cases(J)
    keep, n_removed = cases.pop("bad_removed")
    res = {name: _against_host(lib, device, case, (name, J)) for name, case in cases.items()}
    g = res["none_detected"]
    assert np.isneginf(g["ln_alpha"]).all() and (g["n_eff"] == 0.0).all() and g["n_bad"] == 0
    assert res["bad"]["n_bad"] == n_removed and res["clean"]["n_bad"] == 0
    g = res["no_support"]
    assert np.isneginf(g["ln_alpha"][0]) and g["n_eff"][0] == 0.0 and np.isfinite(g["ln_alpha"][1])
    g = res["span_700"]
    assert tw.want(cases["span_700"])["tmax"].max() > 690 and np.isfinite(g["ln_alpha"]).all() and np.isfinite(g["n_eff"]).all()


def test_a_chunk_without_support_next_to_one_with(lib, device):
    """the second chunk's injections are all undetected (its partial is (-inf, 0, 0)); the third's all bad"""
    case = tw.random_case(2 * CHUNK + 100, 2, TILE + 1, seed=4)
    case["lnd"][CHUNK:2 * CHUNK] = -np.inf
    case["x"][1, 2 * CHUNK:] = np.nan
    got = _against_host(lib, device, case, "empty chunk")
    assert got["n_bad"] == 100 and np.isfinite(got["ln_alpha"]).all()


BLOCK = 256                                                         # threads of k_select_total's workgroup


def many_chunks_case(C, Q, H, bad_tail):
    """J = (C - 1) * CHUNK + 1 injections in C chunks, the last chunk the one injection J - 1.  Flat draws, Gaussian rows
    whose means and widths differ a little, so that r is largest near x = 0 under every row: injection J - 1 sits there
    with lnd = 0 and every other one has lnd <= -12, so it carries the largest term r + lnd of every row and a weight of
    the order of all the others' together.  A whole chunk in the middle and the injection J - 2 are undetected
    (lnd = -inf); an injection of chunk 0 and one of chunk 64 (where that is not the last) have a NaN x.  With ``bad_tail``
    injection J - 1 has a NaN x instead: the last chunk is without support, and its bad count is the last term of n_bad.
    Returns ``(case, n_bad)``."""
    from isochrones_amd import priors as P
    J = (C - 1) * CHUNK + 1
    rng = np.random.default_rng(C + Q + H)
    x = rng.uniform(-3.5, 3.5, (Q, J))
    x[:, J - 1] = 0.0
    lnd = tw._lnd(rng, J) - 12.0
    lnd[J - 1] = 0.0
    mid = C // 2
    lnd[mid * CHUNK:(mid + 1) * CHUNK] = -np.inf
    lnd[J - 2] = -np.inf
    nan_at = [(0, 5)] + ([(Q - 1, 64 * CHUNK + 7)] if C > 65 else []) + ([(0, J - 1)] if bad_tail else [])
    for q, j in nan_at:
        x[q, j] = np.nan
    mu, sg = rng.uniform(-0.2, 0.2, (H, Q)), rng.uniform(0.8, 1.2, (H, Q))
    case = tw.fixed_case(x, lnd, [P.FlatPrior((-4.0, 4.0))] * Q,
                         [[P.GaussianPrior(mu[h, q], sg[h, q]) for q in range(Q)] for h in range(H)])
    if not bad_tail:                                                # the largest term of every row is the last chunk's
        with np.errstate(invalid="ignore"):
            t = sum(-0.5 * ((x[q][None] - mu[:, q, None]) / sg[:, q, None]) ** 2 for q in range(Q)) + lnd[None]
        assert (np.nanmax(t[:, :J - 1], axis=1) < t[:, J - 1] - 11.0).all()
    return case, len(nan_at)


@pytest.mark.parametrize("bad_tail", [False, True])
@pytest.mark.parametrize("C, Q, H", [(BLOCK // 4 + 1, 4, 1), (BLOCK + 1, 1, TILE + 1)])
def test_the_total_over_more_chunks_than_a_wavefront_and_than_the_workgroup(lib, device, C, Q, H, bad_tail):
    """C = 65 chunks: the second wavefront of k_select_total has work.  C = 257: thread 0 takes a second chunk in each of
    the total's three loops (the maximum, the two sums, the bad counts).  Without the last chunk ln_alpha is off in
    its first decimal place, against a limit of 1e-11."""
    case, n_bad = many_chunks_case(C, Q, H, bad_tail)
    assert case["x"].shape == (Q, (C - 1) * CHUNK + 1)
    rc, host = tw.call(lib, case)
    assert rc == 0, lib.iso_select_last_error()
    rc, got = tw.call(lib, case, device=device, guard=True)
    assert rc == 0, lib.iso_select_last_error()
    assert not (got["ln_alpha"] == -7.0).any() and not (got["n_eff"] == -7.0).any()
    assert got["n_bad"] == host["n_bad"] == n_bad
    twin = tw.want(case)
    fin = np.isfinite(twin["ln_alpha"])
    assert fin.all()
    for name, res in (("host", host), ("device", got)):
        print("C = %d, Q = %d, H = %d, bad tail %s: %s against the twin, max |d ln_alpha| = %.2e, max |d n_eff| / n_eff = %.2e"
              % (C, Q, H, bad_tail, name, np.max(np.abs(res["ln_alpha"] - twin["ln_alpha"])),
                 np.max(np.abs(res["n_eff"] - twin["n_eff"]) / twin["n_eff"])))
    tw.assert_matches(got, twin, (C, "device"))
    tw.assert_matches(host, twin, (C, "host"))
    tw.assert_matches(got, dict(host, tmax=twin["tmax"]), (C, "device against host"))
    if bad_tail:
        return
    # the last injection weighs as much as the rest: far fewer effective injections than detected ones
    assert (got["n_eff"] < 1e-3 * case["x"].shape[1]).all()
    rc, again = tw.call(lib, case, device=device, guard=True)
    assert rc == 0 and all(again[k].tobytes() == got[k].tobytes() for k in ("ln_alpha", "n_eff")) and again["n_bad"] == n_bad
    if H > TILE:
        rc, one = tw.call(lib, case, device=device, rows=case["rows"][TILE:TILE + 1], guard=True)
        assert rc == 0 and one["n_bad"] == n_bad
        assert one["ln_alpha"].tobytes() == got["ln_alpha"][TILE:].tobytes() and one["n_eff"].tobytes() == got["n_eff"][TILE:].tobytes()


@pytest.fixture(scope="module")
def batch(lib, device):
    """four chunks with a ragged last one, 29 rows, three columns; evaluated once"""
    case = tw.random_case(3 * CHUNK + 5, 3, 3 * TILE + 5, seed=11)
    rc, got = tw.call(lib, case, device=device)
    assert rc == 0, lib.iso_select_last_error()
    return case, got


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_a_row_alone_and_in_any_range(lib, device, batch):
    case, whole = batch
    H = case["rows"].shape[0]
    for sl in (slice(0, 1), slice(TILE, TILE + 1), slice(H - 1, H), slice(5, 20), slice(3, 3 + TILE), slice(1, H)):
        rc, got = tw.call(lib, case, device=device, rows=case["rows"][sl])
        assert rc == 0 and _same(got["ln_alpha"], whole["ln_alpha"][sl]) and _same(got["n_eff"], whole["n_eff"][sl]), sl
        assert got["n_bad"] == whole["n_bad"]


def test_repeated_calls_and_another_address_give_the_same_bits(lib, device, batch):
    case, whole = batch
    for offset in (0, 0, 1, 37):                                    # x at another device address, 8-byte aligned only
        rc, got = tw.call(lib, case, device=device, x_offset=offset)
        assert rc == 0
        for k in ("ln_alpha", "n_eff"):
            assert _same(got[k], whole[k]), (k, offset)
        assert got["n_bad"] == whole["n_bad"]


@pytest.mark.parametrize("J, Q, H", [(300, 1, TILE + 1), (CHUNK + 1, 3, 3 * TILE + 5)])
def test_zero_one_detection_is_the_hier_kernel_on_the_one_star_chain(lib, device, J, Q, H):
    """ln_alpha = ell of the detected injections as one star's samples + ln(J_det / J), n_eff = its ess, from the device
    iso_hier_lnlike: twice the twin's limits, since the two results are rounded independently"""
    case = tw.random_case(J, Q, H, seed=J + Q)
    case["lnd"] = np.where(np.random.default_rng(J).random(J) < 0.6, 0.0, -np.inf)
    rc, got = tw.call(lib, case, device=device)
    assert rc == 0, lib.iso_select_last_error()
    hcase, shift = tw.one_star_chain(case)
    rc, old = ht.call(hc.lib(), hcase, device=device)
    assert rc == 0, hc.lib().iso_hier_last_error()
    want = dict(ln_alpha=old["ell"][:, 0] + shift, n_eff=old["ess"][:, 0], tmax=tw.want(case)["tmax"])
    assert old["n_bad"][0] == got["n_bad"] == 0 and np.isfinite(want["ln_alpha"]).all()
    tw.assert_matches(got, want, (J, Q, H), factor=2.0)
